"""Measurement (not product): projective data association on the bench scene.

Config 3's scene (640x448), all of seq.canonical_points (the backprojected source frame) with its 1998-node graph, the
target at frame 20, the nodes at their ground-truth motion. Device events around `--reps` calls after a warm-up, the two
sides alternated in blocks:

  associate   ofx_associate: the gate kernel, the scan's three launches and the emit — one number over the whole call
  yardstick   ofx_deform_points followed by ofx_visibility_f32 on the same points: the warp and the lookup as the two
              separate kernels the library had before

plus the wall time (host clock around a synchronised call) of one Registration.track with 3 ICP iterations at config 1
and config 3, next to one optimize on 10000 ground-truth matches. One JSON document on stdout and in --out.

    python tools/assoc_bench.py [--reps 100] [--out profiles/assoc_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402
from occlusionfusion_amd.association import pack_transforms  # noqa: E402
from occlusionfusion_amd.image_proc import backproject_depth_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--blocks", type=int, default=4, help="the reps of each side are split into this many alternating blocks")
ap.add_argument("--frame", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--no-track", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "assoc_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_side(config=3):
    seq = S.config_sequence(config, device=dev)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    pts = torch.from_numpy(np.ascontiguousarray(seq.canonical_points, np.float32)).to(dev)
    nodes = torch.from_numpy(seq.nodes).to(dev)
    P, N = pts.shape[0], nodes.shape[0]
    an, wt, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    valid = v.to(torch.uint8)
    c0, r0 = seq.scene.frame_params(0)   # the scene's own normals: the sphere's outward one, the plane's towards the camera
    cp = seq.canonical_points.astype(np.float64)
    n_np = np.where((cp[:, 2] < seq.scene.plane_z - 0.02)[:, None], (cp - c0) / r0, np.array([0.0, 0.0, -1.0]))
    n_np /= np.linalg.norm(n_np, axis=1, keepdims=True)
    nrm = torch.from_numpy(n_np.astype(np.float32)).to(dev)
    T = torch.from_numpy((seq.scene.deform_points(seq.nodes, a.frame) - seq.nodes).astype(np.float32)).to(dev)
    packed = pack_transforms(nodes, None, T, dev)
    depth = torch.from_numpy(seq.frame(a.frame)[5]).to(dev)
    vmap = backproject_depth_device(depth, *intr)
    M = 10000
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt, warped = torch.empty((P, 3), device=dev), torch.empty((P, 3), device=dev)
    midx = torch.empty(M, dtype=torch.int32, device=dev)
    so, to = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev)
    ao, wo = torch.empty((M, 4), dtype=torch.int32, device=dev), torch.empty((M, 4), device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    vis, dd = torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
    h = _lib.c_void_p()
    call("ofx_assoc_create", P, byref(h))
    camc = _lib.Camera(*intr, W, H)
    prm = _lib.AssocParams(0.05, 0.5, 0.03, 1, M, 0)
    s = stream_ptr()

    def assoc(normals=True):
        call("ofx_associate", h, ptr(pts), ptr(nrm) if normals else None, ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N,
             byref(camc), ptr(vmap), H, W, byref(prm), ptr(code), ptr(tgt), ptr(warped), ptr(midx), ptr(so), ptr(to),
             ptr(ao), ptr(wo), ptr(count), s)

    def pair():
        call("ofx_deform_points", ptr(pts), P, ptr(an), ptr(wt), ptr(valid), 4, ptr(packed), N, 0, ptr(warped), s)
        call("ofx_visibility_f32", ptr(warped), P, byref(camc), ptr(depth), 0.1, ptr(vis), ptr(dd), s)

    for _ in range(10):
        assoc()
        assoc(False)
        pair()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    ms = {"assoc": [], "assoc_no_normals": [], "pair": []}
    for _ in range(a.blocks):
        ms["assoc"].append(events_ms(assoc, per))
        ms["pair"].append(events_ms(pair, per))
        ms["assoc_no_normals"].append(events_ms(lambda: assoc(False), per))
    assoc()
    torch.cuda.synchronize()
    cnt = count.cpu().tolist()
    hist = torch.bincount(code.long(), minlength=7).cpu().tolist()
    _lib.lib.ofx_assoc_destroy(h)
    us = {k: [1e3 * x / per for x in v] for k, v in ms.items()}
    best = {k: min(v) for k, v in us.items()}
    # algorithmic bytes per point: 12 point + 12 normal + 16 anchors + 16 weights = 56 in (+ 1 valid); 4 x 64 B node
    # records and 5 x 12 B vertex-map pixels, gathered (L2); 1 code + 12 tgt + 12 warped = 25 out (+ 1 flag, + the emit's
    # 4 rank + up to 12 + 16 + 16 + 12 + 4 per emitted row: 37 with the rank and the flag's read-back spread over all)
    b_in, b_gather, b_out = 56 + 1, 4 * 64 + 5 * 12, 25 + 1 + 4 + 1
    return {"config": config, "frame": a.frame, "points": P, "nodes": N, "image": [H, W], "max_matches": M,
            "reps_per_block": per, "blocks": a.blocks,
            "associate_us_per_call_blocks": us["assoc"], "associate_us_per_call": best["assoc"],
            "associate_no_normals_us_per_call": best["assoc_no_normals"],
            "yardstick_deform_plus_visibility_us_blocks": us["pair"],
            "yardstick_deform_plus_visibility_us": best["pair"],
            "associate_over_yardstick": best["assoc"] / best["pair"],
            "points_per_second": P / (best["assoc"] * 1e-6),
            "algorithmic_bytes_per_point": {"streamed_in": b_in, "gathered_l2": b_gather, "out": b_out},
            "streamed_gb_per_s": P * (b_in + b_out) / (best["assoc"] * 1e-6) / 1e9,
            "gathered_gb_per_s": P * b_gather / (best["assoc"] * 1e-6) / 1e9,
            "accepted": cnt[0], "emitted": cnt[1], "code_histogram": hist}


def track_side(config):
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.registration import Registration
    c = S.BASELINE_CONFIGS[config]
    seq = S.config_sequence(config, device=dev)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = c["dims"]
    vol = TSDFVolume.from_grid(c["origin"], c["voxel"], (D, D, D), intr, SimpleNamespace(source_frame=0, skip_rate=1),
                               device=dev)
    wf = WarpField(EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage), vol)
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(seq.canonical_points, wf.graph, wf, K)
    frame = {"im": seq.frame(a.frame), "id": a.frame}
    src, tgt, tpos, conf = seq.solver_inputs(a.frame, 10000)
    an, wt, v = wf.skin_device(src)
    gt = (torch.from_numpy(src).to(dev)[v], an[v], wt[v], torch.from_numpy(tgt).to(dev)[v])

    def opt():
        return reg.solver.optimize(seq.nodes, seq.edges, seq.edge_weights, tpos, np.zeros_like(conf), gt[0], gt[1],
                                   gt[2], gt[3], intr)

    res = {}
    for name, fn in (("optimize", opt), ("track", lambda: reg.track(frame, icp_iters=3, mode="plane"))):
        t = []
        for _ in range(3):   # the first is the warm-up
            reg.prev_rot = reg.prev_trans = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        res[name + "_ms"] = min(t[1:])
        res[name + "_ms_runs"] = t
        if name == "track":
            res["assoc"] = out["assoc"]
            res["gn_iterations_last"] = out["convergence_info"]["gn_iterations"]
    res.update(config=config, points=int(reg.source_pcd.shape[0]), nodes=int(seq.nodes.shape[0]))
    return res


doc = {"tool": "tools/assoc_bench.py", "device": torch.cuda.get_device_name(0), "kernel": kernel_side(3)}
if not a.no_track:
    doc["track"] = [track_side(1), track_side(3)]
txt = json.dumps(doc, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
