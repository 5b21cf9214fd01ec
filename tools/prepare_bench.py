"""Measurement (not product): depth-frame preparation (ofx_prepare_depth) on the bench cameras.

Config 1 (320x224) and config 3 (640x448), the sequence's own noisy frame 20. Device events around `--reps` calls after
a warm-up, the sides alternated in blocks, the best block kept:

  prepare r=2/3/4     ofx_prepare_depth with the normal map (sigma_s 2 px, sigma_r 1 cm, range_cut 3 cm): two launches
  prepare r=3 no-nrm  the same without the normal map: what icp_track(depth_filter=True) issues, one launch
  prepare r=0         no taps: the launches, the LDS staging and the 16-28 B/pixel of output alone
  prepare r=3 skipped on an image whose depths are distinct by >= 1 mm inside any 7x7 window, with range_cut 0.5 mm: every
                      tap but the centre is read from LDS, tested and skipped — the window's LDS reads and loop without
                      any f64 exp; r=3 minus this is what the exp and the sums cost
  yardsticks          ofx_backproject_depth alone, and one ofx_associate call of all of seq.canonical_points against the
                      raw frame's vertex map (the nodes at their ground-truth motion), in the same process

plus one Registration.track (config 1, 8229 points, precond="direct", frame 0 -> 20 from the identity, plane mode, 3 ICP
iterations: the scene of tests/test_gpu_prepare.py) with and without depth_filter=True: the residual against the raw
depth, the accepted shares and the wall time. One JSON document on stdout and in --out.

    python tools/prepare_bench.py [--reps 200] [--out profiles/prepare_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import assoc_ref as ar  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402
from occlusionfusion_amd.association import pack_transforms  # noqa: E402
from occlusionfusion_amd.image_proc import backproject_depth_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--blocks", type=int, default=4, help="the reps of each side are split into this many alternating blocks")
ap.add_argument("--frame", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--no-track", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "prepare_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_side(config):
    seq = S.config_sequence(config, device=dev)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    depth = torch.from_numpy(seq.frame(a.frame)[5]).to(dev)
    out, pimg, nimg = (torch.empty((H, W), device=dev), torch.empty((3, H, W), device=dev),
                       torch.empty((3, H, W), device=dev))
    vmap = torch.zeros((3, H, W), device=dev)
    camc = _lib.Camera(*intr, W, H)
    s = stream_ptr()

    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    distinct = (1.0 + 1e-3 * ((xx % 8) + 8 * (yy % 8)).float()).contiguous()   # no two equal depths in a 7x7 window

    def prep(radius, normals=True, cut=0.03, image=depth):
        prm = _lib.PrepareParams(radius, 2.0, 0.01, cut, 0.03, 1000.0)
        return lambda: call("ofx_prepare_depth", ptr(image), 0, H, W, byref(camc), byref(prm), ptr(out), ptr(pimg),
                            ptr(nimg) if normals else None, s)

    def backproject():
        call("ofx_backproject_depth", ptr(depth), 0, H, W, *intr, 1000.0, ptr(vmap), s)

    # the association yardstick: all canonical points, the nodes at their ground-truth motion (tools/assoc_bench.py)
    pts = torch.from_numpy(np.ascontiguousarray(seq.canonical_points, np.float32)).to(dev)
    nodes = torch.from_numpy(seq.nodes).to(dev)
    P, N = pts.shape[0], nodes.shape[0]
    an, wt, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    valid = v.to(torch.uint8)
    T = torch.from_numpy((seq.scene.deform_points(seq.nodes, a.frame) - seq.nodes).astype(np.float32)).to(dev)
    packed = pack_transforms(nodes, None, T, dev)
    M = 10000
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt, warped = torch.empty((P, 3), device=dev), torch.empty((P, 3), device=dev)
    midx = torch.empty(M, dtype=torch.int32, device=dev)
    so, to = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev)
    ao, wo = torch.empty((M, 4), dtype=torch.int32, device=dev), torch.empty((M, 4), device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    h = _lib.c_void_p()
    call("ofx_assoc_create", P, byref(h))
    aprm = _lib.AssocParams(0.05, 0.5, 0.03, 1, M, 0)
    backproject()

    def assoc():
        call("ofx_associate", h, ptr(pts), None, ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N, byref(camc), ptr(vmap),
             H, W, byref(aprm), ptr(code), ptr(tgt), ptr(warped), ptr(midx), ptr(so), ptr(to), ptr(ao), ptr(wo),
             ptr(count), s)

    sides = {"prepare_r2": prep(2), "prepare_r3": prep(3), "prepare_r4": prep(4),
             "prepare_r3_no_normals": prep(3, normals=False), "prepare_r0": prep(0),
             "prepare_r3_all_taps_skipped": prep(3, cut=5e-4, image=distinct), "backproject": backproject, "associate": assoc}
    for _ in range(10):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    ms = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, fn in sides.items():
            ms[k].append(events_ms(fn, per))
    torch.cuda.synchronize()
    _lib.lib.ofx_assoc_destroy(h)
    us = {k: [1e3 * x / per for x in v] for k, v in ms.items()}
    best = {k: min(v) for k, v in us.items()}
    px = H * W
    return {"config": config, "frame": a.frame, "image": [H, W], "pixels": px, "valid_pixels": int((depth > 0).sum()),
            "assoc_points": P, "reps_per_block": per, "blocks": a.blocks,
            "us_per_call": best, "us_per_call_blocks": us,
            "algorithmic_bytes_per_pixel": {"in": 4, "out_without_normals": 16, "out_with_normals": 28},
            "prepare_r3_gb_per_s": px * 32 / (best["prepare_r3"] * 1e-6) / 1e9,
            "prepare_r3_taps_per_s": px * 49 / (best["prepare_r3"] * 1e-6),
            "prepare_r3_over_backproject": best["prepare_r3"] / best["backproject"],
            "prepare_r3_no_normals_over_associate": best["prepare_r3_no_normals"] / best["associate"],
            "split_r3_us": {"launches_staging_output": best["prepare_r0"],
                            "window_lds_reads_and_loop": best["prepare_r3_all_taps_skipped"] - best["prepare_r0"],
                            "f64_exp_and_sums": best["prepare_r3"] - best["prepare_r3_all_taps_skipped"]}}


def track_side():
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.registration import Registration
    c = S.BASELINE_CONFIGS[1]
    seq = S.config_sequence(1, device=dev)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = c["dims"]
    vol = TSDFVolume.from_grid(c["origin"], c["voxel"], (D, D, D), intr, SimpleNamespace(source_frame=0, skip_rate=1),
                               device=dev)
    wf = WarpField(EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage), vol)
    cp = seq.canonical_points
    pts = cp[np.sort(np.random.default_rng(5).choice(cp.shape[0], 2 * 4096 + 37, replace=False))]
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(pts, wf.graph, wf, K, precond="direct")
    im = seq.frame(a.frame)
    depth = im[5]
    n_pts = int(reg.source_pcd.shape[0])
    res = {"config": 1, "frame": a.frame, "points": n_pts, "nodes": int(seq.nodes.shape[0]), "icp_iters": 3,
           "r_identity_mm": 1e3 * ar.depth_residual(reg.source_pcd.cpu().numpy(), depth, intr)}
    for name, filt in (("raw", None), ("filtered", True)):
        t = []
        for _ in range(3):   # the first is the warm-up
            reg.prev_rot = reg.prev_trans = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = reg.track({"im": im, "id": a.frame}, icp_iters=3, mode="plane", depth_filter=filt)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        res[name] = {"r_icp_mm": 1e3 * ar.depth_residual(out["warped_verts"].cpu().numpy(), depth, intr),
                     "accepted_shares": [x["accepted"] / n_pts for x in out["assoc"]],
                     "emitted": [x["emitted"] for x in out["assoc"]], "valid_solve": int(out["valid_solve"]),
                     "track_ms": min(t[1:]), "track_ms_runs": t}
    return res


doc = {"tool": "tools/prepare_bench.py", "device": torch.cuda.get_device_name(0),
       "kernel": [kernel_side(1), kernel_side(3)]}
if not a.no_track:
    doc["track"] = track_side()
txt = json.dumps(doc, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
