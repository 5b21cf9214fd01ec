"""Measurement (not product): the rigid pre-alignment stage on the bench scenes.

Config 1 (320x224, 199 nodes) and config 3 (640x448, 1998 nodes): all of seq.canonical_points, the target at frame 20,
the nodes at the identity (what the stage meets at the start of a frame). Device events around `--reps` calls after a
warm-up, the two sides alternated in blocks, in one process:

  rigid       ofx_rigid_icp with `--iters` iterations per call (two launches each: gate + reduce, total + solve); the
              number reported is per iteration
  associate   one ofx_associate call on the same inputs (gate, scan, emit): the yardstick

plus the wall time (host clock around a synchronised call) of one Registration.track with 3 ICP iterations, with and
without rigid_iters=4. One JSON document on stdout and in --out.

    python tools/rigid_bench.py [--reps 100] [--out profiles/rigid_bench.json]
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
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--frame", type=int, default=20)
ap.add_argument("--configs", default="1,3")
ap.add_argument("--out", default=None)
ap.add_argument("--no-track", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "rigid_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_side(seq, config):
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    pts = torch.from_numpy(np.ascontiguousarray(seq.canonical_points, np.float32)).to(dev)
    nodes = torch.from_numpy(seq.nodes).to(dev)
    P, N = pts.shape[0], nodes.shape[0]
    an, wt, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    valid = v.to(torch.uint8)
    packed = pack_transforms(nodes, None, None, dev)
    vmap = backproject_depth_device(torch.from_numpy(seq.frame(a.frame)[5]).to(dev), *intr)
    M = 10000
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt, warped = torch.empty((P, 3), device=dev), torch.empty((P, 3), device=dev)
    midx = torch.empty(M, dtype=torch.int32, device=dev)
    so, to = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev)
    ao, wo = torch.empty((M, 4), dtype=torch.int32, device=dev), torch.empty((M, 4), device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    systems = torch.empty((a.iters, 32), dtype=torch.float64, device=dev)
    eye = torch.eye(3, 4, dtype=torch.float64, device=dev)
    pose = eye.clone()
    ha, hr = _lib.c_void_p(), _lib.c_void_p()
    call("ofx_assoc_create", P, byref(ha))
    call("ofx_rigid_create", P, byref(hr))
    camc = _lib.Camera(*intr, W, H)
    aprm = _lib.AssocParams(0.05, 0.5, 0.03, 1, M, 0)
    rprm = _lib.RigidParams(0.05, 0.5, 0.03, a.iters, 6, 1e-6, 0.0)
    s = stream_ptr()

    def assoc():
        call("ofx_associate", ha, ptr(pts), None, ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N, byref(camc), ptr(vmap),
             H, W, byref(aprm), ptr(code), ptr(tgt), ptr(warped), ptr(midx), ptr(so), ptr(to), ptr(ao), ptr(wo),
             ptr(count), s)

    def rigid():
        call("ofx_rigid_icp", hr, ptr(pts), None, ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N, byref(camc), ptr(vmap),
             H, W, byref(rprm), ptr(pose), ptr(code), ptr(systems), s)

    for _ in range(10):
        assoc()
        rigid()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    ms = {"assoc": [], "rigid": []}
    for _ in range(a.blocks):
        ms["assoc"].append(events_ms(assoc, per))
        ms["rigid"].append(events_ms(rigid, per))
    pose.copy_(eye)
    rigid()
    torch.cuda.synchronize()
    sysm = systems.cpu().numpy()
    _lib.lib.ofx_assoc_destroy(ha)
    _lib.lib.ofx_rigid_destroy(hr)
    us_a = [1e3 * x / per for x in ms["assoc"]]
    us_r = [1e3 * x / per / a.iters for x in ms["rigid"]]
    return {"config": config, "frame": a.frame, "points": P, "nodes": N, "image": [H, W], "iters_per_call": a.iters,
            "workgroups": (P + 255) // 256, "reps_per_block": per, "blocks": a.blocks,
            "rigid_us_per_iteration_blocks": us_r, "rigid_us_per_iteration": min(us_r),
            "associate_us_per_call_blocks": us_a, "associate_us_per_call": min(us_a),
            "rigid_iteration_over_associate": min(us_r) / min(us_a),
            "accepted_per_iteration": [int(x) for x in sysm[:, 28]], "status_per_iteration": [int(x) for x in sysm[:, 29]],
            "rms_mm_per_iteration": [float(1e3 * np.sqrt(r[27] / r[28])) if r[28] > 0 else None for r in sysm]}


def track_side(seq, config):
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.registration import Registration
    c = S.BASELINE_CONFIGS[config]
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
    res = {}
    for name, ri in (("track", 0), ("track_rigid4", 4)):
        t = []
        for _ in range(3):   # the first is the warm-up
            reg.prev_rot = reg.prev_trans = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = reg.track(frame, icp_iters=3, mode="plane", rigid_iters=ri)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        res[name + "_ms"] = min(t[1:])
        res[name + "_ms_runs"] = t
        res[name + "_accepted"] = [x["accepted"] for x in out["assoc"]]
        if ri:
            res["rigid_status"] = [int(x) for x in out["rigid"]["systems"][:, 29].cpu().tolist()]
    res.update(config=config, points=int(reg.source_pcd.shape[0]), nodes=int(seq.nodes.shape[0]))
    return res


doc = {"tool": "tools/rigid_bench.py", "device": torch.cuda.get_device_name(0), "kernel": [], "track": []}
for cfg in (int(x) for x in a.configs.split(",")):
    seq = S.config_sequence(cfg, device=dev)
    doc["kernel"].append(kernel_side(seq, cfg))
    if not a.no_track:
        doc["track"].append(track_side(seq, cfg))
txt = json.dumps(doc, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
