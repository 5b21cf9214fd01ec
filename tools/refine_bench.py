"""Measurement (not product): the sub-pixel refinement of the photometric matches on the default spin scene.

Config 1's camera (320x224), the spin scene's textured frames 0 (the template) and 1 (the live frame), all of
seq.canonical_points at the identity. ofx_photo_associate emits `rows` matches (3000 and 10 000; the second is capped by
what the search accepts); ofx_photo_refine then refines them. Device events around `--reps` calls after a warm-up, in
alternating blocks, the best block kept:

  refine h3 / h4   ofx_photo_refine at half 3 and 4 (iters 8, the defaults otherwise): one kernel
  photo r4         ofx_photo_associate (radius 4) on the same inputs: the context figure — there is nothing else to
                   compare the refinement with

The library under test is the one OFX_LIB names (default: the product). `--ab [LANES ...]` runs the measurement once per
lane mapping in a fresh child process each — the product (16 lanes per row) and tuning builds with -DOFX_REFINE_LANES=n
(default: 4 and 8), built on the spot under tools/ablib/ unless they are there already — and writes all of them into
one document.

    python tools/refine_bench.py [--reps 60] [--ab 4 8] [--out profiles/refine_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--rows", type=int, nargs="+", default=[3000, 10000])
ap.add_argument("--ab", type=int, nargs="*", default=None, metavar="LANES",
                help="also measure tuning builds with these OFX_REFINE_LANES (no value: 4 8), a fresh child process each")
ap.add_argument("--out", default=None)
a = ap.parse_args()


def tuning_lib(lanes):
    return os.path.join(ROOT, "tools", "ablib", f"libofx_refine{lanes}.so")


def finish(doc):
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if a.ab is not None:
    lanes = a.ab or [4, 8]
    for n in lanes:
        if not os.path.exists(tuning_lib(n)):
            from occlusionfusion_amd import build as B
            os.makedirs(os.path.dirname(tuning_lib(n)), exist_ok=True)
            B.build(out=tuning_lib(n), defines=(f"OFX_REFINE_LANES={n}",))
    doc = {"tool": "tools/refine_bench.py --ab " + " ".join(str(n) for n in lanes)}
    for name, lib in [("product", None)] + [(f"lanes{n}", tuning_lib(n)) for n in lanes]:
        env = dict(os.environ)
        env.pop("OFX_LIB", None)
        if lib:
            env["OFX_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--blocks", str(a.blocks), "--rows"] + \
            [str(r) for r in a.rows]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"refine_bench child ({name}) failed:\n{r.stdout}\n{r.stderr}")
        side = json.loads(r.stdout[r.stdout.index("{"):])
        doc["device"] = side["device"]
        doc[name] = side["kernel"]
    doc["us_over_product"] = {
        name: {f"rows{k['rows']}_{m}": k[m + "_us"] / kp[m + "_us"] for k, kp in zip(doc[name], doc["product"])
               for m in ("refine_h3", "refine_h4")}
        for name in (f"lanes{n}" for n in lanes)}
    finish(doc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402
from occlusionfusion_amd.association import pack_transforms  # noqa: E402
from occlusionfusion_amd.image_proc import prepare_depth_device  # noqa: E402

assert torch.cuda.is_available(), "refine_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_side(rows):
    c = S.BASELINE_CONFIGS[1]
    scene, seed = S.SphereScene(motion="spin", occluder=False), 1
    cam = S.bench_camera(c["cam_scale"])
    seq = S.SyntheticSequence.build(c["nodes"], cam=cam, seed=seed, coverage=c["coverage"], scene=scene,
                                    graph="geodesic", device=dev)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    im0, im1 = S.textured_frame(scene, cam, seed, 0), S.textured_frame(scene, cam, seed, 1)
    cp = np.ascontiguousarray(seq.canonical_points, np.float32)
    pts = torch.from_numpy(cp).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(im0[:3][:, im0[5] > 0].T)).to(dev)
    tpx_all = torch.from_numpy(np.stack([cp[:, 0] * cam.fx / cp[:, 2] + cam.cx,
                                         cp[:, 1] * cam.fy / cp[:, 2] + cam.cy], 1).astype(np.float32)).to(dev)
    nodes = torch.from_numpy(seq.nodes).to(dev)
    P, N = pts.shape[0], nodes.shape[0]
    an, wt, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    valid = v.to(torch.uint8)
    packed = pack_transforms(nodes, None, None, dev)
    prep = prepare_depth_device(torch.from_numpy(im1[5]).to(dev), *intr, radius=0, edge_max=0.03, normals=True)
    vmap, nmap = prep["point_image"], prep["normals"]
    cmap = torch.from_numpy(np.ascontiguousarray(im1[:3])).to(dev)
    tmap = torch.from_numpy(np.ascontiguousarray(im0[:3])).to(dev)
    M = int(rows)
    f, i = torch.float32, torch.int32
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt, warped = torch.empty((P, 3), device=dev), torch.empty((P, 3), device=dev)
    pixel, cost = torch.empty((P, 2), dtype=i, device=dev), torch.empty(P, dtype=f, device=dev)
    midx = torch.zeros(M, dtype=i, device=dev)
    so, to, po = torch.zeros((M, 3), device=dev), torch.zeros((M, 3), device=dev), torch.zeros((M, 2), device=dev)
    ao, wo = torch.zeros((M, 4), dtype=i, device=dev), torch.zeros((M, 4), device=dev)
    count = torch.empty(2, dtype=i, device=dev)
    h = _lib.c_void_p()
    call("ofx_assoc_create", P, byref(h))
    camc = _lib.Camera(*intr, W, H)
    pprm = _lib.PhotoParams(0.05, 0.5, float("inf"), 1.0, 4, M)
    s = stream_ptr()

    def photo():
        call("ofx_photo_associate", h, ptr(pts), None, ptr(col), ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N,
             byref(camc), ptr(vmap), ptr(nmap), ptr(cmap), H, W, byref(pprm), ptr(code), ptr(tgt), ptr(warped),
             ptr(pixel), ptr(cost), ptr(midx), ptr(so), ptr(to), ptr(ao), ptr(wo), ptr(po), ptr(count), s)
    photo()
    tpx = tpx_all[midx.long()].contiguous()
    px_o, tgt_o = torch.empty((M, 2), device=dev), torch.empty((M, 3), device=dev)
    status, ssd = torch.zeros(M, dtype=torch.uint8, device=dev), torch.empty(M, device=dev)

    def refine(half):
        rprm = _lib.RefineParams(half, 8, 1e-3, 4.0, 1e-6, float("inf"), 0.03, 0)

        def run():
            call("ofx_photo_refine", ptr(tmap), None, ptr(cmap), ptr(vmap), ptr(tpx), ptr(po), ptr(to), ptr(count), M, H,
                 W, byref(rprm), ptr(px_o), ptr(tgt_o), ptr(status), ptr(ssd), s)
        return run

    sides = {"refine_h3": refine(3), "refine_h4": refine(4), "photo_r4": photo}
    for fn in sides.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    us = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, fn in sides.items():
            us[k].append(1e3 * events_ms(fn, per) / per)
    sides["refine_h3"]()
    torch.cuda.synchronize()
    cnt = count.cpu().tolist()
    hist = torch.bincount(status[:cnt[1]].long(), minlength=8).cpu().tolist()
    _lib.lib.ofx_assoc_destroy(h)
    res = {"rows": M, "points": P, "image": [H, W], "emitted": cnt[1], "iters": 8, "reps_per_block": per,
           "blocks": a.blocks}
    for k, v in us.items():
        res[k + "_us_blocks"] = v
        res[k + "_us"] = min(v)
    res["h3_status_histogram"] = hist
    return res


finish({"tool": "tools/refine_bench.py", "library": os.path.relpath(_lib.LIB_PATH, ROOT),
        "device": torch.cuda.get_device_name(0), "kernel": [kernel_side(r) for r in a.rows]})
