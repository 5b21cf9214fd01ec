"""Measurement (not product): the photometric correspondence search on the bench scenes.

Config 1's (320x224) and config 3's (640x448) scene, all of seq.canonical_points with the config's graph at the identity,
model colours from the textured source frame, the target the textured frame `--frame`. Device events around `--reps`
calls after a warm-up, in alternating blocks, the best block kept:

  photo r4 / r8   ofx_photo_associate at radius 4 and 8: the search kernel, the scan's three launches and the emit —
                  one number over the whole call
  associate       ofx_associate on the same points and vertex map: the context figure

  ... shuffled    the same calls with the points in a random order: canonical_points are in pixel order, the friendliest
                  order there is for one thread per point; a model sampled from the volume comes in brick order

The library under test is the one OFX_LIB names (default: the product). `--ab [LANES ...]` runs the measurement once per
lane mapping in a fresh child process each — the product (8 lanes per point) and tuning builds with
-DOFX_PHOTO_LANES=n (default: 1, one thread per point), built on the spot under tools/ablib/ unless they are there
already — and writes all of them into one document.

    python tools/photo_bench.py [--reps 60] [--ab 1 4 8] [--out profiles/photo_bench.json]
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
ap.add_argument("--frame", type=int, default=2)
ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
ap.add_argument("--ab", type=int, nargs="*", default=None, metavar="LANES",
                help="also measure tuning builds with these OFX_PHOTO_LANES (no value: 1), a fresh child process each")
ap.add_argument("--out", default=None)
a = ap.parse_args()



def tuning_lib(lanes):
    return os.path.join(ROOT, "tools", "ablib", f"libofx_photo{lanes}.so")


def finish(doc):
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if a.ab is not None:
    lanes = a.ab or [1]
    for n in lanes:
        if not os.path.exists(tuning_lib(n)):
            from occlusionfusion_amd import build as B
            os.makedirs(os.path.dirname(tuning_lib(n)), exist_ok=True)
            B.build(out=tuning_lib(n), defines=(f"OFX_PHOTO_LANES={n}",))
    doc = {"tool": "tools/photo_bench.py --ab " + " ".join(str(n) for n in lanes)}
    for name, lib in [("product", None)] + [(f"lanes{n}", tuning_lib(n)) for n in lanes]:
        env = dict(os.environ)
        env.pop("OFX_LIB", None)
        if lib:
            env["OFX_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--blocks", str(a.blocks), "--frame",
               str(a.frame), "--configs"] + [str(c) for c in a.configs]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"photo_bench child ({name}) failed:\n{r.stdout}\n{r.stderr}")
        side = json.loads(r.stdout[r.stdout.index("{"):])
        doc["device"] = side["device"]
        doc[name] = side["kernel"]
    doc["us_over_product"] = {
        name: {f"config{k['config']}_{m}": k[m + "_us"] / kp[m + "_us"] for k, kp in zip(doc[name], doc["product"])
               for m in ("photo_r4", "photo_r8", "photo_r4_shuffled", "photo_r8_shuffled")}
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

assert torch.cuda.is_available(), "photo_bench needs a HIP device (no CPU timing exists)"
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
    scene, seed = S.config_scene(config)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    im0, im1 = S.textured_frame(scene, cam, seed, 0), S.textured_frame(scene, cam, seed, a.frame)
    pts = torch.from_numpy(np.ascontiguousarray(seq.canonical_points, np.float32)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(im0[:3][:, im0[5] > 0].T)).to(dev)
    nodes = torch.from_numpy(seq.nodes).to(dev)
    P, N = pts.shape[0], nodes.shape[0]
    assert col.shape[0] == P
    an, wt, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    valid = v.to(torch.uint8)
    ordered = (pts, col, an, wt, valid)
    packed = pack_transforms(nodes, None, None, dev)
    prep = prepare_depth_device(torch.from_numpy(im1[5]).to(dev), *intr, radius=0, edge_max=0.03, normals=True)
    vmap, nmap = prep["point_image"], prep["normals"]
    cmap = torch.from_numpy(np.ascontiguousarray(im1[:3])).to(dev)
    M = 10000
    f, i = torch.float32, torch.int32
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt, warped = torch.empty((P, 3), device=dev), torch.empty((P, 3), device=dev)
    pixel, cost = torch.empty((P, 2), dtype=i, device=dev), torch.empty(P, dtype=f, device=dev)
    midx = torch.empty(M, dtype=i, device=dev)
    so, to, po = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev), torch.empty((M, 2), device=dev)
    ao, wo = torch.empty((M, 4), dtype=i, device=dev), torch.empty((M, 4), device=dev)
    count = torch.empty(2, dtype=i, device=dev)
    h = _lib.c_void_p()
    call("ofx_assoc_create", P, byref(h))
    camc = _lib.Camera(*intr, W, H)
    aprm = _lib.AssocParams(0.05, 0.5, 0.03, 0, M, 0)
    s = stream_ptr()

    perm = torch.from_numpy(np.random.default_rng(0).permutation(P)).to(dev)
    shuffled = tuple(x[perm].contiguous() for x in (pts, col, an, wt, valid))

    def photo(radius, order=None):
        prm = _lib.PhotoParams(0.05, 0.5, float("inf"), 1.0, radius, M)
        pts, col, an, wt, valid = order or ordered

        def run():
            call("ofx_photo_associate", h, ptr(pts), None, ptr(col), ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N,
                 byref(camc), ptr(vmap), ptr(nmap), ptr(cmap), H, W, byref(prm), ptr(code), ptr(tgt), ptr(warped),
                 ptr(pixel), ptr(cost), ptr(midx), ptr(so), ptr(to), ptr(ao), ptr(wo), ptr(po), ptr(count), s)
        return run

    def assoc():
        call("ofx_associate", h, ptr(pts), None, ptr(an), ptr(wt), ptr(valid), P, ptr(packed), N, byref(camc), ptr(vmap),
             H, W, byref(aprm), ptr(code), ptr(tgt), ptr(warped), ptr(midx), ptr(so), ptr(to), ptr(ao), ptr(wo),
             ptr(count), s)

    sides = {"photo_r4": photo(4), "photo_r8": photo(8), "photo_r4_shuffled": photo(4, shuffled),
             "photo_r8_shuffled": photo(8, shuffled), "associate": assoc}
    for fn in sides.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    us = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, fn in sides.items():
            us[k].append(1e3 * events_ms(fn, per) / per)
    sides["photo_r8"]()
    torch.cuda.synchronize()
    cnt = count.cpu().tolist()
    hist = torch.bincount(code.long(), minlength=8).cpu().tolist()
    _lib.lib.ofx_assoc_destroy(h)
    res = {"config": config, "frame": a.frame, "points": P, "nodes": N, "image": [H, W], "max_matches": M,
           "reps_per_block": per, "blocks": a.blocks}
    for k, v in us.items():
        res[k + "_us_blocks"] = v
        res[k + "_us"] = min(v)
    # taps read per call at radius 8: nine floats per tap inside the image
    res["photo_r8_tap_loads_per_s"] = P * 289 * 9 / (res["photo_r8_us"] * 1e-6)
    res.update(r8_accepted=cnt[0], r8_emitted=cnt[1], r8_code_histogram=hist)
    return res


finish({"tool": "tools/photo_bench.py", "library": os.path.relpath(_lib.LIB_PATH, ROOT),
        "device": torch.cuda.get_device_name(0), "kernel": [kernel_side(c) for c in a.configs]})
