"""Measurement (not product): the surface-point sampler against the mesh-plus-skin pair it replaces.

Configs 1 and 3, the volume after the source frame and one warped frame (frame 1, the nodes at their ground-truth
motion). In one process, on the same volume, device events around `--reps` calls after a warm-up, the two sides
alternated in blocks:

  sampler   WarpField.surface_points(sync=False): ofx_surface_points, four launches, no host read
  pair      TSDFVolume.extract_mesh_device(with_normals=True) followed by WarpField.skin_device of its vertices (in world
            coordinates): marching cubes with its count read-back, then the brute-force k-NN skin

with both point counts, and at config 1 the per-frame wall time of FusionPipeline.track_step(model="volume") next to
track_step() over a few frames. `--trace DIR` also runs a short copy of itself under `rocprofv3 --kernel-trace --stats`
(a fresh child process) and copies the per-kernel stats csv next to the JSON.

    python tools/surface_bench.py [--reps 100] [--out profiles/surface_bench.json] [--trace out/surface_prof]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd.pipeline import FusionPipeline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--blocks", type=int, default=4, help="the reps of each side are split into this many alternating blocks")
ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
ap.add_argument("--max-points", type=int, default=65536)
ap.add_argument("--frames", type=int, default=6, help="frames of the track_step comparison (config 1)")
ap.add_argument("--no-track", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--trace", default=None, help="folder for a rocprofv3 --kernel-trace --stats run of a short copy")
a = ap.parse_args()


def trace(folder):
    """A short copy under rocprofv3 --kernel-trace --stats, in a fresh child process; -> the kernel stats csv's path."""
    os.makedirs(folder, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", folder, "-o", "surface", "--",
           sys.executable, os.path.abspath(__file__), "--reps", "20", "--no-track", "--configs"] + \
          [str(c) for c in a.configs] + ["--max-points", str(a.max_points)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({r.returncode}):\n{r.stderr[-2000:]}")
    found = sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise RuntimeError(f"no kernel stats csv under {folder}")
    return found[-1]


traced = trace(a.trace) if a.trace else None   # first: the child runs before this process opens the device
assert torch.cuda.is_available(), "surface_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def pipeline(config, seq, **kw):
    c = S.BASELINE_CONFIGS[config]
    return FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=dev, **kw)


def kernel_side(config):
    seq = S.config_sequence(config, device=dev)
    pipe = pipeline(config, seq)
    pipe.integrate_source(pipe.prepare(0))
    fi = pipe.prepare(1)
    T = torch.from_numpy((seq.scene.deform_points(seq.nodes, 1) - seq.nodes).astype(np.float32)).to(dev)
    pipe.prev_rot = torch.eye(3, device=dev).repeat(seq.nodes.shape[0], 1, 1).contiguous()
    pipe.prev_trans = T
    pipe.integrate(fi, 1)
    vol, wf = pipe.vol, pipe.wf
    cache = wf.skin_tsdf_cache()
    origin = torch.from_numpy(np.asarray(vol._vol_origin, np.float32)).to(dev)
    vs = float(np.float32(vol._voxel_size))
    sizes = {}

    def sampler():
        wf.surface_points(a.max_points, sync=False)

    def pair():
        m = vol.extract_mesh_device(with_normals=True)
        world = m["verts"] * vs + origin
        an, wt, v = wf.skin_device(world)
        sizes["verts"], sizes["faces"] = int(world.shape[0]), int(m["faces"].shape[0])
        sizes["skinned"] = v

    for _ in range(5):
        sampler()
        pair()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    ms = {"sampler": [], "pair": []}
    for _ in range(a.blocks):
        ms["sampler"].append(events_ms(sampler, per))
        ms["pair"].append(events_ms(pair, per))
    m = wf.surface_points(a.max_points, with_codes=True)
    us = {k: [1e3 * x / per for x in v] for k, v in ms.items()}
    best = {k: min(v) for k, v in us.items()}
    hist = m["histogram"]
    # algorithmic bytes: the listed bricks' tsdf and weight (8 B a voxel); the six face layers, tsdf and weight, of the
    # bricks that pass codes 1-3 somewhere (not counted apart here: at most 6*64*8 B a listed brick); 8 B of anchors per
    # geometric survivor (codes 0 and 7) and 24 B of skin, 28 B of tsdf gathers and 57 B of row per emitted point; 1 B
    # of code per listed voxel when asked for; 72 B of scratch per listed brick (count, offset, 8 bit words)
    n_list = cache.n_list
    b_bricks = n_list * 512 * 8
    b_face_max = n_list * 6 * 64 * 8
    b_surv = (hist[0] + hist[7]) * 8
    b_rows = m["emitted"] * (24 + 28 + 57) + (a.max_points - m["emitted"]) * 57
    return {"config": config, "dims": S.BASELINE_CONFIGS[config]["dims"], "nodes": int(seq.nodes.shape[0]),
            "listed_bricks": n_list, "max_points": a.max_points, "reps_per_block": per, "blocks": a.blocks,
            "sampler_us_per_call_blocks": us["sampler"], "sampler_us_per_call": best["sampler"],
            "pair_us_per_call_blocks": us["pair"], "pair_us_per_call": best["pair"],
            "pair_over_sampler": best["pair"] / best["sampler"],
            "sampler_points": {"accepted": m["accepted"], "emitted": m["emitted"], "code_histogram": hist},
            "pair_points": {"vertices": sizes["verts"], "faces": sizes["faces"],
                            "skin_valid_vertices": int(sizes["skinned"].sum().item())},
            "algorithmic_bytes": {"bricks_tsdf_weight": b_bricks, "face_layers_upper_bound": b_face_max,
                                  "survivor_anchors": b_surv, "rows_and_gathers": b_rows,
                                  "scratch": n_list * 72},
            "bricks_gb_per_s": b_bricks / (best["sampler"] * 1e-6) / 1e9}


def track_side(config=1):
    seq = S.config_sequence(config, device=dev)
    res = {"config": config, "frames": a.frames}
    for model in ("canonical", "volume"):
        pipe = pipeline(config, seq, gn_params=dict(precond="direct") if seq.nodes.shape[0] <= 512 else None)
        pipe.integrate_source(pipe.prepare(0))
        fis = [pipe.prepare(t) for t in range(1, a.frames + 1)]
        t_ms, acc = [], []
        for t, fi in enumerate(fis, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.track_step(fi, t, model=model, max_model_points=a.max_points)
            torch.cuda.synchronize()
            t_ms.append(1e3 * (time.perf_counter() - t0))
            acc.append([x["accepted"] for x in out["assoc"]])
        res[model] = {"ms_per_frame": t_ms, "ms_per_frame_after_first": float(np.mean(t_ms[1:])), "accepted": acc}
        if model == "volume":
            res[model]["model_counts"] = torch.stack(pipe.model_counts).cpu().tolist()
        else:
            res[model]["model_points"] = int(pipe._track[0].shape[0])
    return res


doc = {"tool": "tools/surface_bench.py", "device": torch.cuda.get_device_name(0),
       "kernel": [kernel_side(c) for c in a.configs]}
if not a.no_track:
    doc["track_step"] = track_side(1)
if traced:
    csv = traced
    if a.out:
        dst = os.path.splitext(os.path.abspath(a.out))[0] + "_kernel_stats.csv"
        shutil.copyfile(csv, dst)
        doc["kernel_stats_csv"] = os.path.relpath(dst, ROOT)
txt = json.dumps(doc, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
