"""Measurement (not product): what the weighted integrate costs on the bench scene.

Config 3's volume, graph and frames (512^3 at 4 mm, 640x448): the source frame integrated, frame 1 solved once (step()), then
frame 1's warped integrate launched again and again on that state — with the frame's observation-weight image
(TSDFVolume.integrate_device(weight_image=)) and without it, alternating blocks in one process, the best block kept. Two
clocks: the library's own events around the integrate launches (TSDFVolume.integrate_timing: tile maxima, brick cull and
integrate kernel) and device events around the whole calls. ofx_observation_weights is timed on the same frame's vertex
and normal maps, beside the ofx_prepare_depth call that makes them.

    python tools/weighted_integrate_bench.py [--reps 60] [--config 3] [--out profiles/weighted_integrate.json]

The library under test is the one OFX_LIB names (default: the product), e.g. a tuning build with -DOFX_INT_WPE_W=n
(occlusionfusion_amd.build.build(out=..., defines=("OFX_INT_WPE_W=6",))).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

import torch  # noqa: E402
from occlusionfusion_amd import _lib  # noqa: E402
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd.image_proc import prepare_depth_device  # noqa: E402
from occlusionfusion_amd.pipeline import FusionPipeline  # noqa: E402
from occlusionfusion_amd.tsdf import FUSION_EDGE_MAX, TSDFVolume, fusion_weight_params  # noqa: E402

assert torch.cuda.is_available(), "weighted_integrate_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


c = S.BASELINE_CONFIGS[a.config]
seq = S.config_sequence(a.config, device=dev)
D = c["dims"]
pipe = FusionPipeline(seq, c["origin"], c["voxel"], (D, D, D), n_matches=10000, device=dev)
pipe.integrate_source(pipe.prepare(0))
fi = pipe.prepare(1)
pipe.step(fi, 1)
vol = pipe.vol
torch.cuda.synchronize()

fw = fusion_weight_params(True)
intr = pipe.intr
depth = fi.im[-1].contiguous()


def prepare():
    return prepare_depth_device(depth, *intr, edge_max=FUSION_EDGE_MAX, **fw["filter"])


prep = prepare()


def weights():
    return vol.observation_weights(prep["point_image"], prep["normals"], fw["cos_power"], fw["z_ref"], fw["w_floor"],
                                   fw["edge_weight"])


wim = weights()
sides = {"unweighted": lambda: vol.integrate_device(),
         "weighted": lambda: vol.integrate_device(weight_image=wim),
         "weighted_capped": lambda: vol.integrate_device(weight_image=wim, max_weight=64.0)}
for fn in list(sides.values()) + [prepare, weights]:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
per = max(1, a.reps // a.blocks)
call_us = {k: [] for k in sides}
kern_us = {k: [] for k in sides}
for _ in range(a.blocks):
    for k, fn in sides.items():
        TSDFVolume.integrate_timing(True)
        call_us[k].append(1e3 * events_ms(fn, per) / per)
        ms, n = TSDFVolume.integrate_timing(False)
        assert n == per, (k, n, per)
        kern_us[k].append(1e3 * ms / per)
aux = {"prepare_depth": [], "observation_weights": []}
for _ in range(a.blocks):
    aux["prepare_depth"].append(1e3 * events_ms(prepare, per) / per)
    aux["observation_weights"].append(1e3 * events_ms(weights, per) / per)

wn = wim.cpu().numpy()
cache = vol.warpfield.skin_tsdf_cache()
res = {"tool": "tools/weighted_integrate_bench.py", "library": os.path.relpath(_lib.LIB_PATH, ROOT),
       "device": torch.cuda.get_device_name(0), "config": a.config, "dims": D, "image": list(wn.shape),
       "listed_bricks": int(cache.n_list), "reps_per_block": per, "blocks": a.blocks,
       "weight_image": {"zero_share": float((wn == 0).mean()), "mean_of_positive": float(wn[wn > 0].mean())}}
for k in sides:
    res[k + "_kernel_us_blocks"] = kern_us[k]
    res[k + "_kernel_us"] = min(kern_us[k])
    res[k + "_call_us"] = min(call_us[k])
for k, v in aux.items():
    res[k + "_us_blocks"] = v
    res[k + "_us"] = min(v)
res["weighted_over_unweighted_kernel"] = res["weighted_kernel_us"] / res["unweighted_kernel_us"]
res["weighted_capped_over_unweighted_kernel"] = res["weighted_capped_kernel_us"] / res["unweighted_kernel_us"]
txt = json.dumps(res, indent=1)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")
