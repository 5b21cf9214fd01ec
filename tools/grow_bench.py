"""Measurement (not product): graph growth at config 3's sizes (512^3, 1998 nodes, 65 536 model rows).

The volume after the source frame and one warped frame (frame 1, the nodes at their ground-truth motion). In one
process, device events around `--reps` calls after a warm-up, the sides alternated in blocks, the median of the blocks'
per-call times:

  grow          one ofx_grow_nodes call (NodeGrower.grow) on the sampled model with the defaults (min_dist 2·coverage,
                spacing = coverage, max_new 256), and its counts
  incremental   for 8, 32 and 128 added nodes: ofx_skin_grow_plan + the enlarged cache tensors + ofx_skin_grow_apply
                (WarpField._skin_plan / _skin_apply: the in-place update of grow_from_volume, without its host read)
  full          for the same graphs: WarpField.skin_tsdf_cache() from nothing, as a growth did it before the in-place
                update existed (brick cull with its count read-back, skin of every listed brick, palette)

The graphs with exactly 8 / 32 / 128 new nodes come from ofx_grow_nodes with max_new = that number; where the defaults
select fewer, min_dist is lowered step by step (the factor used is recorded).

    python tools/grow_bench.py [--reps 20] [--out profiles/grow_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd.grow import NodeGrower  # noqa: E402
from occlusionfusion_amd.pipeline import FusionPipeline  # noqa: E402
from occlusionfusion_amd.warpfield import SkinCache  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--max-points", type=int, default=65536)
ap.add_argument("--added", type=int, nargs="+", default=[8, 32, 128])
ap.add_argument("--out", default=None)
a = ap.parse_args()

assert torch.cuda.is_available(), "grow_bench needs a HIP device (no CPU timing exists)"
dev = torch.device("cuda", 0)


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def timed(sides):
    """sides: name -> fn; alternating blocks after a warm-up -> name -> median per-call ms."""
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    per = max(1, a.reps // a.blocks)
    ms = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, fn in sides.items():
            ms[k].append(events_ms(fn, per))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


c = S.BASELINE_CONFIGS[a.config]
seq = S.config_sequence(a.config, device=dev)
pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=dev)
pipe.integrate_source(pipe.prepare(0))
fi = pipe.prepare(1)
N0 = seq.nodes.shape[0]
pipe.prev_rot = torch.eye(3, device=dev).repeat(N0, 1, 1).contiguous()
pipe.prev_trans = torch.from_numpy((seq.scene.deform_points(seq.nodes, 1) - seq.nodes).astype(np.float32)).to(dev)
pipe.integrate(fi, 1)
pipe.flush()
torch.cuda.synchronize()
vol, wf = pipe.vol, pipe.wf
cache0 = wf.skin_tsdf_cache()
cov = wf.node_coverage
K_e = wf.graph.edges.shape[1]
m = wf.surface_points(a.max_points, sync=False)
model_counts = m["count"].cpu().tolist()
grower = NodeGrower(a.max_points, 256, dev)
nodes0, R0, T0 = wf.nodes_t.clone(), wf.R_t.clone(), wf.T_t.clone()
E0 = torch.from_numpy(wf.graph.edges).to(dev)
W0 = torch.from_numpy(wf.graph.edges_weights).to(dev)


def buffers(max_new):
    rows = N0 + max_new
    out = [torch.zeros((rows, 3), device=dev), torch.zeros((rows, 3, 3), device=dev), torch.zeros((rows, 3), device=dev),
           torch.full((rows, K_e), -1, dtype=torch.int32, device=dev), torch.zeros((rows, K_e), device=dev)]
    for t, src in zip(out, (nodes0, R0, T0, E0, W0)):
        t[:N0] = src
    return out


def grow(buf, max_new, factor=2.0):
    return grower.grow(m["points"], m["anchors"], m["weights"], m["valid"], buf[0], N0, buf[1], buf[2], buf[3], buf[4], cov,
                       factor * cov, cov, max_new)


res = {"config": a.config, "dims": c["dims"], "nodes": N0, "model_rows": a.max_points,
       "model_counts_accepted_emitted": model_counts, "listed_bricks": cache0.n_list, "coverage": cov, "reps": a.reps,
       "blocks": a.blocks, "device": torch.cuda.get_device_name(0)}
buf = buffers(256)
med, blocks = timed({"grow": lambda: grow(buf, 256)})
res["grow_nodes"] = {"ms": med["grow"], "blocks_ms": blocks["grow"], "count_candidates_selected_capped": grow(buf, 256).cpu().tolist()}
print("ofx_grow_nodes:", res["grow_nodes"])

res["skin_update"] = []
for k in a.added:
    for factor in (2.0, 1.5, 1.0, 0.75, 0.5, 0.25):
        buf = buffers(k)
        cnt = grow(buf, k, factor)
        if int(cnt[1].item()) == k:
            break
    n_sel = int(cnt[1].item())
    n_added = cnt[1:2].clone()
    wf.nodes_t, wf.num_nodes, wf._packed = buf[0][:N0 + n_sel].contiguous(), N0 + n_sel, None
    wf._cache = cache0
    wb, ws, pc = wf._skin_plan(buf[0], N0, n_added)
    n_re, n_app = (int(v) for v in pc.cpu().tolist())
    keep = SkinCache(cache0.brick_list, cache0.n_list, cache0.anchors.clone(), cache0.weights.clone(), cache0.k,
                     cache0.pal_ids.clone(), cache0.pal_n.clone(), cache0.local.clone())
    state = {}

    def incremental():
        wf._cache = keep
        w1, w2, _ = wf._skin_plan(buf[0], N0, n_added)
        state["inc"] = wf._skin_apply(keep, w1, w2, n_re, n_app)

    def full():
        wf._cache = None
        state["full"] = wf.skin_tsdf_cache()

    med, blocks = timed({"incremental": incremental, "full": full})
    assert state["inc"].n_list == state["full"].n_list, (state["inc"].n_list, state["full"].n_list)
    row = {"added": n_sel, "min_dist_factor": factor, "reskinned": n_re, "appended": n_app, "n_list": state["full"].n_list,
           "incremental_ms": med["incremental"], "full_ms": med["full"], "full_over_incremental": med["full"] / med["incremental"],
           "blocks_ms": blocks}
    print(row)
    res["skin_update"].append(row)
    state.clear()

line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
print(line)
