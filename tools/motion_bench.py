"""Measures the motion completion path (motion completion): prints one JSON line and writes it to --out.

* hipEvent time of one MotionCompleter call (pre-processing + 32-launch forward + post-processing) at N = 254 (the demo
  fixture's frame 20) and at config 3's graph (1998 nodes), beside the Gauss-Newton solve of config 1 / config 3
  (10,000 ground-truth matches, default parameters);
* the occluded nodes' position error on config 1's scene with the occluder, frames 1..F tracked from depth alone
  (track_step, canonical model): with no motion term, and with motion_net=.

    python tools/motion_bench.py --out profiles/motion_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from occlusionfusion_amd import synthetic as S  # noqa: E402
from occlusionfusion_amd.motion import MotionCompleter  # noqa: E402
from occlusionfusion_amd.pipeline import FusionPipeline  # noqa: E402
from occlusionfusion_amd.registration import GaussNewtonSolver  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def weights():
    sd = {}
    for n in ("motion_net.npz", "motion_net_l7.npz"):
        with np.load(os.path.join(GOLD, n)) as z:
            sd.update({k: z[k] for k in z.files})
    return sd


def pyramid(nodes, edges):
    pyd, idx = {"nn_index_l0": np.asarray(edges)}, np.arange(len(nodes))
    for l, k in ((1, 6), (2, 4), (3, 3)):
        keep = np.arange(0, len(idx), 4)
        pyd[f"down_sample_idx{l}"] = keep
        pyd[f"up_sample_idx{l}"] = np.minimum(np.arange(len(idx)) // 4, len(keep) - 1)
        idx = idx[keep]
        p = np.asarray(nodes, np.float64)[idx]
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d, np.inf)
        pyd[f"nn_index_l{l}"] = np.argsort(d, axis=1)[:, :min(k, len(idx) - 1)]
    return pyd


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def completer_time(sd, dev, pyd, src, dst, vis, reps):
    mc = MotionCompleter(sd, max_nodes=4096, device=dev)
    mc.set_graph(pyd)
    src, dst, vis = (torch.as_tensor(a, device=dev) for a in (src, dst, vis))
    for _ in range(16):          # fill the history: the steady state has T = 16
        mc(src, dst, vis)
    return timed(lambda: mc(src, dst, vis), reps)


def solve_time(config, dev, reps):
    seq = S.config_sequence(config, device=dev)
    solver = GaussNewtonSolver(len(seq.nodes), 10000)
    src, tgt, tpos, conf = seq.solver_inputs(1, 10000)
    a, w, v = torch.ops.ofx.skin_points(torch.from_numpy(src).to(dev), torch.from_numpy(seq.nodes).to(dev),
                                        float(seq.node_coverage), 4)
    s, t = torch.from_numpy(src).to(dev)[v], torch.from_numpy(tgt).to(dev)[v]
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    tp, cf = torch.from_numpy(tpos).to(dev), torch.from_numpy(conf).to(dev)
    nodes, edges, ew = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (seq.nodes, seq.edges, seq.edge_weights))
    out = timed(lambda: solver.optimize(nodes, edges, ew, tp, cf, s, a[v], w[v], t, intr), reps)
    out["nodes"] = len(seq.nodes)
    return out, seq


def occluded_error(sd, dev, frames):
    c = S.BASELINE_CONFIGS[1]
    seq = S.SyntheticSequence.build(c["nodes"], cam=S.bench_camera(c["cam_scale"]), seed=c["seed"],
                                    scene=S.SphereScene(motion="nonrigid", occluder=True),
                                    coverage=S.config_coverage(1), graph="geodesic", device=dev)
    res = {}
    for name in ("no_motion_term", "motion_net"):
        pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=dev,
                              gn_params=dict(precond="direct"))
        pipe.integrate_source(pipe.prepare(0))
        mc = None
        if name == "motion_net":
            mc = MotionCompleter(sd, max_nodes=512, device=dev)
            mc.set_graph(pyramid(seq.nodes, seq.edges))
        occ, vis, n_occ = [], [], []
        for t in range(1, frames + 1):
            out = pipe.track_step(pipe.prepare(t), t, motion=False, motion_net=mc)
            got = seq.nodes + out["node_translations"].cpu().numpy()
            want = seq.scene.deform_points(seq.nodes, t)
            err = np.linalg.norm(got - want, axis=1)
            hidden = ~seq.visible(want, t, tol=0.02)
            occ.append(float(err[hidden].mean()) if hidden.any() else 0.0)
            vis.append(float(err[~hidden].mean()))
            n_occ.append(int(hidden.sum()))
        res[name] = dict(occluded_mean_err_mm=[round(1e3 * x, 3) for x in occ],
                         visible_mean_err_mm=[round(1e3 * x, 3) for x in vis], occluded_nodes=n_occ,
                         occluded_mean_over_frames_mm=round(1e3 * float(np.mean(occ)), 3),
                         visible_mean_over_frames_mm=round(1e3 * float(np.mean(vis)), 3))
    res["nodes"], res["frames"] = len(seq.nodes), frames
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = weights()
    with np.load(os.path.join(GOLD, "motion_demo.npz")) as z:
        node = z["node_20"]
        keys = [f"nn_index_l{l}" for l in range(4)] + [f"{d}_sample_idx{l}" for d in ("down", "up") for l in (1, 2, 3)]
        pyd = {k: z[f"{k}_20"] for k in keys}
    pos, mo = node[:, :3].astype(np.float64), node[:, 3:6].astype(np.float64)
    out = {"completer_n254": completer_time(sd, dev, pyd, pos, pos + mo, node[:, 6] > 0.5, a.reps)}
    out["solve_config1"], _ = solve_time(1, dev, a.reps)
    out["solve_config3"], seq3 = solve_time(3, dev, a.reps)
    n3 = seq3.nodes.astype(np.float64)
    tp3 = seq3.scene.deform_points(seq3.nodes, 1).astype(np.float64)
    out[f"completer_n{len(n3)}"] = completer_time(sd, dev, pyramid(seq3.nodes, seq3.edges), n3, tp3,
                                                  seq3.visible(tp3, 1, tol=0.02), a.reps)
    out["occluder_sequence"] = occluded_error(sd, dev, a.frames)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
