"""The Gauss-Newton parameter problem of test_gn_params_ref.py / test_gpu_gn_params.py: gn_small.npz (257 nodes, 600
matches, 8 neighbours) with everything the golden file cannot exercise derived from it under fixed seeds:

* target_px / target_py: the projection of tgt through the intrinsics plus N(0, 0.3 px), stored as f32;
* two non-uniform edge-weight arrays (the golden weights are 1/8, so NB·w = 1 and use_edge_weighting is a no-op on them):
  "a" uniform(0.5, 2)/8 per entry, "b" the graph builder's exp(-d²/(2·0.05²)) normalised per row (NB·w over five decades);
* an edge table with -1 padding: every third node loses its last two neighbours, node PAD_BARE loses all of them;
* a non-identity start pose: R = exp(N(0, 0.2 rad)), t = N(0, 0.01), rounded to f32 (both sides take the f32 values).

SETS names the parameter sets and the level each is held to ("all": assembly, exact solve, cluster PCG, forced Schwarz;
"direct": assembly and exact solve; "direct1": assembly and a one-step exact solve). oracle() caches the f64 reference
solve per (set, padded) so the GPU tests share it.
"""
import functools
import os

import numpy as np

from oracle import fusion_oracle as fo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD_BARE = 100          # the node without any neighbour in the padded table
# Every golden fixture has fx = fy, so nothing tells fx/z from fy/z (or mfx from mfy where they meet equal x and y
# factors). ANISO is gn_small's camera with fy = 1.25 fx and a shifted cy, for the checks that must tell them apart; the
# parameter sets' own solves and condition numbers stay on the golden camera.
ANISO = (131.25, 164.0625, 79.875, 48.875)
MIXED = dict(lambda_flow=1e-3, use_edge_weighting=True, lambda_depth=0.5, lambda_arap=2.0, lambda_motion=0.25,
             lm_factor=1e-5)
# tag -> (solver parameters, edge-weight kind or None, level)
SETS = {
    "default": ({}, None, "all"),
    "ew_mild": (dict(use_edge_weighting=True), "a", "all"),
    "ew_builder": (dict(use_edge_weighting=True), "b", "all"),
    "flow_1e-4": (dict(lambda_flow=1e-4), None, "all"),
    "flow_1e-3": (dict(lambda_flow=1e-3), None, "all"),
    "mixed": (MIXED, "a", "all"),
    "no_motion": (dict(lambda_motion=0.0), None, "all"),
    "depth4": (dict(lambda_depth=4.0, lambda_arap=0.1), None, "all"),
    "flow_1e-2": (dict(lambda_flow=1e-2, stop_loss_diff=1e9), None, "direct"),
    "flow_1": (dict(lambda_flow=1.0), None, "direct"),
    "flow_ref": (dict(lambda_flow=5.0, num_iter=1), None, "direct1"),
}
ALL_SETS = [k for k, v in SETS.items() if v[2] == "all"]
DIRECT_SETS = ALL_SETS + ["flow_1e-2", "flow_1", "flow_ref"]


@functools.lru_cache(maxsize=None)
def base():
    """The derived arrays (read-only): the golden problem plus tpx, tpy, ew_a, ew_b, edges_pad, R0, t0."""
    g = np.load(os.path.join(GOLDEN, "gn_small.npz"), allow_pickle=False)
    d = {k: g[k] for k in ("nodes", "edges", "edge_weights", "tpos", "conf", "src", "anchors", "weights", "tgt")}
    d["intr"] = tuple(float(v) for v in g["intr"])
    fx, fy, cx, cy = d["intr"]
    N, NB = d["edges"].shape
    M = d["src"].shape[0]
    rng = np.random.default_rng(20240611)
    tgt = d["tgt"].astype(np.float64)
    d["tpx"] = (fx * tgt[:, 0] / tgt[:, 2] + cx + rng.normal(0.0, 0.3, M)).astype(np.float32)
    d["tpy"] = (fy * tgt[:, 1] / tgt[:, 2] + cy + rng.normal(0.0, 0.3, M)).astype(np.float32)
    d["ew_a"] = (rng.uniform(0.5, 2.0, (N, NB)) / NB).astype(np.float32)
    nodes = d["nodes"].astype(np.float64)
    dist2 = ((nodes[:, None, :] - nodes[np.maximum(d["edges"], 0)]) ** 2).sum(2)
    wb = np.where(d["edges"] >= 0, np.exp(-dist2 / (2 * 0.05 ** 2)), 0.0)
    d["ew_b"] = (wb / wb.sum(1, keepdims=True)).astype(np.float32)
    ep = d["edges"].copy()
    ep[::3, -2:] = -1
    ep[PAD_BARE, :] = -1
    d["edges_pad"] = ep
    d["R0"] = fo.angle_axis_to_rotation_matrix(rng.normal(0.0, 0.2, (N, 3))).astype(np.float32)
    d["t0"] = rng.normal(0.0, 0.01, (N, 3)).astype(np.float32)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def params(tag):
    return dict(SETS[tag][0])


def edge_weights(tag):
    kind = SETS[tag][1]
    return base()["edge_weights" if kind is None else "ew_" + kind]


def inputs(tag, pad=False, intr=None):
    """The ten positional arguments of GaussNewtonSolver.optimize / fo.gn_optimize for the set (intr: other intrinsics
    than the golden file's, ANISO)."""
    d = base()
    return (d["nodes"], d["edges_pad" if pad else "edges"], edge_weights(tag), d["tpos"], d["conf"], d["src"],
            d["anchors"], d["weights"], d["tgt"], d["intr"] if intr is None else intr)


def flow_targets(tag):
    """target_px / target_py keywords: given whenever the set has flow rows."""
    d = base()
    return dict(target_px=d["tpx"], target_py=d["tpy"]) if SETS[tag][0].get("lambda_flow", 0.0) > 0 else {}


def pose(identity=False):
    """(R, t) as f64 copies of the f32 start pose (or the identity pose)."""
    d = base()
    N = d["nodes"].shape[0]
    if identity:
        return np.tile(np.eye(3), (N, 1, 1)), np.zeros((N, 3))
    return d["R0"].astype(np.float64), d["t0"].astype(np.float64)


def system(tag, pad=False, identity=False, gn_iter=0, intr=None, **kw):
    """fo.gn_system of the set at the start pose, with the LM factor of GN step gn_iter (model.py:418-419)."""
    i = inputs(tag, pad, intr)
    p = params(tag)
    lm = p.pop("lm_factor", fo.GN_DEFAULTS["lm_factor"])
    for k in range(gn_iter + 1):
        if k % 3 == 2:
            lm /= 2
    p.pop("num_iter", None)
    R, t = pose(identity)
    return fo.gn_system(i[0], i[1], *i[3:], R, t, lm_factor=lm, graph_edges_weights=i[2], **flow_targets(tag), **p,
                        **kw)


@functools.lru_cache(maxsize=None)
def oracle(tag, pad=False, sparse=True, intr=None):
    """The f64 reference solve of the set from the non-identity pose (gn_optimize_sparse: the dense one's entries in
    another summation order, test_gn_params_ref.py holds the two to 1e-9 of each other)."""
    R, t = pose()
    f = fo.gn_optimize_sparse if sparse else fo.gn_optimize
    return f(*inputs(tag, pad, intr), prev_rot=R, prev_trans=t, **flow_targets(tag), **params(tag))
