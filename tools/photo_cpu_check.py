"""Measurement (not product, CPU only): the photometric tracking bar of tests/test_gpu_photo.py, run through the numpy
restatement (tests/photo_ref.py, tests/assoc_ref.py) and the oracle's sparse Gauss-Newton (oracle.fusion_oracle.
gn_optimize_sparse) before relying on it on the device — as was done for ofx_associate.

The spin scene at config 1's camera on the Euclidean-graph form of the sequence (the depth-mesh graph needs the device),
8229 canonical points with the textured source frame's colours, frame 0 -> 2 from the identity, 3 ICP iterations, no
motion data, at most `--matches` matches per solve. Prints e_id, e_geo (plane mode, the geometric loop), e_gt (one solve
on 3000 ground-truth matches) and e_photo, the mean 3-D error over the front-facing sphere points, and the bar.

    python tools/photo_cpu_check.py [--matches 3000]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import assoc_ref as ar  # noqa: E402
import photo_ref as pr  # noqa: E402
import prepare_ref as pp  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from occlusionfusion_amd import synthetic as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--matches", type=int, default=3000)
ap.add_argument("--frame", type=int, default=2)
ap.add_argument("--radius", type=int, default=4)
ap.add_argument("--geo-weight", type=float, default=1.0)
a = ap.parse_args()

scene = S.SphereScene(motion="spin", occluder=False)
cam = S.bench_camera(2)
seq = S.SyntheticSequence.build(200, cam=cam, seed=1, scene=scene, graph="euclidean")
intr = (cam.fx, cam.fy, cam.cx, cam.cy)
im0, im1 = S.textured_frame(scene, cam, 1, 0), S.textured_frame(scene, cam, 1, a.frame)
cp = S.backproject(im0[5], cam)
col = im0[:3][:, im0[5] > 0].T
sel = np.sort(np.random.default_rng(5).choice(cp.shape[0], 2 * 4096 + 37, replace=False))
pts, col = cp[sel], np.ascontiguousarray(col[sel])
anc, wts, valid = fo.skin(pts, seq.nodes, seq.node_coverage)
pts, col, anc, wts = pts[valid], col[valid], anc[valid], wts[valid]
N = seq.nodes.shape[0]
vm = fo.backproject_depth(np.ascontiguousarray(im1[5]), *intr)
nm = pp.normal_map(vm, intr, 0.03)
gt = scene.deform_points(pts.astype(np.float64), a.frame)
c = np.array(scene.center)


def facing(p):
    n = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
    return (n * p).sum(1) / np.linalg.norm(p, axis=1) < -0.3


src64 = pts.astype(np.float64)
front = (np.linalg.norm(src64 - c, axis=1) < scene.radius + 0.01) & (src64[:, 2] < scene.plane_z - 0.02) \
    & facing(src64) & facing(gt)


def err(R, T):
    w = fo.ed_warp(pts, anc, wts, np.ones(len(pts), bool), R.astype(np.float32), T.astype(np.float32), seq.nodes)
    return float(np.linalg.norm(w.astype(np.float64) - gt, axis=1)[front].mean())


def solve(src, an, wt, tgt, R, T):
    out = fo.gn_optimize_sparse(seq.nodes, seq.edges, seq.edge_weights, seq.nodes, np.zeros(N), src, an, wt, tgt, intr,
                                prev_rot=R, prev_trans=T)
    assert out["valid_solve"] == 1
    return out["node_rotations"], out["node_translations"]


def track(photo):
    R, T = np.tile(np.eye(3), (N, 1, 1)), np.zeros((N, 3))
    for _ in range(3):
        args = (anc, wts, None, R.astype(np.float32), T.astype(np.float32), seq.nodes, intr, vm)
        if photo:
            m = pr.associate(pts, None, col, *args, nm, im1[:3], radius=a.radius, geo_weight=a.geo_weight,
                             max_matches=a.matches)
        else:
            m = ar.associate(pts, None, *args, mode=ar.PLANE, max_matches=a.matches)
        R, T = solve(m["src"], m["anchors"], m["weights"], m["tgt_out"], R, T)
    return err(R, T), int(m["count"][0])


I, Z = np.tile(np.eye(3), (N, 1, 1)), np.zeros((N, 3))
e_id = err(I, Z)
s, t, _, _ = seq.solver_inputs(a.frame, 3000)
sa, sw, sv = fo.skin(s, seq.nodes, seq.node_coverage)
e_gt = err(*solve(s[sv], sa[sv], sw[sv], t[sv], None, None))
e_geo, n_geo = track(False)
e_photo, n_photo = track(True)
print(f"CPU, spin 0 -> {a.frame}, {N} nodes (Euclidean graph), {len(pts)} points, {int(front.sum())} front-facing, "
      f"<= {a.matches} matches per solve: e_id = {1e3 * e_id:.3f} mm, e_geo = {1e3 * e_geo:.3f} mm ({n_geo} accepted), "
      f"e_gt = {1e3 * e_gt:.3f} mm, e_photo = {1e3 * e_photo:.3f} mm ({n_photo} matched), "
      f"bar = {1e3 * (e_gt + 0.25 * (e_geo - e_gt)):.3f} mm")
