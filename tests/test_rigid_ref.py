"""CPU: the numpy restatement of the rigid point-to-plane ICP (tests/rigid_ref.py) does what the stage is for, so that the
GPU tests can pin the kernel to it.

* a room corner (three non-parallel planes, all six unknowns observable): model points moved by 3° and 2 cm are brought
  back; the final pose error is printed — the GPU test compares against that figure, computed live;
* one plane facing the camera (rank 3): the damped step is finite and has nothing in the three unobservable directions;
* fewer accepted points than min_matches: status 1 with the pose kept, then status 3;
* fold_rigid followed by the oracle's ED warp is R·warp + S·t.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as rr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

GATES = dict(dist_max=0.1, cos_min=0.5, edge_max=0.03)


def test_corner_scene_brings_displaced_points_back():
    """The start is 3° (0.0524 rad) and 2 cm off. Point-to-plane ICP on exact planes converges quadratically once the
    matches settle; what remains comes from the creases, where central differences blend two planes' normals. Asked:
    both errors under a hundredth of the start's. Measured: 8.5e-5 rad and 9.5e-5 m after 8 iterations (with and
    without the normal gate), steps below 1e-7 from iteration 4 on."""
    s = rr.corner_problem()
    ang0, d0 = rr.pose_error(rr.IDENTITY, s["truth"], s["apex"])
    assert abs(ang0 - np.radians(3.0)) < 1e-9 and abs(d0 - 0.02) < 1e-4
    for nrm in (s["nrm"], None):
        out = rr.icp(s["pts"], nrm, s["anchors"], s["weights"], None, s["R"], s["T"], s["nodes"], rr.INTR_C, s["vmap"],
                     iters=8, **GATES)
        sysm = out["systems"]
        ang, d = rr.pose_error(out["pose"], s["truth"], s["apex"])
        print(f"corner scene, normals {nrm is not None}: accepted {sysm[:, rr.COUNT].astype(int).tolist()}, "
              f"rms {np.sqrt(sysm[:, rr.RR] / sysm[:, rr.COUNT]).tolist()}, final pose error {ang:.3e} rad {d:.3e} m")
        assert (sysm[:, rr.STATUS] == 0).all() and (sysm[:, rr.COUNT] > 0.9 * s["pts"].shape[0]).all()
        assert ang < 0.01 * ang0 and d < 0.01 * d0
        assert sysm[-1, rr.RR] < 0.01 * sysm[0, rr.RR]
        assert len(out["poses"]) == 8 and np.array_equal(out["poses"][0], rr.IDENTITY)


def _plane_problem():
    """A plane z = 1.2 facing the camera and 800 points 1 cm behind it. Its vertex map gives n_q = (0, 0, -1) exactly
    (the neighbour differences are (a, 0, 0) and (0, b, 0)), so rows are [(-y_y, y_x, 0), (0, 0, -1)]: rotation about z and
    translation along x and y are exactly unobservable. (A tilted plane is rank 3 only in exact arithmetic: the f32
    rounding of its vertex map turns the normals by ~1e-6, which gives the null directions eigenvalues far below the
    damping and components that the damping, not the data, decides.)"""
    H, W = rr.H_C, rr.W_C
    fx, fy, cx, cy = rr.INTR_C
    vmap = fo.backproject_depth(np.full((H, W), 1.2, np.float32), *rr.INTR_C)
    rng = np.random.default_rng(3)
    pu, pv = rng.uniform(6, W - 7, 800), rng.uniform(6, H - 7, 800)
    pts = np.stack([(pu - cx) / fx * 1.21, (pv - cy) / fy * 1.21, np.full(800, 1.21)], 1).astype(np.float32)
    nodes = pts[:8].copy()
    a, w = rr.knn_skin(pts, nodes)
    R = np.broadcast_to(np.eye(3, dtype=np.float32), (8, 3, 3)).copy()
    return pts, a, w, R, np.zeros((8, 3), np.float32), nodes, vmap


def test_single_plane_is_rank_three_and_the_damped_step_stays_observable():
    pts, a, w, R, T, nodes, vmap = _plane_problem()
    code, J, r = rr.rows(pts, None, a, w, None, R, T, nodes, rr.INTR_C, vmap, rr.IDENTITY, 0.05, 0.5, 0.03)
    assert (code == 0).all()
    row, _ = rr.system(code, J, r)
    A, b = rr.unpack(row)
    ev, U = np.linalg.eigh(A)
    assert np.linalg.matrix_rank(A) == 3 and np.all(np.abs(ev[:3]) <= 1e-12 * ev[-1])
    assert np.isinf(np.linalg.cond(A)) or np.linalg.cond(A) > 1e15       # undamped: no Cholesky
    solved, pose, xi = rr.solve(row, rr.IDENTITY, damping=1e-6)
    assert solved[rr.STATUS] == 0 and np.isfinite(xi).all() and np.isfinite(pose).all()
    unobs, obs = np.abs(U[:, :3].T @ xi).max(), np.linalg.norm(U[:, 3:].T @ xi)
    print(f"plane: eigenvalues / largest {(ev / ev[-1]).tolist()}, step {xi.tolist()}, unobservable {unobs:.3e}, "
          f"observable {obs:.3e}")
    assert obs > 0 and unobs <= 1e-6 * obs
    assert abs(xi[5] + 0.01) < 1e-4                                       # the 1 cm along the normal is what it finds


def test_too_few_matches_keeps_the_pose_then_drains():
    pts, a, w, R, T, nodes, vmap = _plane_problem()
    start = rr.rigid_about((0, 1, 0), 0.5, (0, 0, 1.2), (0.001, 0, 0))
    out = rr.icp(pts[:5], None, a[:5], w[:5], None, R, T, nodes, rr.INTR_C, vmap, pose=start, iters=3, min_matches=6)
    assert out["systems"][:, rr.STATUS].tolist() == [1, 3, 3] and out["systems"][0, rr.COUNT] == 5
    assert np.array_equal(out["pose"], start) and not out["systems"][1:, :29].any()
    out = rr.icp(pts[:5], None, a[:5], w[:5], None, R, T, nodes, rr.INTR_C, vmap, pose=start, iters=2, min_matches=5)
    assert out["systems"][0, rr.STATUS] == 0 and not np.array_equal(out["pose"], start)
    empty = rr.icp(pts[:0], None, a[:0], w[:0], None, R, T, nodes, rr.INTR_C, vmap, pose=start, iters=2)
    assert empty["systems"][:, rr.STATUS].tolist() == [1, 1] and np.array_equal(empty["pose"], start)


def test_stop_twist_drains_after_the_converged_iteration():
    s = rr.corner_problem(count=400)
    out = rr.icp(s["pts"], None, s["anchors"], s["weights"], None, s["R"], s["T"], s["nodes"], rr.INTR_C, s["vmap"],
                 iters=8, stop_twist=1e-4, **GATES)
    st = out["systems"][:, rr.STATUS].tolist()
    k = st.index(3)
    assert 2 <= k < 8 and st == [0] * k + [3] * (8 - k)
    assert max(out["systems"][k - 1, rr.WNORM], out["systems"][k - 1, rr.VNORM]) < 1e-4
    assert len(out["poses"]) == k


def test_fold_rigid_then_warp_is_the_posed_warp():
    """The folded transforms go through the oracle's f32 ED warp; the other side is R·warp(x) + S·t in f64 from the
    oracle's f32 warp under the unfolded transforms. Both sides carry the f32 warp's own rounding, a few ulp of the
    largest coordinate: 4 ulp are asked."""
    rng = np.random.default_rng(5)
    N, P = 24, 3000
    nodes = (rng.uniform(-0.4, 0.4, (N, 3)) + [0, 0, 1.3]).astype(np.float32)
    Rk = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.05, (N, 3))).astype(np.float32)
    Tk = rng.normal(0, 0.01, (N, 3)).astype(np.float32)
    pts = (rng.uniform(-0.4, 0.4, (P, 3)) + [0, 0, 1.3]).astype(np.float32)
    a, w = rr.knn_skin(pts, nodes)
    w[: P // 2] *= np.float32(0.8)                                   # weights that do not sum to one: S != 1
    ok = np.ones(P, bool)
    pose = rr.rigid_about((0.3, 1.0, 0.2), 3.0, (0, 0, 1.3), (0.012, -0.008, 0.0139))
    base = fo.ed_warp(pts, a, w, ok, Rk, Tk, nodes).astype(np.float64)
    want = base @ pose[:, :3].T + w.astype(np.float64).sum(1, keepdims=True) * pose[:, 3]
    for rot, trans, ref in ((Rk, Tk, want), (None, None, None)):
        R2, T2 = rr.fold_rigid(nodes, rot, trans, pose)
        assert R2.dtype == np.float32 and T2.dtype == np.float32 and R2.shape == (N, 3, 3) and T2.shape == (N, 3)
        got = fo.ed_warp(pts, a, w, ok, R2, T2, nodes).astype(np.float64)
        if ref is None:
            eye = np.broadcast_to(np.eye(3, dtype=np.float32), (N, 3, 3))
            b0 = fo.ed_warp(pts, a, w, ok, eye, np.zeros((N, 3), np.float32), nodes).astype(np.float64)
            ref = b0 @ pose[:, :3].T + w.astype(np.float64).sum(1, keepdims=True) * pose[:, 3]
        ulp = np.spacing(np.float32(np.abs(ref).max()))
        err = np.abs(got - ref).max()
        print(f"fold_rigid: max |folded warp - posed warp| = {err:.3e} = {err / ulp:.2f} ulp of {np.abs(ref).max():.3f}")
        assert err <= 4 * ulp
    assert np.array_equal(rr.fold_rigid(nodes, Rk, Tk, rr.IDENTITY)[0], Rk)
