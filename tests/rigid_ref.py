"""Numpy restatement of ofx_rigid_icp (occlusionfusion_amd/csrc/rigid.hip) and of association.fold_rigid.

Rigid point-to-plane ICP has no reference twin, so this file is what the kernel is pinned to. Per point everything is
f32, one operation per rounding in the kernel's order (the library is compiled without contraction): codes, rows J and
residuals r are reproduced bit for bit. The normal equations are the correctly rounded sums (math.fsum) of the exact f64
products; the kernel's fixed-order f64 sums differ from them by the summation error only. The solve and the pose update
are f64. The warp and the whole gate from the pixel to the cosine test are assoc_ref's / the oracle's.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
IDENTITY = np.eye(3, 4)
# systems row layout (ofx_rigid_icp)
A_SL, B_SL, RR, COUNT, STATUS, WNORM, VNORM = slice(0, 21), slice(21, 27), 27, 28, 29, 30, 31
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def _rigid_rows(R, t, x):
    """((R_a0·x + R_a1·y) + R_a2·z) + t_a per row a, f32; t None: no translation (normals)."""
    cols = []
    for a in range(3):
        v = (R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]) + R[a, 2] * x[:, 2]
        cols.append(v if t is None else v + t[a])
    return np.stack(cols, 1).astype(F32)


def rows(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image, pose, dist_max=0.05,
         cos_min=0.5, edge_max=0.03):
    """One iteration's per-point part: (code u8[P], J f32[P,6], r f32[P]); J and r are zero where code != 0. The
    association's gate (assoc_ref.project_gate) with y = Rf x' + tf and m = Rf n' in place of x' and n'."""
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    Rf, tf = pose[:, :3].astype(F32), pose[:, 3].astype(F32)
    ok, warped, nw = ar.warp_skinned(points, normals, anchors, weights, valid, node_R, node_T, nodes)
    P = warped.shape[0]
    J, r = np.zeros((P, 6), F32), np.zeros(P, F32)
    if P == 0:
        return np.zeros(0, np.uint8), J, r
    with np.errstate(all="ignore"):
        y = _rigid_rows(Rf, tf, warped)
        m = _rigid_rows(Rf, None, nw) if nw is not None else None
        code, live, _, nq, e = ar.project_gate(ok, y, m, intr, point_image, dist_max, cos_min, edge_max)
        res = ar._dot(e, nq)
        cr = np.stack([y[:, 1] * nq[:, 2] - y[:, 2] * nq[:, 1], y[:, 2] * nq[:, 0] - y[:, 0] * nq[:, 2],
                       y[:, 0] * nq[:, 1] - y[:, 1] * nq[:, 0]], 1)
    J[live, :3], J[live, 3:], r[live] = cr[live], nq[live], res[live]
    return code, J, r


def system(code, J, r):
    """The normal equations of the accepted rows -> (row f64[32] with status / norms zero, mag f64[28]): entries 0..27
    are math.fsum of the exact products (a product of two f32 values is exact in f64), mag their Σ|term| (what the
    summation-error bound of any fixed order is stated in), entry 28 the accepted count."""
    acc = code == 0
    Jd, rd = J[acc].astype(np.float64), r[acc].astype(np.float64)
    terms = [Jd[:, i] * Jd[:, j] for i, j in UPPER] + [Jd[:, i] * rd for i in range(6)] + [rd * rd]
    row, mag = np.zeros(32), np.zeros(28)
    for k, t in enumerate(terms):
        row[k] = math.fsum(t.tolist())
        mag[k] = math.fsum(np.abs(t).tolist())
    row[COUNT] = int(acc.sum())
    return row, mag


def unpack(row):
    """(A 6x6 symmetric undamped, b) of a systems row."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(UPPER):
        A[i, j] = A[j, i] = row[k]
    return A, np.array(row[B_SL], np.float64)


def damped(A, damping):
    return A + (damping * np.trace(A) / 6.0) * np.eye(6)


def exp_so3(w):
    """Rodrigues in f64, the series for |ω| < 1e-8."""
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-8:
        ca, cb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        ca, cb = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + ca * K + cb * (K @ K)


def apply_twist(pose, xi):
    """pose <- [ΔR·R | ΔR·t + v], ΔR = exp(ω), ξ = (ω, v)."""
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    dR = exp_so3(np.asarray(xi[:3], np.float64))
    return np.concatenate([dR @ pose[:, :3], (dR @ pose[:, 3] + xi[3:])[:, None]], 1)


def solve(row, pose, damping=1e-6, min_matches=6):
    """Status, twist and new pose of one system row -> (row with status / |ω| / |v| filled in, pose, ξ)."""
    row = np.array(row, np.float64)
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    xi = np.zeros(6)
    if row[COUNT] < min_matches:
        row[STATUS] = 1
        return row, pose, xi
    A, b = unpack(row)
    try:
        L = np.linalg.cholesky(damped(A, damping))
    except np.linalg.LinAlgError:
        row[STATUS] = 2
        return row, pose, xi
    xi = np.linalg.solve(L.T, np.linalg.solve(L, b))
    if not np.isfinite(xi).all():
        row[STATUS] = 2
        return row, pose, np.zeros(6)
    row[STATUS], row[WNORM], row[VNORM] = 0, np.linalg.norm(xi[:3]), np.linalg.norm(xi[3:])
    return row, apply_twist(pose, xi), xi


def icp(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image, pose=None, iters=4,
        dist_max=0.05, cos_min=0.5, edge_max=0.03, damping=1e-6, min_matches=6, stop_twist=0.0):
    """The whole call -> dict(pose (3,4) f64, systems (iters,32), code of the last iteration that ran, poses: the pose
    before each executed iteration)."""
    pose = IDENTITY.copy() if pose is None else np.array(pose, np.float64).reshape(3, 4)
    P = np.asarray(points).reshape(-1, 3).shape[0]
    systems = np.zeros((iters, 32))
    code = np.zeros(P, np.uint8)
    if P == 0:
        systems[:, STATUS] = 1
        return {"pose": pose, "systems": systems, "code": code, "poses": []}
    stopped, poses = False, []
    for it in range(iters):
        if stopped:
            systems[it, STATUS] = 3
            continue
        poses.append(pose.copy())
        code, J, r = rows(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image, pose,
                          dist_max, cos_min, edge_max)
        row, pose, _ = solve(system(code, J, r)[0], pose, damping, min_matches)
        systems[it] = row
        stopped = row[STATUS] != 0 or (row[WNORM] < stop_twist and row[VNORM] < stop_twist)
    return {"pose": pose, "systems": systems, "code": code, "poses": poses}


def fold_rigid(nodes, rot, trans, pose):
    """R_k' = R·R_k, T_k' = R·(g_k + T_k) + t − g_k in f64, rounded once to f32; None = identity / zero."""
    g = np.asarray(nodes, np.float64).reshape(-1, 3)
    N = g.shape[0]
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    R, t = pose[:, :3], pose[:, 3]
    Rk = np.broadcast_to(np.eye(3), (N, 3, 3)) if rot is None else np.asarray(rot, np.float64).reshape(N, 3, 3)
    Tk = np.zeros((N, 3)) if trans is None else np.asarray(trans, np.float64).reshape(N, 3)
    return (np.einsum("ij,njk->nik", R, Rk).astype(F32), ((g + Tk) @ R.T + t - g).astype(F32))


INTR_C, H_C, W_C = (60.0, 60.0, 31.5, 23.5), 48, 64


def corner_scene():
    """A room corner seen from inside, 64x48: three mutually non-parallel planes n_i·p = d_i through one apex, with
    n_i pointing away from the camera. The camera is inside the convex room {n_i·p <= d_i}, so a ray leaves it through
    the nearest plane it meets: depth = min_i d_i / (n_i·ray). Analytic, no holes. -> (depth f32 (H,W), n (3,3), d (3,),
    apex)."""
    apex = np.array([0.02, -0.01, 1.3])
    n = np.array([[0.62, 0.18, 0.76], [-0.58, 0.30, 0.76], [0.05, -0.70, 0.71]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = n @ apex
    z, _ = _corner_hits(n, d, *np.meshgrid(np.arange(W_C, dtype=np.float64), np.arange(H_C, dtype=np.float64)))
    return z.astype(F32), n, d, apex


def _corner_hits(n, d, u, v):
    fx, fy, cx, cy = INTR_C
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    den = ray @ n.T
    assert (den > 0).all()
    z = d / den
    return z.min(-1), z.argmin(-1)


def corner_points(n, d, count, rng):
    """`count` surface points of the corner at random sub-pixel positions (6 pixels inside the image) and their unit
    normals towards the camera -> (points f32 (count,3), normals f32 (count,3))."""
    fx, fy, cx, cy = INTR_C
    u, v = rng.uniform(6, W_C - 7, count), rng.uniform(6, H_C - 7, count)
    z, k = _corner_hits(n, d, u, v)
    pts = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    return pts.astype(F32), (-n[k]).astype(F32)


def rigid_about(axis, degrees, centre, trans):
    """(3,4) pose p -> R(p − c) + c + T."""
    R = exp_so3(np.asarray(axis, np.float64) / np.linalg.norm(axis) * math.radians(degrees))
    c = np.asarray(centre, np.float64)
    return np.concatenate([R, (c - R @ c + np.asarray(trans, np.float64))[:, None]], 1)


def invert(pose):
    R, t = pose[:, :3], pose[:, 3]
    return np.concatenate([R.T, (-R.T @ t)[:, None]], 1)


def pose_error(pose, truth, centre):
    """(rotation angle of R·R_truthᵀ in radians, distance between the two images of `centre`)."""
    dR = pose[:, :3] @ truth[:, :3].T
    ang = math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0)))
    c = np.asarray(centre, np.float64)
    return ang, float(np.linalg.norm(pose[:, :3] @ c + pose[:, 3] - truth[:, :3] @ c - truth[:, 3]))


def knn_skin(points, nodes, sigma=0.15):
    """A plain 4-nearest-node skin (f64 distances, weights exp(-d²/2σ²) normalised to sum 1 in f32): anchors i32 (P,4),
    weights f32 (P,4). Test plumbing only; any valid skin serves."""
    p, g = np.asarray(points, np.float64), np.asarray(nodes, np.float64)
    d2 = ((p[:, None, :] - g[None, :, :]) ** 2).sum(-1)
    a = np.argsort(d2, 1, kind="stable")[:, :4]
    w = np.exp(-np.take_along_axis(d2, a, 1) / (2 * sigma * sigma))
    w = (w / w.sum(1, keepdims=True)).astype(F32)
    return a.astype(np.int32), w


def corner_problem(count=1500, n_nodes=12, seed=11):
    """The corner scene with `count` model points moved off it: the surface points taken through the inverse of a known
    pose (3° about (0.3, 1, 0.2) through the apex, 2 cm), so that aligning from the identity must find that pose. Node
    transforms are the identity (the ED warp then only rounds). -> dict(pts, nrm, anchors, weights, nodes, R, T, vmap,
    depth, truth, apex)."""
    rng = np.random.default_rng(seed)
    depth, n, d, apex = corner_scene()
    surf, snrm = corner_points(n, d, count, rng)
    truth = rigid_about((0.3, 1.0, 0.2), 3.0, apex, (0.012, -0.008, 0.0139))
    inv = invert(truth)
    pts = (surf.astype(np.float64) @ inv[:, :3].T + inv[:, 3]).astype(F32)
    nrm = (snrm.astype(np.float64) @ inv[:, :3].T).astype(F32)
    nodes = pts[rng.choice(count, n_nodes, replace=False)].copy()
    a, w = knn_skin(pts, nodes)
    return dict(pts=pts, nrm=nrm, anchors=a, weights=w, nodes=nodes,
                R=np.broadcast_to(np.eye(3, dtype=F32), (n_nodes, 3, 3)).copy(), T=np.zeros((n_nodes, 3), F32),
                vmap=fo.backproject_depth(depth, *INTR_C), depth=depth, truth=truth, apex=apex)
