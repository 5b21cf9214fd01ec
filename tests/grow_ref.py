"""numpy restatement of ofx_grow_nodes (include/ofx.h), op for op: the yardstick the kernels are compared with bit for
bit (tests/test_gpu_grow.py), itself checked against closed-form answers (tests/test_grow_ref.py). numpy evaluates f32
and f64 expressions one rounding per operation (no contraction); f64 sqrt and division are correctly rounded: the same
steps as the kernels'. The selection is the plain sequential loop the kernel has to equal."""
import numpy as np

F32 = np.float32
F64 = np.float64


def sqdist(p, q):
    """(dx² + dy²) + dz² in f32 between broadcastable (.., 3) arrays (the ofx_knn_points form)."""
    d = np.asarray(p, F32) - np.asarray(q, F32)
    a, b, c = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
    return (a + b) + c


def sqrt_rn(x):
    """Correctly rounded f32 square root (through f64)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F32).astype(F64)).astype(F32)


def dist_min(points, nodes, chunk=4096):
    """f32 distance of every point to its nearest node (NaN distances skipped, as fminf)."""
    points, nodes = np.asarray(points, F32).reshape(-1, 3), np.asarray(nodes, F32).reshape(-1, 3)
    out = np.full(points.shape[0], np.inf, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, points.shape[0], chunk):
            d2 = sqdist(points[s:s + chunk, None, :], nodes[None, :, :])
            out[s:s + chunk] = np.fmin.reduce(d2, axis=1, initial=np.inf)
    return sqrt_rn(out)


def candidates(points, anchors, valid, nodes, min_dist):
    """Candidate flags (M,) bool."""
    points = np.asarray(points, F32).reshape(-1, 3)
    a = np.asarray(anchors, np.int64).reshape(-1, 4)
    n = np.asarray(nodes).reshape(-1, 3).shape[0]
    ok = (np.asarray(valid).reshape(-1) != 0) & np.isfinite(points).all(1) & ((a >= 0) & (a < n)).all(1)
    with np.errstate(invalid="ignore"):
        return ok & (dist_min(points, nodes) > F32(min_dist))


def select(points, rows, spacing, max_new):
    """The sequential greedy loop over the candidate rows (ascending) -> (selected rows, capped)."""
    points = np.asarray(points, F32).reshape(-1, 3)
    spacing = F32(spacing)
    sel, pos = [], np.empty((0, 3), F32)
    for r in rows:
        if len(sel) and (sqrt_rn(sqdist(pos, points[r])) < spacing).any():
            continue
        if len(sel) == int(max_new):
            return np.asarray(sel, np.int64), 1
        sel.append(int(r))
        pos = np.concatenate([pos, points[r][None]], 0)
    return np.asarray(sel, np.int64), 0


def ed_warp(p, anchors, weights, nodes, R, T):
    """ofx_deform_points (normals = 0, K = 4) of points (S,3) under node-relative (R (N,3,3), T, nodes): f32,
    y_k = ((R_k(x - g_k) + g_k) + t_k)·w_k with R d = (R0·dx + R1·dy) + R2·dz, summed from y_0 in anchor order."""
    p = np.asarray(p, F32).reshape(-1, 3)
    R = np.asarray(R, F32).reshape(-1, 3, 3)
    T, nodes = np.asarray(T, F32).reshape(-1, 3), np.asarray(nodes, F32).reshape(-1, 3)
    a, w = np.asarray(anchors, np.int64).reshape(-1, 4), np.asarray(weights, F32).reshape(-1, 4)
    acc = None
    for k in range(4):
        Rk, g, t = R[a[:, k]], nodes[a[:, k]], T[a[:, k]]
        d = p - g
        r = Rk[:, :, 0] * d[:, 0:1]
        r = r + Rk[:, :, 1] * d[:, 1:2]
        r = r + Rk[:, :, 2] * d[:, 2:3]
        y = ((r + g) + t) * w[:, k:k + 1]
        acc = y if acc is None else acc + y
    return acc


def quat_of(m):
    """(S,3,3) f64 rotation matrices -> unit quaternions (S,4) as (w, x, y, z): Shepperd's form, the branch of the largest
    of (trace, m00, m11, m22), the first of equals."""
    m = np.asarray(m, F64).reshape(-1, 3, 3)
    q = np.empty((m.shape[0], 4), F64)
    for i, M in enumerate(m):
        m00, m11, m22 = M[0, 0], M[1, 1], M[2, 2]
        tr = (m00 + m11) + m22
        br, big = 0, tr
        for b, v in ((1, m00), (2, m11), (3, m22)):
            if v > big:
                br, big = b, v
        with np.errstate(all="ignore"):
            if br == 0:
                s = np.sqrt(tr + 1.0) * 2.0
                v = (0.25 * s, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s)
            elif br == 1:
                s = np.sqrt(((1.0 + m00) - m11) - m22) * 2.0
                v = ((M[2, 1] - M[1, 2]) / s, 0.25 * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s)
            elif br == 2:
                s = np.sqrt(((1.0 + m11) - m00) - m22) * 2.0
                v = ((M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, 0.25 * s, (M[1, 2] + M[2, 1]) / s)
            else:
                s = np.sqrt(((1.0 + m22) - m00) - m11) * 2.0
                v = ((M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, 0.25 * s)
            v = np.array(v, F64)
            n = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
            q[i] = v / n if (n > 0.0 and np.isfinite(n)) else (1.0, 0.0, 0.0, 0.0)
    return q


def blend_rotations(anchors, weights, R):
    """The f64 quaternion blend of each row's four anchor rotations -> (S,3,3) f32."""
    a, w = np.asarray(anchors, np.int64).reshape(-1, 4), np.asarray(weights, F32).reshape(-1, 4).astype(F64)
    R = np.asarray(R, F32).reshape(-1, 3, 3).astype(F64)
    S = a.shape[0]
    q0 = quat_of(R[a[:, 0]])
    acc = w[:, 0:1] * q0
    for k in range(1, 4):
        q = quat_of(R[a[:, k]])
        dot = ((q0[:, 0] * q[:, 0] + q0[:, 1] * q[:, 1]) + q0[:, 2] * q[:, 2]) + q0[:, 3] * q[:, 3]
        sg = np.where(dot < 0.0, -1.0, 1.0)[:, None]
        acc = acc + w[:, k:k + 1] * (sg * q)
    with np.errstate(all="ignore"):
        n = np.sqrt(((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]) + acc[:, 3] * acc[:, 3])
        ok = (n > 0.0) & np.isfinite(n)
        q = np.where(ok[:, None], acc / np.where(ok, n, 1.0)[:, None], np.array([1.0, 0.0, 0.0, 0.0]))
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    out = np.empty((S, 3, 3), F64)
    out[:, 0, 0] = 1.0 - 2.0 * (qy * qy + qz * qz)
    out[:, 0, 1] = 2.0 * (qx * qy - qz * qw)
    out[:, 0, 2] = 2.0 * (qx * qz + qy * qw)
    out[:, 1, 0] = 2.0 * (qx * qy + qz * qw)
    out[:, 1, 1] = 1.0 - 2.0 * (qx * qx + qz * qz)
    out[:, 1, 2] = 2.0 * (qy * qz - qx * qw)
    out[:, 2, 0] = 2.0 * (qx * qz - qy * qw)
    out[:, 2, 1] = 2.0 * (qy * qz + qx * qw)
    out[:, 2, 2] = 1.0 - 2.0 * (qx * qx + qy * qy)
    return out.astype(F32)


def edge_rows(nodes_all, first, k_e, node_coverage):
    """Edge rows of the nodes [first, len(nodes_all)): the k_e nearest other nodes by (f32 d², id) and their weights."""
    X = np.asarray(nodes_all, F32).reshape(-1, 3)
    n_all, S = X.shape[0], X.shape[0] - first
    cov = F32(node_coverage)
    two_c2 = (F32(2.0) * cov) * cov
    E = -np.ones((S, k_e), np.int32)
    W = np.zeros((S, k_e), F32)
    for j in range(S):
        me = first + j
        d2 = sqdist(X, X[me])
        ids = np.arange(n_all)
        keep = ids != me
        order = np.lexsort((ids[keep], d2[keep]))[:k_e]
        nb, dd = ids[keep][order], d2[keep][order]
        d = sqrt_rn(dd)
        with np.errstate(all="ignore"):
            w = np.exp(((-(d * d)).astype(F64) / F64(two_c2)).astype(F32).astype(F64)).astype(F32)
            s = F32(0.0)
            for v in w:
                s = F32(s + v)
            den = s if s > 0 else F32(len(nb))
            E[j, :len(nb)] = nb
            W[j, :len(nb)] = (w.astype(F64) / F64(den)).astype(F32)
    return E, W


def grow_nodes(points, anchors, weights, valid, nodes, R, T, edges, edge_weights, node_coverage, min_dist, spacing,
               max_new):
    """The whole call on host arrays holding exactly n_nodes rows -> dict(nodes, R (.,3,3), T, edges, edge_weights: the
    grown arrays (n_nodes + selected rows), count i32 [candidates, selected, capped], rows: the selected model rows)."""
    points = np.asarray(points, F32).reshape(-1, 3)
    nodes = np.asarray(nodes, F32).reshape(-1, 3)
    R, T = np.asarray(R, F32).reshape(-1, 3, 3), np.asarray(T, F32).reshape(-1, 3)
    edges, edge_weights = np.asarray(edges, np.int32), np.asarray(edge_weights, F32)
    n = nodes.shape[0]
    out = {"nodes": nodes, "R": R, "T": T, "edges": edges, "edge_weights": edge_weights,
           "count": np.zeros(3, np.int32), "rows": np.empty(0, np.int64)}
    if points.shape[0] == 0 or int(max_new) == 0:
        return out
    flag = candidates(points, anchors, valid, nodes, min_dist)
    rows, capped = select(points, np.nonzero(flag)[0], spacing, max_new)
    out["count"] = np.array([int(flag.sum()), rows.shape[0], capped], np.int32)
    out["rows"] = rows
    if rows.shape[0] == 0:
        return out
    p = points[rows]
    a, w = np.asarray(anchors).reshape(-1, 4)[rows], np.asarray(weights, F32).reshape(-1, 4)[rows]
    out["nodes"] = np.concatenate([nodes, p], 0)
    out["T"] = np.concatenate([T, ed_warp(p, a, w, nodes, R, T) - p], 0)
    out["R"] = np.concatenate([R, blend_rotations(a, w, R)], 0)
    E, W = edge_rows(out["nodes"], n, edges.shape[1], node_coverage)
    out["edges"] = np.concatenate([edges, E], 0)
    out["edge_weights"] = np.concatenate([edge_weights, W], 0)
    return out


def brick_reach(dims, origin, voxel_size, nodes, node_coverage):
    """(n_bricks, N) bool: node within the cull radius of the brick's AABB (k_brick_cull's test, f32; bricks numbered
    (bx*nby + by)*nbz + bz over the whole volume)."""
    D = [int(d) for d in dims]
    nb = [(d + 7) // 8 for d in D]
    o, vs = np.asarray(origin, F32).astype(F64), float(voxel_size)
    r = 4.0 * float(node_coverage) * (1.0 + 1e-4) + 1e-6
    cull_r2 = F32(r * r)
    X = np.asarray(nodes, F32).reshape(-1, 3)
    e2 = None
    grids = np.meshgrid(*[np.arange(n) for n in nb], indexing="ij")
    for a in range(3):
        i0 = grids[a].reshape(-1) * 8
        i1 = np.minimum(i0 + 7, D[a] - 1)
        lo = (o[a] + vs * i0.astype(F64)).astype(F32)[:, None]
        hi = (o[a] + vs * i1.astype(F64)).astype(F32)[:, None]
        e = np.maximum(np.maximum(lo - X[None, :, a], X[None, :, a] - hi), F32(0))
        e2 = e * e if e2 is None else e2 + e * e
    return e2 <= cull_r2


def skin_grow_plan(dims, origin, voxel_size, nodes_all, n_old, node_coverage, k, brick_list):
    """ofx_skin_grow_plan's brick sets -> (re-skinned: the touched listed bricks, ascending id; appended: the touched
    unlisted bricks with >= k of all nodes within the cull radius, ascending id)."""
    reach = brick_reach(dims, origin, voxel_size, nodes_all, node_coverage)
    touched = reach[:, n_old:].any(1)
    listed = np.zeros(reach.shape[0], bool)
    listed[np.asarray(brick_list, np.int64)] = True
    return np.nonzero(touched & listed)[0], np.nonzero(touched & ~listed & (reach.sum(1) >= k))[0]


def listed_bricks(dims, origin, voxel_size, nodes, node_coverage, k):
    """ofx_skin_volume_bricks' list: bricks with >= k nodes within the cull radius, ascending."""
    return np.nonzero(brick_reach(dims, origin, voxel_size, nodes, node_coverage).sum(1) >= k)[0]
