"""Op-for-op float32 numpy restatement of ofx_associate (occlusionfusion_amd/csrc/assoc.hip) and of its compaction rule.

Projective association has no reference twin (the reference's matches come from learned front-ends), so this file is
what the kernel is pinned to, bit for bit: every product, sum and quotient below is one f32 operation in the kernel's
order (the library is compiled without contraction); square roots and divisions are correctly rounded in both.
"""
import numpy as np

from oracle import fusion_oracle as fo

F32 = np.float32
POINT, PLANE = 0, 1
CODES = {0: "accepted", 1: "invalid skin", 2: "behind / non-finite / off-image", 3: "hole", 4: "no target normal",
         5: "too far", 6: "normal mismatch"}


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def warp_normals(normals, anchors, weights, node_R):
    """ofx_deform_points, normals = 1 (WarpField.deform_normals): Σ_{k: w_k != 0} w_k (R_k n), accumulated from zero in
    anchor order, then n / sqrt((x² + y²) + z²)."""
    n = np.asarray(normals, F32)
    R = np.asarray(node_R, F32).reshape(-1, 3, 3)
    acc = np.zeros_like(n)
    for k in range(anchors.shape[1]):
        use = weights[:, k] != 0
        Rk = R[np.where(use, anchors[:, k], 0)]
        r = np.stack([(Rk[:, i, 0] * n[:, 0] + Rk[:, i, 1] * n[:, 1]) + Rk[:, i, 2] * n[:, 2] for i in range(3)], 1)
        acc = np.where(use[:, None], acc + weights[:, k:k + 1] * r, acc)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        return (acc / nrm[:, None]).astype(F32)


def pixel_f32(points, intr, H, W):
    """The pixel ofx_visibility_f32 takes for an f32 point (fusion_oracle.check_visibility_f32's projection):
    (x·fx)/z + cx in f32, rint, range test on the rounded value -> (inside, u, v)."""
    p = np.asarray(points, F32)
    fx, fy, cx, cy = (F32(v) for v in intr[:4])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = np.rint(((p[:, 0] * fx) / p[:, 2] + cx).astype(F32))
        v = np.rint(((p[:, 1] * fy) / p[:, 2] + cy).astype(F32))
        inside = np.isfinite(p).all(1) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (p[:, 2] > 0)
    return inside, np.where(inside, u, 0).astype(np.int64), np.where(inside, v, 0).astype(np.int64)


def warp_skinned(points, normals, anchors, weights, valid, node_R, node_T, nodes):
    """Trips 1 and 2 -> (ok bool[P]: valid skin with every anchor inside the graph, warped f32[P,3], warped unit normals
    f32[P,3] or None). Invalid points keep x (ofx_deform_points)."""
    x = np.ascontiguousarray(points, F32).reshape(-1, 3)
    P = x.shape[0]
    a = np.asarray(anchors, np.int32).reshape(P, 4)
    w = np.asarray(weights, F32).reshape(P, 4)
    N = np.asarray(nodes).reshape(-1, 3).shape[0]
    ok = np.ones(P, bool) if valid is None else np.asarray(valid).reshape(P) != 0
    ok = ok & ((a >= 0) & (a < N)).all(1)                        # an anchor outside the graph cannot be gathered
    warped = fo.ed_warp(x, a, w, ok, node_R, node_T, nodes)
    with np.errstate(all="ignore"):
        nw = warp_normals(normals, np.where(ok[:, None], a, 0), w, node_R) if normals is not None else None
    return ok, warped, nw


def project_gate(ok, y, m, intr, point_image, dist_max=0.05, cos_min=0.5, edge_max=0.03):
    """The gate of camera-space points y f32[P,3] with unit normals m (None: no cosine gate), from the pixel to the
    cosine gate; the points outside ok get code 1 -> (code u8[P], live = code == 0, q, nq, e): the target vertex, its
    normal towards the camera and q - y, f32[P,3], meaningful where live. point_image: (3, H, W) f32 vertex map."""
    vm = np.asarray(point_image, F32)
    _, H, W = vm.shape
    dist_max, cos_min, edge_max = F32(dist_max), F32(cos_min), F32(edge_max)
    code = np.where(ok, 0, 1).astype(np.uint8)
    with np.errstate(all="ignore"):
        inside, u, v = pixel_f32(y, intr, H, W)
        code[ok & ~inside] = 2
        live = ok & inside
        q = vm[:, v, u].T                                         # (P, 3)
        code[live & ~(q[:, 2] > 0)] = 3
        live &= q[:, 2] > 0
        border = (u == 0) | (v == 0) | (u == W - 1) | (v == H - 1)
        ul, ur, vu, vd = np.maximum(u - 1, 0), np.minimum(u + 1, W - 1), np.maximum(v - 1, 0), np.minimum(v + 1, H - 1)
        ql, qr, qu, qd = vm[:, v, ul].T, vm[:, v, ur].T, vm[:, vu, u].T, vm[:, vd, u].T
        zs = np.stack([ql[:, 2], qr[:, 2], qu[:, 2], qd[:, 2]], 1)
        no_normal = border | ~(zs > 0).all(1) | (np.abs(zs - q[:, 2:3]) > edge_max).any(1)
        A, B = qr - ql, qd - qu
        c = np.stack([A[:, 1] * B[:, 2] - A[:, 2] * B[:, 1], A[:, 2] * B[:, 0] - A[:, 0] * B[:, 2],
                      A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]], 1)
        l2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        no_normal |= ~((l2 > 0) & np.isfinite(l2))
        code[live & no_normal] = 4
        live &= ~no_normal
        nq = (c / np.sqrt(l2)[:, None]).astype(F32)
        nq = np.where((_dot(nq, q) > 0)[:, None], -nq, nq)
        e = q - y
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        far = d2 > dist_max * dist_max
        code[live & far] = 5
        live &= ~far
        if m is not None:
            away = _dot(m, nq) < cos_min
            code[live & away] = 6
            live &= ~away
    assert np.array_equal(live, code == 0)
    return code, live, q, nq, e


def gate(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image, dist_max=0.05,
         cos_min=0.5, edge_max=0.03, mode=PLANE):
    """Per point: (code u8[P], tgt f32[P,3], warped f32[P,3]): the gate, then the target rule of an accepted point."""
    ok, warped, nw = warp_skinned(points, normals, anchors, weights, valid, node_R, node_T, nodes)
    code, live, q, nq, e = project_gate(ok, warped, nw, intr, point_image, dist_max, cos_min, edge_max)
    with np.errstate(all="ignore"):
        t = warped + nq * _dot(e, nq)[:, None] if mode == PLANE else q
    tgt = np.zeros(warped.shape, F32)
    tgt[live] = t[live]
    return code, tgt, warped


def emitted_ranks(n, max_matches):
    """Ranks (0..n-1, ascending) of the accepted points that are emitted: all of them for n <= max_matches, else rank r
    iff floor((r+1)·max_matches/n) > floor(r·max_matches/n) — exactly max_matches, evenly spread."""
    n, m = int(n), int(max_matches)
    if n <= m:
        return np.arange(n, dtype=np.int64)
    r = np.arange(n, dtype=np.int64)
    return r[((r + 1) * m) // n > (r * m) // n]


def associate(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image, dist_max=0.05,
              cos_min=0.5, edge_max=0.03, mode=PLANE, max_matches=10000):
    """The whole call: dict(code, tgt, warped, match_idx, src, tgt_out, anchors, weights, count = [accepted, emitted])."""
    code, tgt, warped = gate(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, point_image,
                             dist_max, cos_min, edge_max, mode)
    acc = np.nonzero(code == 0)[0]
    idx = acc[emitted_ranks(acc.shape[0], max_matches)].astype(np.int32)
    x = np.ascontiguousarray(points, F32).reshape(-1, 3)
    return {"code": code, "tgt": tgt, "warped": warped, "match_idx": idx, "src": x[idx], "tgt_out": tgt[idx],
            "anchors": np.asarray(anchors, np.int32).reshape(-1, 4)[idx],
            "weights": np.asarray(weights, F32).reshape(-1, 4)[idx],
            "count": np.array([acc.shape[0], idx.shape[0]], np.int32)}


def depth_residual(warped, depth, intr, max_diff=0.1):
    """Mean |depth at the pixel - z| over the warped points whose pixel holds a depth and whose difference is under
    max_diff (metres): the tracking tests' measure of how well a warp explains a depth frame."""
    H, W = depth.shape
    p = np.asarray(warped, F32)
    inside, u, v = pixel_f32(p, intr, H, W)
    d = np.asarray(depth, np.float64)[v, u]
    diff = np.abs(d - p[:, 2].astype(np.float64))
    m = inside & (d > 0) & (diff < max_diff)
    return float(diff[m].mean())
