"""Op-for-op float32 numpy restatement of ofx_splat_points (occlusionfusion_amd/csrc/splat.hip): the z-buffer of the
warped model points and the occlusion code of every point.

The model z-buffer has no reference twin (the reference renders a warped marching-cubes mesh with an external renderer),
so this file is what the kernel is pinned to, bit for bit: every product, sum and quotient below is one f32 operation in
the kernel's order (the library is compiled without contraction); divisions are correctly rounded in both. The device
takes a 64-bit atomic minimum per covered pixel; np.minimum.at over the 81 offsets gives the same buffer, because a
minimum does not depend on the order of its arguments.

two_layer_scene() is the scene the occlusion tests share: a small patch 4 cm in front of a larger layer, both facing the
camera, where a tracker without an occlusion gate pulls the hidden part of the rear layer onto the patch.
"""
import numpy as np

import assoc_ref as ar
from oracle import fusion_oracle as fo

F32 = np.float32
RMAX = 4                                           # OFX_SPLAT_RMAX
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
CODES = {0: "visible", 1: "invalid skin", 2: "behind / non-finite / off-image", 3: "back-facing", 4: "occluded"}


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _extent(f, rho, z, live):
    """clamp(ceil((f·rho)/z), 0, RMAX), NaN -> 0; 0 for points that are not live."""
    with np.errstate(all="ignore"):
        r = np.ceil(((f * rho) / z).astype(F32))
    r = np.where(r >= RMAX, RMAX, np.where(r > 0, r, 0))
    return np.where(live, r, 0).astype(np.int64)


def splat_warped(x, n, ok, intr, H, W, rho, margin):
    """The rule from the warped points on: x (P,3) f32, n (P,3) unit normals or None (= (0, 0, -1)), ok (P,) bool (False:
    code 1) -> depth f32 (H,W), index i32 (H,W), code u8 (P,)."""
    x = np.ascontiguousarray(x, F32).reshape(-1, 3)
    P = x.shape[0]
    fx, fy, cx, cy = (F32(t) for t in intr[:4])
    rho, margin = F32(rho), F32(margin)
    ok = np.asarray(ok, bool).reshape(P)
    code = np.where(ok, 0, 1).astype(np.uint8)
    inside, u, v = ar.pixel_f32(x, intr, H, W)
    code[ok & ~inside] = 2
    live = ok & inside
    n = np.tile(np.array([0, 0, -1], F32), (P, 1)) if n is None else np.ascontiguousarray(n, F32).reshape(P, 3)
    with np.errstate(all="ignore"):
        s = _dot(n, x)
        back = ~(s < 0)
    code[live & back] = 3
    live = live & ~back
    z = x[:, 2]
    ru, rv = _extent(fx, rho, z, live), _extent(fy, rho, z, live)
    idx = np.arange(P, dtype=np.uint64)
    zb = np.full(H * W, EMPTY)
    r2 = rho * rho
    for dv in range(-RMAX, RMAX + 1):
        for du in range(-RMAX, RMAX + 1):
            uu, vv = u + du, v + dv
            m = live & (abs(du) <= ru) & (abs(dv) <= rv) & (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            if du == 0 and dv == 0:
                zp = z
            else:
                with np.errstate(all="ignore"):
                    dx, dy = (uu.astype(F32) - cx) / fx, (vv.astype(F32) - cy) / fy
                    den = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
                    zp = (s / den).astype(F32)
                    ex, ey, ez = dx * zp - x[:, 0], dy * zp - x[:, 1], zp - z
                    d2 = (ex * ex + ey * ey) + ez * ez
                    m = m & (den < 0) & (zp > 0) & np.isfinite(zp) & (d2 <= r2)
            key = (np.ascontiguousarray(zp, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
            np.minimum.at(zb, (vv * W + uu)[m], key[m])
    empty = zb == EMPTY
    depth = np.where(empty, F32(0), (zb >> np.uint64(32)).astype(np.uint32).view(F32)).astype(F32).reshape(H, W)
    index = np.where(empty, -1, (zb & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32).reshape(H, W)
    with np.errstate(all="ignore"):
        occ = (z - depth[v, u]) > margin
    code[live & occ] = 4
    return depth, index, code


def splat(points, normals, anchors, weights, valid, node_R, node_T, nodes, intr, H, W, splat_radius, occl_margin=0.01):
    """The whole call: dict(depth (H,W) f32, index (H,W) i32, code u8 (P,), warped (P,3), warped_normals (P,3) or
    None). A point with valid == 0 (or an anchor outside the graph) keeps its position and its normal."""
    x = np.ascontiguousarray(points, F32).reshape(-1, 3)
    P = x.shape[0]
    a = np.asarray(anchors, np.int32).reshape(P, 4)
    w = np.asarray(weights, F32).reshape(P, 4)
    N = np.asarray(nodes).reshape(-1, 3).shape[0]
    ok = np.ones(P, bool) if valid is None else np.asarray(valid).reshape(P) != 0
    ok = ok & ((a >= 0) & (a < N)).all(1)
    warped = fo.ed_warp(x, a, w, ok, node_R, node_T, nodes) if P else x.copy()
    nw = None
    if normals is not None:
        n = np.ascontiguousarray(normals, F32).reshape(P, 3)
        with np.errstate(all="ignore"):
            nw = ar.warp_normals(n, np.where(ok[:, None], a, 0), w, node_R) if P else n.copy()
        nw = np.where(ok[:, None], nw, n).astype(F32)
    depth, index, code = splat_warped(warped, nw, ok, intr, H, W, splat_radius, occl_margin)
    return {"depth": depth, "index": index, "code": code, "warped": warped, "warped_normals": nw}


def random_cloud(seed=3, P=3000):
    """Warped points in front of the 33 x 33 camera (100, 100, 16, 16) for the permutation tests: normals scattered about
    (0, 0, -1) (some back-facing), 200 exact duplicates (tied z on all of their pixels), points off the image, one NaN
    point and 5 % marked invalid -> (x, n, ok)."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-0.2, 0.2, P), rng.uniform(-0.2, 0.2, P), rng.uniform(0.8, 1.3, P)], 1).astype(F32)
    n = rng.normal(size=(P, 3)) * 0.5 + np.array([0, 0, -1.0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    x[:200] = x[200:400]
    n[:200] = n[200:400]
    x[-1] = np.nan
    ok = rng.uniform(size=P) > 0.05
    return x, n, ok


# ----------------------------------------------------------------------------------------------- the two-layer scene
def _grid(x0, x1, y0, y1, z, h):
    xs, ys = np.arange(x0, x1 + 1e-9, h), np.arange(y0, y1 + 1e-9, h)
    X, Y = np.meshgrid(xs, ys)
    return np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1).astype(F32)


def two_layer_scene():
    """A rear layer at z = 1.04 (0.48 x 0.32 m) and a front patch at z = 1.0 (0.16 x 0.16 m), both sampled on 4 mm
    grids with normals (0, 0, -1), skinned to nodes on 4 cm grids of both layers; the depth image is the analytic render
    of the two layers under bench_camera(4). -> dict(points, normals, anchors, weights, nodes, edges, edge_weights, depth,
    intr, H, W, hidden (P,) bool: the rear points behind the patch, hidden_nodes (N,) bool: the nine rear nodes with |x|,
    |y| <= 0.05, n_rear)."""
    from occlusionfusion_amd import synthetic as S
    cam = S.bench_camera(4)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    H, W = cam.height, cam.width
    zf, zr = F32(1.0), F32(1.04)
    rear, front = _grid(-0.24, 0.24, -0.16, 0.16, zr, 0.004), _grid(-0.08, 0.08, -0.08, 0.08, zf, 0.004)
    pts = np.concatenate([rear, front])
    P = pts.shape[0]
    is_rear = np.arange(P) < rear.shape[0]
    nrm = np.tile(np.array([0, 0, -1], F32), (P, 1))
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
    hitf = (np.abs(dx * float(zf)) <= 0.08) & (np.abs(dy * float(zf)) <= 0.08)
    hitr = (np.abs(dx * float(zr)) <= 0.24) & (np.abs(dy * float(zr)) <= 0.16)
    depth = np.where(hitf, zf, np.where(hitr, zr, 0)).astype(F32)
    nodes = np.concatenate([_grid(-0.24, 0.24, -0.16, 0.16, zr, 0.04), _grid(-0.08, 0.08, -0.08, 0.08, zf, 0.04)])
    d = np.linalg.norm(pts[:, None, :].astype(np.float64) - nodes[None].astype(np.float64), axis=2)
    a = np.argsort(d, 1, kind="stable")[:, :4].astype(np.int32)
    dd = np.take_along_axis(d, a.astype(np.int64), 1)
    w = np.exp(-dd ** 2 / (2 * 0.02 ** 2))
    w = (w / w.sum(1, keepdims=True)).astype(F32)
    edges = np.asarray(S.euclidean_edges(nodes, 8)[0], np.int32)
    hidden = is_rear & (np.abs(pts[:, 0] / pts[:, 2] * float(zf)) <= 0.08) \
        & (np.abs(pts[:, 1] / pts[:, 2] * float(zf)) <= 0.08)
    hn = (np.abs(nodes[:, 0]) <= 0.05) & (np.abs(nodes[:, 1]) <= 0.05) & (nodes[:, 2] > 1.02)
    return {"points": pts, "normals": nrm, "anchors": a, "weights": w, "nodes": nodes, "edges": edges,
            "edge_weights": np.ones_like(edges, dtype=F32), "depth": depth, "intr": intr, "H": H, "W": W,
            "hidden": hidden, "hidden_nodes": hn, "n_rear": int(rear.shape[0])}
