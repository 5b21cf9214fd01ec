"""numpy restatement of ofx_surface_points (include/ofx.h), op for op: the yardstick the kernel is compared with bit for
bit (tests/test_gpu_surface.py), itself checked against closed-form answers (tests/test_surface_ref.py). It works on the
dense C-order volume and the dense skin (WarpField.skin_tsdf / ofx_skin_volume_to_dense: anchors -1 = none); the brick
list only fixes which voxels are visited and in which order. numpy evaluates f32 expressions one rounding per operation
(no contraction), f64 sqrt and division are correctly rounded: the same steps as the kernel's."""
import numpy as np

F32 = np.float32
CODES = {0: "accepted", 1: "padding / boundary layer", 2: "unobserved", 3: "not in [0, 1)", 4: "unobserved neighbour",
         5: "no negative neighbour", 6: "degenerate gradient", 7: "invalid skin"}


def cdiv(a, b):
    """f32 a / b correctly rounded (through f64, as the kernel's cdiv)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(np.float64) / np.asarray(b, F32).astype(np.float64)).astype(F32)


def classify(tsdf, weight, skin_anchors, w_min):
    """Dense pass -> (code u8 (Dx,Dy,Dz), g f32 (3,Dx,Dy,Dz), len f32 (Dx,Dy,Dz)). Neighbours come from np.roll: it wraps
    at the volume's faces, where the voxel is code 1 whatever it reads."""
    phi = np.ascontiguousarray(tsdf, F32)
    w = np.ascontiguousarray(weight, F32)
    D = phi.shape
    w_min = F32(w_min)
    with np.errstate(all="ignore"):
        inner = np.zeros(D, bool)
        inner[1:-1, 1:-1, 1:-1] = True
        seen = np.ones(D, bool)
        neg = np.zeros(D, bool)
        g = np.empty((3,) + D, F32)
        for a in range(3):
            hi, lo = np.roll(phi, -1, a), np.roll(phi, 1, a)          # phi(+e_a), phi(-e_a)
            seen &= (np.roll(w, -1, a) >= w_min) & (np.roll(w, 1, a) >= w_min)
            neg |= (hi < 0) | (lo < 0)
            g[a] = hi - lo
        l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        ln = np.sqrt(l2.astype(np.float64)).astype(F32)
        degenerate = ~(l2 > 0) | ~np.isfinite(l2) | (phi > ln)
        no_skin = (np.asarray(skin_anchors).reshape(D + (4,)) < 0).any(-1)
        code = np.select([~inner, ~(w >= w_min), ~((phi >= 0) & (phi < 1)), ~seen, ~neg, degenerate, no_skin],
                         [1, 2, 3, 4, 5, 6, 7], 0).astype(np.uint8)
    return code, g, ln


def listed_voxels(dims, brick_list):
    """(i, j, k, inside) int arrays (n_list, 512): the voxels of the listed bricks in (slot, l = (lx*8 + ly)*8 + lz)
    order; inside = not brick padding. Bricks are numbered ((bx*nby) + by)*nbz + bz."""
    Dx, Dy, Dz = (int(d) for d in dims)
    nby, nbz = (Dy + 7) // 8, (Dz + 7) // 8
    b = np.asarray(brick_list, np.int64).reshape(-1, 1)
    l = np.arange(512, dtype=np.int64).reshape(1, -1)
    i = (b // nbz // nby) * 8 + (l >> 6)
    j = (b // nbz % nby) * 8 + ((l >> 3) & 7)
    k = (b % nbz) * 8 + (l & 7)
    return i, j, k, (i < Dx) & (j < Dy) & (k < Dz)


def emitted_ranks(n, max_points):
    """Ranks of the accepted voxels that are emitted (ofx_associate's rule): all for n <= max_points, else rank r iff
    floor((r+1)*max/n) > floor(r*max/n) in integers."""
    n, m = int(n), int(max_points)
    if n <= m:
        return np.arange(n, dtype=np.int64)
    r = np.arange(n, dtype=np.int64)
    return r[((r + 1) * m) // n > (r * m) // n]


def surface_points(tsdf, weight, origin, voxel_size, brick_list, skin_anchors, skin_weights, w_min=1.0, max_points=0):
    """The whole call -> dict(points, normals f32 (M,3), anchors i32 (M,4), weights f32 (M,4), voxel i32 (M,), valid u8
    (M,), code u8 (n_list*512,), count i32 [accepted, emitted]) with M = max_points padded rows."""
    phi = np.ascontiguousarray(tsdf, F32)
    D = phi.shape
    M = int(max_points)
    code_d, g, ln = classify(phi, weight, skin_anchors, w_min)
    i, j, k, inside = listed_voxels(D, brick_list)
    ic, jc, kc = np.minimum(i, D[0] - 1), np.minimum(j, D[1] - 1), np.minimum(k, D[2] - 1)
    code = np.where(inside, code_d[ic, jc, kc], 1).astype(np.uint8).reshape(-1)
    acc = np.nonzero(code == 0)[0]
    sel = acc[emitted_ranks(acc.shape[0], M)]
    vi, vj, vk = i.reshape(-1)[sel], j.reshape(-1)[sel], k.reshape(-1)[sel]
    E = sel.shape[0]
    out = {"points": np.zeros((M, 3), F32), "normals": np.zeros((M, 3), F32), "anchors": np.zeros((M, 4), np.int32),
           "weights": np.zeros((M, 4), F32), "voxel": np.full(M, -1, np.int32), "valid": np.zeros(M, np.uint8),
           "code": code, "count": np.array([acc.shape[0], E], np.int32)}
    if E:
        o = np.asarray(origin, F32).astype(np.float64)
        vs = float(voxel_size)
        f = phi[vi, vj, vk]
        length = ln[vi, vj, vk]
        two_h = F32(2.0 * vs)
        t = cdiv(f * two_h, length)                                   # the product rounds to f32 first
        vox = (vi * D[1] + vj) * D[2] + vk
        for a, idx in enumerate((vi, vj, vk)):
            c = (o[a] + vs * idx.astype(np.float64)).astype(F32)
            n = cdiv(g[a][vi, vj, vk], length)
            out["normals"][:E, a] = n
            out["points"][:E, a] = c - n * t
        out["anchors"][:E] = np.asarray(skin_anchors, np.int32).reshape(-1, 4)[vox]
        out["weights"][:E] = np.asarray(skin_weights, F32).reshape(-1, 4)[vox]
        out["voxel"][:E] = vox
        out["valid"][:E] = 1
    return out
