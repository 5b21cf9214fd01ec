"""Plain numpy restatement of the skin cache and of the fusion that consumes it, built on oracle.fusion_oracle
(world_points, skin, ed_warp, integrate), plus the seeded scenes that drive the skin / palette / integrate kernels to
their edges (tests/test_gpu_skin_cache_edges.py compares the kernels with this, bit for bit; tests/
test_skin_cache_ref.py asserts on the CPU that every scene really reaches the edge it is meant for).

Layout conventions restated here (csrc/ofx_common.h): 8^3 bricks, brick id = (bx * nby + by) * nbz + bz, in-brick voxel
l = (lx * 8 + ly) * 8 + lz; a wave of the integrate kernels holds 64 consecutive l of one brick."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import fusion_oracle as fo

F32, F64 = np.float32, np.float64
TRUNC = fo.TRUNC_MARGIN
PAL = 64          # OFX_PALETTE
BRICK = 8
WEIGHTS = np.array([0, .5, .7, 1, 3], F32)


# ------------------------------------------------------------------------------------------------ restatement
def dense_skin(origin, dims, vs, nodes, cov, k=None):
    """fo.skin over the whole C-order grid, in chunks of <= 4096 points (bounded memory).
    -> anchors i32 (V,K) (-1 = none), weights f32 (V,K), valid bool (V,)."""
    world = fo.world_points(origin, dims, vs)
    out = [fo.skin(world[s:s + 4096], nodes, cov, k) for s in range(0, world.shape[0], 4096)]
    return tuple(np.concatenate([o[i] for o in out], 0) for i in range(3))


def dense_skin_high_ids(origin, dims, vs, nodes, cov, first):
    """dense_skin of a node set whose nodes below `first` are decoys no voxel can reach (farther than 4 sigma from the
    whole grid, asserted): the skin is computed against nodes[first:] only and the ids are shifted by `first`. The remap
    id -> id + first is monotone, so the order of equal distances (lower id first) is the full set's, and a decoy can
    never enter a voxel's K nearest ahead of a reachable node that passes the cut-off; anchors beyond the cut-off are
    -1 either way."""
    nodes = np.asarray(nodes, F32)
    world = fo.world_points(origin, dims, vs)
    lo, hi = world.min(0).astype(F64), world.max(0).astype(F64)
    gap = np.maximum(np.maximum(lo - nodes[:first], nodes[:first] - hi), 0)
    assert (np.sqrt((gap ** 2).sum(1)) > 8 * cov).all(), "a decoy node is within reach of the grid"
    a, w, v = dense_skin(origin, dims, vs, nodes[first:], cov, k=min(4, nodes.shape[0]))
    return np.where(a >= 0, a + first, -1).astype(np.int32), w, v


def brick_index(dims):
    """-> (brick id (V,), in-brick voxel l (V,), number of bricks) of the C-order grid."""
    Dx, Dy, Dz = (int(d) for d in dims)
    i, j, k = np.indices((Dx, Dy, Dz))
    nby, nbz = (Dy + 7) // 8, (Dz + 7) // 8
    b = ((i // 8) * nby + j // 8) * nbz + k // 8
    l = ((i % 8) * 8 + j % 8) * 8 + k % 8
    return b.reshape(-1), l.reshape(-1), ((Dx + 7) // 8) * nby * nbz


def brick_palettes(anchors, valid, dims):
    """k_skin_palette's documented rule: per brick the ascending distinct anchors of its skin-valid voxels
    -> list over bricks of int64 arrays (empty for a brick without a skin-valid voxel)."""
    b, _, nb = brick_index(dims)
    valid = np.asarray(valid, bool)
    return [np.unique(anchors[valid & (b == q)]).astype(np.int64) for q in range(nb)]


def clipped_axes(dims):
    """-> bool (n_bricks, 3): brick is cut by the volume's end along x / y / z."""
    Dx, Dy, Dz = (int(d) for d in dims)
    nb = [(d + 7) // 8 for d in (Dx, Dy, Dz)]
    bx, by, bz = np.indices(nb).reshape(3, -1)
    return np.stack([bx * 8 + 8 > Dx, by * 8 + 8 > Dy, bz * 8 + 8 > Dz], 1)


def two_frame_fusion(sc, skin, state, obs_weight, R=None, T=None, depth=None, color_im=None, intr=None):
    """One warped fo.integrate of scene `sc` (its volume, nodes and frame) with a caller-given obs_weight onto the old
    state (tsdf, weight, colour), each flat (V,) f32, left untouched. skin = (anchors, weights, valid) of the grid, or
    None for a source frame (every voxel at its world position). R / T / depth / color_im / intr default to the
    scene's. -> namespace: tsdf, weight, color (V,) f32, updated bool (V,), counts int (n_bricks,) updates per brick,
    n, pts (V,3) warped positions, px / py the voxels' pixels (0 where outside)."""
    world = fo.world_points(sc.origin, sc.dims, sc.vs)
    V = world.shape[0]
    if skin is None:
        pts, valid = world, np.ones(V, bool)
    else:
        a, w, valid = skin
        pts = fo.ed_warp(world, a, w, valid, sc.R if R is None else R, sc.T if T is None else T, sc.nodes)
    depth = sc.depth if depth is None else depth
    color_im = sc.color_im if color_im is None else color_im
    intr = sc.intr if intr is None else intr
    t, w_, c = (np.array(x, F32).reshape(-1).copy() for x in state)
    with np.errstate(all="ignore"):
        vis, _, px, py = fo.check_visibility(np.asarray(pts, F32).astype(F64), np.asarray(depth, F32), intr, TRUNC)
        n = fo.integrate(t, w_, c, pts, valid, depth, color_im, intr, obs_weight=obs_weight)
    updated = vis & valid
    assert n == int(updated.sum())
    b, _, nb = brick_index(sc.dims)
    counts = np.bincount(b[updated], minlength=nb)
    return SimpleNamespace(tsdf=t, weight=w_, color=c, updated=updated, counts=counts, n=n, pts=pts, px=px, py=py)


def w_new_is_one(weight_old, obs_weight):
    """The integrate's f32 new weight equals 1 (tsdf.py:366-376: f32(f64(w) + obs))."""
    return (np.asarray(weight_old, F32).astype(F64) + F64(obs_weight)).astype(F32) == F32(1)


def mixed_wave_groups(dims, updated, weight_old, obs_weight):
    """Number of wave-sized voxel groups (64 consecutive in-brick voxels of one brick) whose updated voxels hold both
    w_new == 1 and w_new != 1: where the wave-uniform reciprocal skip of sdf_color_update must not be taken."""
    b, l, _ = brick_index(dims)
    grp = b * 8 + l // 64
    one = w_new_is_one(weight_old, obs_weight)
    n = int(grp.max()) + 1
    has1 = np.bincount(grp[updated & one], minlength=n) > 0
    has0 = np.bincount(grp[updated & ~one], minlength=n) > 0
    return int((has1 & has0).sum())


def next_to(mask, px, py, sel):
    """Number of the selected voxels whose pixel (px, py) has a 4-neighbour pixel in `mask` (H,W)."""
    H, W = mask.shape
    m = np.zeros((H + 2, W + 2), bool)
    m[1:-1, 1:-1] = mask
    near = m[:-2, 1:-1] | m[2:, 1:-1] | m[1:-1, :-2] | m[1:-1, 2:]
    return int(near[py[sel], px[sel]].sum())


# ------------------------------------------------------------------------------------------------ scenes
def random_state(rng, V):
    """Random old volume: tsdf in [-1, 1], weight in {0, .5, .7, 1, 3}, packed 24-bit colours."""
    return (rng.uniform(-1, 1, V).astype(F32), rng.choice(WEIGHTS, V),
            rng.integers(0, 2 ** 24, V).astype(F32))


def hostile_depth(rng, W, H, base):
    """`base` (H,W) with 5 % zero pixels, a NaN patch, a +inf patch, a negative patch and a 16-pixel-wide column band
    of zeros (tile columns 4 and 5). -> depth f32 and the masks of the three patches."""
    d = np.array(base, F32)
    d[rng.random((H, W)) < 0.05] = 0.0
    nan, inf, neg = (np.zeros((H, W), bool) for _ in range(3))
    nan[18:23, 50:55] = True
    inf[28:34, 50:56] = True
    neg[38:44, 49:57] = True
    d[:, 32:48] = 0.0
    d[nan], d[inf], d[neg] = np.nan, np.inf, -0.8
    return d, nan, inf, neg


def frame(rng, depth):
    """(6,H,W) f32 frame built by hand (non-finite depth kept): random 8-bit rgb / 255, depth last; and its packed
    colour image."""
    H, W = depth.shape
    im = np.zeros((6, H, W), F32)
    im[:3] = (rng.integers(0, 256, (3, H, W)) / 255.0).astype(F32)
    im[5] = depth
    return im, fo.pack_color(im)


def _plane(W, H, z0=0.82, su=0.0010, sv=0.0008):
    v, u = np.indices((H, W))
    return (z0 + su * (u - 41) + sv * (v - 30)).astype(F32)


@functools.lru_cache(maxsize=None)
def scene_a(width=83, height=61, seed=20240611):
    """Ragged volume (37, 29, 44), mixed palette (a dense node lattice that overflows the 64-entry palette for
    x < -0.06, a sparse one for x > -0.03), large per-node rotations, hostile depth, random old state."""
    rng = np.random.default_rng(seed)
    sc = SimpleNamespace(origin=np.array([-0.19, -0.14, 0.62], F32), dims=(37, 29, 44), vs=0.01, cov=0.02,
                         intr=(70.0, 70.0, 41.3, 30.1), width=width, height=height)
    hi = sc.origin.astype(F64) + np.array(sc.dims) * sc.vs

    def lattice(x0, x1, h, jitter):
        ax = [np.arange(x0, x1, h), np.arange(sc.origin[1] - h, hi[1] + h, h), np.arange(sc.origin[2] - h, hi[2] + h, h)]
        g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
        return g + rng.uniform(-jitter, jitter, g.shape)
    nodes = np.concatenate([lattice(sc.origin[0] - 0.0165, -0.06, 0.0165, 0.004), lattice(-0.03, hi[0] + 0.05, 0.05, 0.01)])
    sc.nodes = nodes[rng.permutation(nodes.shape[0])].astype(F32)
    N = sc.nodes.shape[0]
    sc.R = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.15, (N, 3))).astype(F32)
    g = sc.nodes.astype(F64)
    smooth = 0.02 * np.stack([np.sin(7 * g[:, 1] + 1), np.cos(9 * g[:, 2]), np.sin(8 * g[:, 0] + 2)], 1)
    sc.T = (smooth + rng.normal(0, 0.003, (N, 3))).astype(F32)
    sc.depth, sc.nan, sc.inf, sc.neg = hostile_depth(rng, width, height, _plane(width, height))
    sc.im, sc.color_im = frame(rng, sc.depth)
    sc.state = random_state(rng, int(np.prod(sc.dims)))
    return sc


@functools.lru_cache(maxsize=None)
def skin_a():
    sc = scene_a()
    return dense_skin(sc.origin, sc.dims, sc.vs, sc.nodes, sc.cov)


def identity_transforms(sc, t):
    N = sc.nodes.shape[0]
    return np.tile(np.eye(3, dtype=F32), (N, 1, 1)), np.tile(np.asarray(t, F32), (N, 1))


@functools.lru_cache(maxsize=None)
def keep_rule_scenes():
    """Scene A's volume, nodes and old state under identity rotations and one common translation: the cull's keep
    rules. -> dict name -> namespace(R, T, intr, depth, im, color_im [, brick])."""
    sc = scene_a()
    rng = np.random.default_rng(77)
    out = {}

    def case(name, t, depth, intr=None, **kw):
        R, T = identity_transforms(sc, t)
        im, cim = frame(rng, depth)
        out[name] = SimpleNamespace(R=R, T=T, intr=sc.intr if intr is None else intr, depth=depth, im=im, color_im=cim,
                                    **kw)
    # 1: part of the warped volume at z < 1e-3 and behind the camera; the depth follows it
    d = np.where(sc.depth == 0, F32(0), sc.depth - F32(0.72)).astype(F32)
    case("behind", (0.0, 0.0, -0.80), d)
    # 2: a brick spans more than 64 tiles
    case("wide", (0.0, 0.0, 0.0), sc.depth, intr=(700.0, 700.0, 41.3, 30.1))
    # 3: nothing to fuse
    case("empty", (0.0, 0.0, 0.0), np.zeros_like(sc.depth))
    # 4: a constant depth 2e-4 inside / outside of (nearest warped voxel of a chosen brick) - trunc
    a, w, v = skin_a()
    t4 = (0.004, -0.003, 0.006)
    R, T = identity_transforms(sc, t4)
    pts = fo.ed_warp(fo.world_points(sc.origin, sc.dims, sc.vs), a, w, v, R, T, sc.nodes)
    b, _, _ = brick_index(sc.dims)
    pals = brick_palettes(a, v, sc.dims)
    clip = clipped_axes(sc.dims)
    # a whole, non-overflowing brick of the sparse side with every voxel skinned, in the middle of the image
    cand = [q for q in range(len(pals)) if 0 < len(pals[q]) <= PAL and not clip[q].any() and v[b == q].all()]
    ctr = np.array([pts[b == q].mean(0) for q in cand])
    brick = cand[int(np.argmin(np.abs(ctr[:, 0] - 0.03) + np.abs(ctr[:, 1]) + np.abs(ctr[:, 2] - 0.80)))]
    zmin = F64(pts[b == brick, 2].min())
    for name, off in (("inside", 2e-4), ("outside", -2e-4)):
        case(name, t4, np.full_like(sc.depth, F32(zmin - TRUNC + off)), brick=brick, zmin=zmin)
    return out


@functools.lru_cache(maxsize=None)
def scene_rows():
    """Scene A with a depth image that is zero except on the last row of every 8-row tile (and the first column of
    every 8-column tile): a tile maximum that misses its last row or column loses every pixel of the tile."""
    sc = scene_a()
    rng = np.random.default_rng(5)
    d = np.zeros_like(sc.depth)
    d[7::8, :] = _plane(sc.width, sc.height)[7::8, :]
    im, cim = frame(rng, d)
    return SimpleNamespace(depth=d, im=im, color_im=cim)


@functools.lru_cache(maxsize=None)
def scene_b(seed=99):
    """65534 nodes: about 7k reachable lattice nodes at the HIGHEST ids, decoys 100 m away below them."""
    rng = np.random.default_rng(seed)
    sc = SimpleNamespace(origin=np.array([-0.10, -0.08, 0.50], F32), dims=(20, 17, 12), vs=0.01, cov=0.012,
                         intr=(70.0, 70.0, 20.3, 15.1), width=41, height=31, n_nodes=65534)
    h = 0.011
    hi = sc.origin.astype(F64) + np.array(sc.dims) * sc.vs
    ax = [np.arange(sc.origin[j] - 2 * h, hi[j] + 2 * h, h) for j in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    g = (g + rng.uniform(-0.002, 0.002, g.shape))[rng.permutation(g.shape[0])]
    sc.first = sc.n_nodes - g.shape[0]
    decoys = np.array([100.0, 100.0, 100.0]) + rng.uniform(-1, 1, (sc.first, 3))
    sc.nodes = np.concatenate([decoys, g]).astype(F32)
    N = sc.n_nodes
    sc.R = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.05, (N, 3))).astype(F32)
    sc.T = rng.normal(0, 0.004, (N, 3)).astype(F32)
    v, u = np.indices((sc.height, sc.width))
    d = (0.56 + 0.001 * (u - 20)).astype(F32)
    d[rng.random(d.shape) < 0.05] = 0.0
    sc.depth = d
    sc.im, sc.color_im = frame(rng, d)
    sc.state = random_state(rng, int(np.prod(sc.dims)))
    return sc


@functools.lru_cache(maxsize=None)
def skin_b():
    sc = scene_b()
    return dense_skin_high_ids(sc.origin, sc.dims, sc.vs, sc.nodes, sc.cov, sc.first)


C_CUT2 = 10    # squared node-voxel distance (in voxels) that the cut-off of scene C sits on


@functools.lru_cache(maxsize=None)
def scene_c(seed=3):
    """Exact ties: voxel 1/64 and an origin of multiples of 1/64, so every coordinate and squared distance is exact in
    f32; nodes on every third voxel centre of a sub-block (shuffled ids, some duplicated); 4 sigma = the f32 distance
    sqrt(10)/64, which voxels one step off a node along one axis attain at their 4th anchor (among four equal ones)."""
    rng = np.random.default_rng(seed)
    sc = SimpleNamespace(origin=np.array([-12 / 64, -10 / 64, 40 / 64], F32), dims=(26, 21, 19), vs=1 / 64,
                         intr=(70.0, 70.0, 41.3, 30.1), width=83, height=61)
    ii, jj, kk = np.meshgrid(np.arange(3, 24, 3), np.arange(2, 20, 3), np.arange(2, 18, 3), indexing="ij")
    vox = np.stack([ii, jj, kk], -1).reshape(-1, 3)
    vox = np.concatenate([vox, vox[rng.choice(vox.shape[0], 24, replace=False)]])     # duplicates
    vox = vox[rng.permutation(vox.shape[0])]
    sc.node_vox = vox
    sc.nodes = (sc.origin.astype(F64) + vox / 64.0).astype(F32)
    cut = np.sqrt(F32(C_CUT2 / 4096.0))            # f32 sqrt of the exact f32 squared distance, as the skin forms it
    assert cut.dtype == F32
    sc.cov = float(cut) / 4.0                      # 4.0 * cov == cut exactly
    N = sc.nodes.shape[0]
    sc.R = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.1, (N, 3))).astype(F32)
    sc.T = rng.normal(0, 0.005, (N, 3)).astype(F32)
    sc.depth = _plane(sc.width, sc.height, z0=0.76)
    sc.depth[rng.random(sc.depth.shape) < 0.05] = 0.0
    sc.im, sc.color_im = frame(rng, sc.depth)
    sc.state = random_state(rng, int(np.prod(sc.dims)))
    return sc


def scene_c_ties(sc):
    """Integer squared distances (voxel units) of scene C -> (voxels with a tie straddling the K-th slot, voxels with
    a top-K distance exactly on the cut-off), bool (V,) each. Integer arithmetic: no rounding involved."""
    i, j, k = np.indices(sc.dims).reshape(3, -1)
    d2 = ((np.stack([i, j, k], 1)[:, None, :] - sc.node_vox[None]) ** 2).sum(-1)
    s = np.sort(d2, 1)
    straddle = s[:, 3] == s[:, 4]
    on_cut = ((s[:, :4] == C_CUT2).any(1)) & (s[:, 3] <= C_CUT2)
    return straddle, on_cut


@functools.lru_cache(maxsize=None)
def scene_c3():
    """Scene C's grid with a 3-node graph (K = 3): two coincident nodes and a third one 3 voxels away, a coverage that
    reaches a part of the volume only."""
    sc0 = scene_c()
    sc = SimpleNamespace(**vars(sc0))
    vox = np.array([[12, 10, 9], [12, 10, 9], [15, 10, 9]])
    sc.node_vox = vox
    sc.nodes = (sc.origin.astype(F64) + vox / 64.0).astype(F32)
    sc.cov = float(np.sqrt(F32(81 / 4096.0))) / 4.0     # 4 sigma = 9 voxels, attained along the axes
    rng = np.random.default_rng(8)
    sc.R = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.1, (3, 3))).astype(F32)
    sc.T = rng.normal(0, 0.005, (3, 3)).astype(F32)
    return sc


@functools.lru_cache(maxsize=None)
def scene_d():
    """Source frame on scene A's ragged volume, hostile depth and old state, with the principal point placed so that
    (X fx)/Z + cx of one voxel column (and cy of one voxel row) lands within 1e-9 of a half-integer: the f64 rint of
    the per-brick pixel tables sits on a tie."""
    a = scene_a()
    sc = SimpleNamespace(**vars(a))
    world = fo.world_points(a.origin, a.dims, a.vs).reshape(*a.dims, 3)
    xs, ys, zs = world[:, 0, 0, 0].astype(F64), world[0, :, 0, 1].astype(F64), world[0, 0, :, 2].astype(F64)

    def place(coord, f, target, size):
        """the f32 principal point c nearest to `target` for which some (coord f)/z + c lies within 1e-9 of a
        half-integer inside the image -> (c, number of such voxel columns)"""
        q = ((coord[:, None] * F64(F32(f))) / zs[None, :]).reshape(-1)
        zz = np.broadcast_to(zs[None, :], (coord.shape[0], zs.shape[0])).reshape(-1)
        cands = np.concatenate([(m + 0.5 - q).astype(F32) for m in range(size)])
        cands = np.unique(cands[np.abs(cands - target) < 8])
        for c in cands[np.argsort(np.abs(cands - target), kind="stable")]:
            s = q + F64(c)
            hit = (np.abs((s - np.floor(s)) - 0.5) < 1e-9) & (s > 0) & (s < size - 1) & (zz < 0.8)
            if hit.any():
                return float(c), int(hit.sum()), np.unique(np.floor(s[hit]).astype(int))
        return None, 0, None
    cx, sc.ties_u, pu = place(xs, 70.0, a.intr[2], a.width)
    cy, sc.ties_v, pv = place(ys, 70.0, a.intr[3], a.height)
    # the tied voxels are in front of the surface: give their pixels (either side of the tie) a plain depth
    plane = _plane(a.width, a.height)
    sc.depth = a.depth.copy()
    for d in (0, 1):
        sc.depth[:, pu + d] = plane[:, pu + d]
        sc.depth[pv + d, :] = plane[pv + d, :]
    sc.im, sc.color_im = frame(np.random.default_rng(11), sc.depth)
    sc.intr = (70.0, 70.0, cx, cy)
    return sc
