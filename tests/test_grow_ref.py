"""CPU: the numpy restatement of ofx_grow_nodes (tests/grow_ref.py) against closed-form answers, and the growth of the
graph over the sphere scene of tests/test_gpu_surface.py with the CPU restatements of the skin and the surface sampler.

The restatement is what the kernels are compared with bit for bit (tests/test_gpu_grow.py); here it is checked itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_ref as gr  # noqa: E402
import surface_ref as sr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
COV = 0.02


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _plane(nx=81, ny=41, h=0.005, z=0.5):
    x, y = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], 1).astype(F32)


def _left_nodes(x_max, y_max=0.2, z=0.5):
    x, y = np.meshgrid(np.arange(0, x_max + 1e-9, COV), np.arange(0, y_max + 1e-9, COV), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], 1).astype(F32)


def _graph(nodes, k_e=8):
    n = nodes.shape[0]
    return (np.tile(np.eye(3, dtype=F32), (n, 1, 1)), np.zeros((n, 3), F32), -np.ones((n, k_e), np.int32),
            np.zeros((n, k_e), F32))


def _uniform_skin(m):
    return np.tile(np.arange(4, dtype=np.int32), (m, 1)), np.full((m, 4), 0.25, F32)


@pytest.fixture(scope="module")
def plane():
    pts = _plane()
    nodes = _left_nodes(0.2)                      # the left half of the 0.4 m patch
    a, w = _uniform_skin(pts.shape[0])
    R, T, E, W = _graph(nodes)
    out = gr.grow_nodes(pts, a, w, np.ones(pts.shape[0], np.uint8), nodes, R, T, E, W, COV, 2 * COV, COV, 4096)
    return pts, nodes, out


def test_plane_selection_is_separated_and_maximal(plane):
    pts, nodes, out = plane
    n_cand, n_sel, capped = (int(v) for v in out["count"])
    assert capped == 0 and 0 < n_sel < n_cand
    new = out["nodes"][nodes.shape[0]:]
    assert new.shape[0] == n_sel and np.array_equal(new, pts[out["rows"]])
    assert np.all(np.diff(out["rows"]) > 0)                                   # ascending row order
    d = gr.sqrt_rn(gr.sqdist(new[:, None], new[None]))
    assert (d[~np.eye(n_sel, dtype=bool)] >= F32(COV)).all()                  # pairwise >= spacing
    assert (gr.dist_min(new, nodes) > F32(2 * COV)).all()                     # each > min_dist from every old node
    cand = gr.candidates(pts, _uniform_skin(pts.shape[0])[0], np.ones(pts.shape[0]), nodes, 2 * COV)
    assert int(cand.sum()) == n_cand
    assert (gr.dist_min(pts[cand], new) < F32(COV)).all()                     # maximal: the cap was not hit
    assert not cand[pts[:, 0] <= F32(0.2)].any()                              # nothing over the covered half


def test_cap_cuts_the_same_prefix(plane):
    pts, nodes, full = plane
    a, w = _uniform_skin(pts.shape[0])
    R, T, E, W = _graph(nodes)
    n_full = int(full["count"][1])
    for cap, flag in ((7, 1), (n_full, 0), (n_full - 1, 1)):
        out = gr.grow_nodes(pts, a, w, np.ones(pts.shape[0], np.uint8), nodes, R, T, E, W, COV, 2 * COV, COV, cap)
        assert list(out["count"]) == [int(full["count"][0]), cap, flag]
        assert np.array_equal(out["rows"], full["rows"][:cap])


def test_planted_rows():
    """An exact duplicate, a pair at exactly the spacing (both kept), a pair one ulp under it (the second dropped), a NaN
    point, an out-of-range anchor, invalid padding."""
    s = F32(COV)
    under = np.nextafter(s, F32(0))
    nodes = _left_nodes(0.06, 0.06)
    pts = np.array([[1, 0, 0.5], [1, 0, 0.5],                   # 0, 1: duplicate
                    [0, 1, 0.5], [s, 1, 0.5],                   # 2, 3: exactly the spacing apart
                    [0, 2, 0.5], [under, 2, 0.5],               # 4, 5: one ulp under
                    [np.nan, 3, 0.5], [1, 3, 0.5], [1, 4, 0.5],  # 6 NaN, 7 bad anchor, 8 negative anchor
                    [2, 4, 0.5], [0, 0, 0]], F32)               # 9 invalid row, 10 padding
    a, w = _uniform_skin(pts.shape[0])
    a[7, 2] = nodes.shape[0]
    a[8, 0] = -1
    valid = np.ones(pts.shape[0], np.uint8)
    valid[9:] = 0
    R, T, E, W = _graph(nodes)
    out = gr.grow_nodes(pts, a, w, valid, nodes, R, T, E, W, COV, 2 * COV, COV, 64)
    assert gr.sqrt_rn(gr.sqdist(pts[2], pts[3])) == s and gr.sqrt_rn(gr.sqdist(pts[4], pts[5])) < s
    assert list(out["rows"]) == [0, 2, 3, 4] and list(out["count"]) == [6, 4, 0]
    # nothing within min_dist of a node is a candidate; max_new = 0 and no rows are legal and empty
    near = gr.grow_nodes(nodes + F32(0.001), *_uniform_skin(nodes.shape[0]), np.ones(nodes.shape[0]), nodes, R, T, E, W,
                         COV, 2 * COV, COV, 64)
    assert list(near["count"]) == [0, 0, 0] and near["nodes"].shape == nodes.shape
    assert list(gr.grow_nodes(pts, a, w, valid, nodes, R, T, E, W, COV, 2 * COV, COV, 0)["count"]) == [0, 0, 0]
    assert list(gr.grow_nodes(pts[:0], a[:0], w[:0], valid[:0], nodes, R, T, E, W, COV, 2 * COV, COV, 8)["count"]) == [0, 0, 0]


@pytest.mark.parametrize("axis,angle", [((1, 2, 3), 0.3), ((0, 0, 1), 3.0), ((1, 0, 0), 3.1), ((0, 1, 0.1), 2.9),
                                        ((1, 1, 1), 0.0)])
def test_common_transform_is_reproduced(axis, angle):
    """Four anchors with one rotation and translation: that rotation within 2 ulp (every Shepperd branch), and exactly
    the translation the shared warp gives."""
    rng = np.random.default_rng(5)
    nodes = rng.uniform(0, 0.1, (6, 3)).astype(F32)
    Rc = _rot(axis, angle).astype(F32)
    R = np.tile(Rc, (6, 1, 1))
    T = np.tile(np.array([0.01, -0.02, 0.03], F32), (6, 1))
    pts = (rng.uniform(0.3, 0.31, (5, 3)) + 0.05 * np.arange(5)[:, None]).astype(F32)   # more than the spacing apart
    a = np.stack([rng.permutation(6)[:4] for _ in range(5)]).astype(np.int32)
    w = rng.uniform(0.1, 1, (5, 4)).astype(F32)
    w = (w / w.sum(1, keepdims=True)).astype(F32)
    _, _, E, W = _graph(nodes)
    out = gr.grow_nodes(pts, a, w, np.ones(5, np.uint8), nodes, R, T, E, W, COV, 2 * COV, COV, 8)
    assert int(out["count"][1]) == 5
    Rn, Tn = out["R"][6:], out["T"][6:]
    ulp = np.spacing(np.maximum(np.abs(Rc), F32(0.5)))             # of entries of magnitude up to 1
    assert (np.abs(Rn - Rc) <= 2 * ulp).all()
    assert np.array_equal(Tn, fo.ed_warp(pts, a, w, np.ones(5, bool), R, T, nodes) - pts)


def test_blended_rotation_is_orthonormal():
    rng = np.random.default_rng(6)
    R = np.stack([_rot(rng.normal(size=3), rng.uniform(0, 3.1)) for _ in range(40)]).astype(F32)
    a = np.stack([rng.permutation(40)[:4] for _ in range(200)]).astype(np.int32)
    w = rng.uniform(0, 1, (200, 4)).astype(F32)
    B = gr.blend_rotations(a, w, R).astype(np.float64)
    err = np.linalg.norm(np.einsum("nji,njk->nik", B, B) - np.eye(3), axis=(1, 2))
    assert err.max() < 1e-6 and (np.linalg.det(B) > 0).all()
    # q and -q are one rotation: negating an anchor's matrix representation changes nothing (sign alignment)
    q = gr.quat_of(R[:8])
    assert np.allclose(np.linalg.norm(q, axis=1), 1, atol=1e-15)


def test_edge_rows():
    """The 8 nearest other nodes in (d², id) order — ties by id — and weights that sum to one."""
    nodes = np.array([[0, 0, 0], [0.02, 0, 0], [-0.02, 0, 0], [0, 0.02, 0], [0, -0.02, 0], [0.04, 0, 0]], F32)
    E, W = gr.edge_rows(nodes, 0, 8, COV)
    assert list(E[0]) == [1, 2, 3, 4, 5, -1, -1, -1] and (W[0, 5:] == 0).all()
    assert abs(float(W[0, :5].sum()) - 1) < 1e-6 and W[0, 0] == W[0, 3] > W[0, 4] > 0
    e = np.exp(-np.array([1, 1, 1, 1, 4.0]) / 2)
    assert np.allclose(W[0, :5], e / e.sum(), rtol=1e-6)
    E2, _ = gr.edge_rows(nodes, 4, 3, COV)                     # rows of nodes 4 and 5 only
    assert E2.shape == (2, 3) and list(E2[1]) == [1, 0, 3]


# ---------------------------------------------------------------------------------------------- the sphere scene
def _sphere_round(phi, w, nodes, dims, origin, h):
    """Skin + sample on the CPU -> (model, histogram of codes)."""
    a, sw, _ = fo.skin(fo.world_points(origin, dims, h), nodes, COV)
    nb = int(np.prod([(d + 7) // 8 for d in dims]))
    m = sr.surface_points(phi, w, origin, h, np.arange(nb), a, sw, 1.0, 1024)
    return m, np.bincount(m["code"], minlength=8)


def test_sphere_scene_grows_to_a_fixed_point():
    """tests/test_gpu_surface.py's sphere, all weights 1, min_dist = 2·coverage, spacing = coverage: the first round
    leaves no skin-invalid surface voxel, and within 4 rounds no candidate is left."""
    import test_gpu_surface as tg
    phi, _, nodes = tg.scene_arrays()
    w = np.ones(tg.DIMS, F32)
    n_nodes, accepted, code7 = [], [], []
    for rnd in range(5):
        m, hist = _sphere_round(phi, w, nodes, tg.DIMS, tg.ORIGIN, tg.H_VOX)
        n_nodes.append(nodes.shape[0]); accepted.append(int(hist[0])); code7.append(int(hist[7]))
        R, T, E, W = _graph(nodes)
        out = gr.grow_nodes(m["points"], m["anchors"], m["weights"], m["valid"], nodes, R, T, E, W, COV, 2 * COV, COV, 256)
        if int(out["count"][1]) == 0:
            assert int(out["count"][0]) == 0
            break
        nodes = out["nodes"]
    print("nodes", n_nodes, "accepted", accepted, "code 7", code7)
    assert n_nodes[0] == 14 and code7[0] > 0 and accepted[0] + code7[0] == accepted[1]
    assert code7[1:] == [0] * (len(code7) - 1) and len(set(accepted[1:])) == 1
    assert len(n_nodes) <= 4 and n_nodes[1] > n_nodes[0]                     # the last entry is the round that added none
    acc_pts = m["points"][:accepted[-1]]
    assert (gr.dist_min(acc_pts, nodes) <= F32(2 * COV)).all()
    # what the restatements give with every brick listed in ascending order (another brick list visits the voxels in
    # another order, and the greedy selection follows the order)
    assert (n_nodes, accepted, code7) == ([14, 33, 44], [270, 419, 419], [149, 0, 0])


# ---------------------------------------------------------------------------------------------- the skin update's plan
def test_plan_closed_form():
    """A 24^3 volume at 0.01 m (27 bricks of 0.08 m), coverage 0.005 (cull radius just over 0.02 m): four nodes in the
    first brick list it alone; a new node in the middle of the centre brick touches only that brick, which stays unlisted
    (one node in reach, K = 4); four new nodes there append it; a new node by the first brick's far corner touches the
    eight bricks around that corner and re-skins the listed one."""
    dims, o, h, cov = (24, 24, 24), np.zeros(3, F32), 0.01, 0.005
    old = np.array([[0.03, 0.03, 0.03], [0.035, 0.03, 0.03], [0.03, 0.035, 0.03], [0.03, 0.03, 0.035]], F32)
    bl = gr.listed_bricks(dims, o, h, old, cov, 4)
    assert list(bl) == [0]
    mid = np.array([[0.115, 0.115, 0.115]], F32)
    re, ap = gr.skin_grow_plan(dims, o, h, np.concatenate([old, mid]), 4, cov, 4, bl)
    assert list(re) == [] and list(ap) == []
    four = mid + np.array([[0, 0, 0], [0.004, 0, 0], [0, 0.004, 0], [0, 0, 0.004]], F32)
    re, ap = gr.skin_grow_plan(dims, o, h, np.concatenate([old, four]), 4, cov, 4, bl)
    assert list(re) == [] and list(ap) == [13]
    corner = np.array([[0.075, 0.075, 0.075]], F32)
    re, ap = gr.skin_grow_plan(dims, o, h, np.concatenate([old, corner]), 4, cov, 4, bl)
    reach = gr.brick_reach(dims, o, h, corner, cov)[:, 0]
    assert list(re) == [0] and list(ap) == [] and list(np.nonzero(reach)[0]) == [0, 1, 3, 4, 9, 10, 12, 13]


def test_plan_on_the_sphere_scene():
    """The GPU skin test's scene (tests/test_gpu_grow.py, SKIN_COVERAGE): one round appends bricks and re-skins fewer than
    are listed; old list plus appended bricks is the list a full build makes on the grown graph. At the scene's own
    coverage 0.02 every listed brick is touched, which is why that test shrinks it."""
    import test_gpu_surface as tg
    phi, _, nodes = tg.scene_arrays()
    w = np.ones(tg.DIMS, F32)
    got = {}
    for cov in (0.02, 0.006):
        bl = gr.listed_bricks(tg.DIMS, tg.ORIGIN, tg.H_VOX, nodes, cov, 4)
        a, sw, _ = fo.skin(fo.world_points(tg.ORIGIN, tg.DIMS, tg.H_VOX), nodes, cov)
        m = sr.surface_points(phi, w, tg.ORIGIN, tg.H_VOX, bl, a, sw, 1.0, 1024)
        R, T, E, W = _graph(nodes)
        out = gr.grow_nodes(m["points"], m["anchors"], m["weights"], m["valid"], nodes, R, T, E, W, cov, 2 * cov, cov, 256)
        re, ap = gr.skin_grow_plan(tg.DIMS, tg.ORIGIN, tg.H_VOX, out["nodes"], nodes.shape[0], cov, 4, bl)
        full = gr.listed_bricks(tg.DIMS, tg.ORIGIN, tg.H_VOX, out["nodes"], cov, 4)
        assert sorted(list(bl) + list(ap)) == list(full) and set(re) <= set(bl)
        got[cov] = (len(bl), int(out["count"][1]), len(re), len(ap))
    assert got[0.02] == (16, 19, 16, 10) and got[0.006] == (4, 3, 3, 1)


# ---------------------------------------------------------------------------------------------- the plane, on the CPU
def test_six_rounds_cover_the_plane_on_the_cpu():
    """The GPU growth test's scene (tests/test_gpu_grow.py: a static fronto-parallel plane, dims (40, 24, 16) at 0.01 m,
    frame 0 valid over the left third, the nodes there, frames 1-6 whole) with the oracle's integrate and the restatements
    of the skin, the sampler and the growth: six rounds leave an accepted surface point in at least 95 % of the interior
    columns, and the fixed graph never passes its rim."""
    dims, h, cov, z0 = (40, 24, 16), 0.01, 0.02, 0.5837
    origin = np.array([-0.195, -0.115, 0.5], F32)
    intr, (H, W) = (200.0, 200.0, 80.0, 60.0), (120, 160)
    x_third = float(origin[0]) + dims[0] * h / 3
    full = np.full((H, W), z0, F32)
    left = full.copy()
    left[:, (np.arange(W) - intr[2]) * z0 / intr[0] >= x_third] = 0
    gx, gy = np.meshgrid(np.arange(float(origin[0]) + 0.01, x_third - 1e-9, cov),
                         np.arange(float(origin[1]) + 0.01, float(origin[1]) + dims[1] * h, cov), indexing="ij")
    nodes0 = np.stack([gx.reshape(-1), gy.reshape(-1), np.full(gx.size, z0)], 1).astype(F32)
    world = fo.world_points(origin, dims, h)
    V = world.shape[0]
    bricks = np.arange(int(np.prod([(d + 7) // 8 for d in dims])))
    interior = (dims[0] - 2) * (dims[1] - 2)

    def run(grow):
        nodes = nodes0
        tsdf, weight = np.ones(V, F32), np.zeros(V, F32)
        fo.integrate(tsdf, weight, None, world, np.ones(V, bool), left, None, intr, with_color=False)
        for _ in range(6):
            n = nodes.shape[0]
            R, T, E, Wt = _graph(nodes)
            a, sw, valid = fo.skin(world, nodes, cov)
            pts = fo.ed_warp(world, np.where(a < 0, 0, a), sw, valid, R, T, nodes)
            fo.integrate(tsdf, weight, None, pts, valid, full, None, intr, with_color=False)
            m = sr.surface_points(tsdf.reshape(dims), weight.reshape(dims), origin, h, bricks, a, sw, 1.0, 4096)
            if grow:
                nodes = gr.grow_nodes(m["points"], m["anchors"], m["weights"], m["valid"], nodes, R, T, E, Wt, cov, 2 * cov,
                                      cov, 256)["nodes"]
        a, sw, _ = fo.skin(world, nodes, cov)
        m = sr.surface_points(tsdf.reshape(dims), weight.reshape(dims), origin, h, bricks, a, sw, 1.0, 4096)
        e = int(m["count"][1])
        i, j, _ = np.unravel_index(m["voxel"][:e], dims)
        return len(set(zip(i.tolist(), j.tolist()))), float(m["points"][:e, 0].max()), nodes.shape[0]

    cols_fixed, x_fixed, _ = run(False)
    cols, _, n_nodes = run(True)
    print(f"plane on the CPU: {cols_fixed} of {interior} interior columns with the fixed graph, {cols} with growth, "
          f"{n_nodes} nodes")
    assert x_fixed <= float(nodes0[:, 0].max()) + 4 * cov and cols_fixed < 0.6 * interior
    assert cols >= 0.95 * interior
