"""CPU: the scenes of tests/skin_cache_ref.py reach the edges they are built for — asserted from the numpy restatement
alone, so that no comparison of tests/test_gpu_skin_cache_edges.py can pass vacuously — and the restatement helpers
give closed-form answers on hand-made inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cache_ref as sr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32, F64 = np.float32, np.float64
OBS = (1.0, 0.5, 0.3)


# ------------------------------------------------------------------------------------------------ helpers
def test_brick_index_and_palettes_closed_form():
    dims = (9, 8, 17)
    b, l, nb = sr.brick_index(dims)
    assert nb == 2 * 1 * 3
    b3, l3 = b.reshape(dims), l.reshape(dims)
    assert b3[0, 0, 0] == 0 and b3[0, 0, 8] == 1 and b3[0, 7, 16] == 2 and b3[8, 0, 0] == 3 and b3[8, 7, 16] == 5
    assert l3[1, 2, 3] == 64 + 16 + 3 and l3[8, 7, 16] == 7 * 8
    clip = sr.clipped_axes(dims)
    np.testing.assert_array_equal(clip[2], [False, False, True])
    np.testing.assert_array_equal(clip[3], [True, False, False])
    V = int(np.prod(dims))
    a = np.full((V, 4), -1, np.int32)
    valid = np.zeros(V, bool)
    a3 = a.reshape(*dims, 4)
    a3[0, 0, 0] = [7, 3, 7, 40000]
    a3[1, 1, 1] = [3, 9, 1, 2]
    a3[2, 2, 2] = [100, 101, 102, 103]       # not valid: must not enter the palette
    a3[8, 0, 16] = [5, 5, 5, 5]
    v3 = valid.reshape(dims)
    v3[0, 0, 0] = v3[1, 1, 1] = v3[8, 0, 16] = True
    pals = sr.brick_palettes(a, valid, dims)
    np.testing.assert_array_equal(pals[0], [1, 2, 3, 7, 9, 40000])
    np.testing.assert_array_equal(pals[5], [5])
    assert all(len(pals[q]) == 0 for q in (1, 2, 3, 4))


def test_dense_skin_is_chunked_fo_skin():
    rng = np.random.default_rng(0)
    origin, dims, vs = np.array([0.1, -0.2, 0.5], F32), (19, 17, 15), 0.01     # 4845 voxels: two chunks
    nodes = (origin + rng.uniform(0, 0.10, (300, 3))).astype(F32)
    a, w, v = sr.dense_skin(origin, dims, vs, nodes, 0.02)
    a1, w1, v1 = fo.skin(fo.world_points(origin, dims, vs), nodes, 0.02)
    np.testing.assert_array_equal(a, a1)
    np.testing.assert_array_equal(w, w1)
    np.testing.assert_array_equal(v, v1)
    assert v.any() and not v.all()
    # decoys ahead of the reachable nodes: ids shift, nothing else changes
    decoys = np.full((50, 3), 100.0, F32)
    a2, w2, v2 = sr.dense_skin_high_ids(origin, dims, vs, np.concatenate([decoys, nodes]), 0.02, 50)
    a3, w3, v3 = fo.skin(fo.world_points(origin, dims, vs), np.concatenate([decoys, nodes]), 0.02)
    np.testing.assert_array_equal(a2, a3)
    np.testing.assert_array_equal(w2, w3)
    np.testing.assert_array_equal(v2, v3)
    with pytest.raises(AssertionError):
        sr.dense_skin_high_ids(origin, dims, vs, nodes, 0.02, 50)


def test_two_frame_fusion_counts_and_weights():
    """A flat depth in front of half of a small volume, source frame: the voxels up to depth + trunc update, each by
    obs_weight, and the per-brick counts add up."""
    sc = sr.SimpleNamespace(origin=np.array([-0.05, -0.05, 0.5], F32), dims=(10, 10, 20), vs=0.01,
                            intr=(100.0, 100.0, 15.5, 15.5), depth=np.full((32, 32), 0.555, F32),
                            color_im=np.full((32, 32), 255.0, F32))
    V = 2000
    state = (np.zeros(V, F32), np.full(V, 0.5, F32), np.zeros(V, F32))
    r = sr.two_frame_fusion(sc, None, state, 0.3)
    z = fo.world_points(sc.origin, sc.dims, sc.vs)[:, 2].astype(F64)
    np.testing.assert_array_equal(r.updated, F64(F32(0.555)) - z >= -sr.TRUNC)
    assert r.n == 1000 and r.counts.tolist() == [512, 128, 0, 128, 32, 0, 128, 32, 0, 32, 8, 0]
    np.testing.assert_array_equal(r.weight[r.updated], F32(F64(F32(0.5)) + 0.3))
    np.testing.assert_array_equal(r.weight[~r.updated], F32(0.5))
    assert (state[1] == 0.5).all()          # the old state is left untouched
    assert sr.w_new_is_one(F32(0.7), 0.3) and sr.w_new_is_one(F32(0.5), 0.5) and not sr.w_new_is_one(F32(1), 0.3)


def test_next_to_and_mixed_groups():
    m = np.zeros((5, 6), bool)
    m[2, 3] = True
    px, py = np.array([3, 2, 4, 3, 0]), np.array([1, 2, 2, 2, 0])
    assert sr.next_to(m, px, py, np.ones(5, bool)) == 3          # the pixel itself does not count
    dims = (8, 8, 8)
    upd = np.zeros(512, bool)
    w = np.zeros(512, F32)
    upd[:4] = True
    w[:2] = 1.0                     # group 0: w_new 2, 2, 1, 1 -> mixed
    upd[64:66] = True               # group 1: all w_new == 1
    assert sr.mixed_wave_groups(dims, upd, w, 1.0) == 1


# ------------------------------------------------------------------------------------------------ scene A
@pytest.fixture(scope="module")
def A():
    sc = sr.scene_a()
    a, w, v = sr.skin_a()
    pals = sr.brick_palettes(a, v, sc.dims)
    fus = {o: sr.two_frame_fusion(sc, (a, w, v), sc.state, o) for o in OBS}
    return sr.SimpleNamespace(sc=sc, a=a, w=w, v=v, pn=np.array([len(p) for p in pals]), fus=fus)


def test_scene_a_conditions(A):
    sc, pn = A.sc, A.pn
    f = A.fus[1.0]
    assert 4000 < sc.nodes.shape[0] < 8192                  # (one bitmap word chunk per thread: scene B covers more)
    listed = pn > 0                                         # bricks with a skin-valid voxel: all of them are listed
    over = pn > sr.PAL
    small = listed & ~over
    print("bricks with skin:", int(listed.sum()), "overflowing:", int(over.sum()), "max distinct:", int(pn.max()),
          "overflowing updated:", int((over & (f.counts > 0)).sum()), "small updated:", int((small & (f.counts > 0)).sum()),
          "small idle:", int((small & (f.counts == 0)).sum()))
    assert over.sum() >= 20 and small.sum() >= 20
    assert pn.max() > 2 * sr.PAL
    assert (over & (f.counts > 0)).sum() >= 10
    idle = small & (f.counts == 0)
    assert idle.sum() >= 10
    # idle bricks farther than trunc + 2 cm behind every finite depth: the cull has to see those
    b, _, nb = sr.brick_index(sc.dims)
    zmin = np.full(nb, np.inf)
    np.minimum.at(zmin, b[A.v], f.pts[A.v, 2].astype(F64))
    far = idle & (zmin > sc.depth[np.isfinite(sc.depth)].max() + sr.TRUNC + 0.02)
    print("of them far behind the depth:", int(far.sum()))
    assert far.sum() >= 5
    clip = sr.clipped_axes(sc.dims)
    for ax in range(3):
        assert (clip[:, ax] & (f.counts > 0)).any()
        assert (clip[:, ax] & (f.counts > 0) & small).any()      # (the cull sees the non-overflowing ones only)
    for o in OBS:
        g = sr.mixed_wave_groups(sc.dims, A.fus[o].updated, sc.state[1], o)
        print("obs", o, "mixed wave groups:", g, "updates:", A.fus[o].n)
        assert g >= 10
        np.testing.assert_array_equal(A.fus[o].updated, f.updated)
    for name in ("nan", "inf", "neg"):
        n = sr.next_to(getattr(sc, name), f.px, f.py, f.updated)
        print("updated voxels next to a", name, "pixel:", n)
        assert n >= 1
    # the +inf patch updates (dist clamps to 1), the others never
    on = lambda m: int(m[f.py[f.updated], f.px[f.updated]].sum())
    assert on(sc.inf) > 0 and on(sc.nan) == 0 and on(sc.neg) == 0
    # large rotations: the |R| h term of the cull's box matters
    ang = np.arccos(np.clip((np.trace(sc.R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert np.median(ang) > 0.15 and ang.max() > 0.5


def test_scene_a_second_camera():
    sc = sr.scene_a(84, 62)
    assert sc.width % 4 == 0 and sc.width % 8 == 4 and sc.height % 8 == 6
    r = sr.two_frame_fusion(sc, sr.skin_a(), sc.state, 0.5)
    assert r.n > 5000
    np.testing.assert_array_equal(sc.nodes, sr.scene_a().nodes)          # the same graph: the skin is shared


def test_scene_rows_only_last_tile_rows(A):
    sc, rows = A.sc, sr.scene_rows()
    assert (rows.depth[np.arange(sc.height) % 8 != 7] == 0).all()
    r = sr.two_frame_fusion(sc, (A.a, A.w, A.v), sc.state, 1.0, depth=rows.depth, color_im=rows.color_im)
    small = (A.pn > 0) & (A.pn <= sr.PAL)
    assert (small & (r.counts > 0)).sum() >= 10
    assert (r.py[r.updated] < 56).sum() > 100        # rows of whole tiles (the last tile row is partial: 61 = 7 * 8 + 5)


def test_keep_rule_scenes(A):
    sc = A.sc
    K = sr.keep_rule_scenes()
    small = (A.pn > 0) & (A.pn <= sr.PAL)
    res = {n: sr.two_frame_fusion(sc, (A.a, A.w, A.v), sc.state, 1.0, R=k.R, T=k.T, depth=k.depth,
                                  color_im=k.color_im, intr=k.intr) for n, k in K.items()}
    b, _, nb = sr.brick_index(sc.dims)
    # 1: warped voxels at z < 1e-3, behind the camera, and in front of it with updates
    r = res["behind"]
    z = r.pts[A.v, 2]
    assert (z < 0).sum() > 1000 and ((z >= 0) & (z < 1e-3)).sum() + ((z > 0) & (z < 0.02)).sum() > 0
    zlo, zhi = np.full(nb, np.inf), np.full(nb, -np.inf)
    np.minimum.at(zlo, b[A.v], z)
    np.maximum.at(zhi, b[A.v], z)
    assert (small & (zlo < 1e-3) & (zhi > 0) & (r.counts > 0)).any()      # a kept brick that does update
    assert r.n > 500
    # 2: a non-overflowing brick whose updated voxels alone span more than 8 x 8 tiles
    r = res["wide"]
    spans = []
    for q in np.nonzero(small & (r.counts > 0))[0]:
        s = r.updated & (b == q)
        spans.append((r.px[s].max() // 8 - r.px[s].min() // 8 + 1) * (r.py[s].max() // 8 - r.py[s].min() // 8 + 1))
    assert max(spans) > 64
    # 3: nothing updates
    assert res["empty"].n == 0
    # 4: the chosen brick updates just inside and not just outside
    q = K["inside"].brick
    assert small[q] and K["outside"].brick == q
    assert 0 < res["inside"].counts[q] <= 64 and res["outside"].counts[q] == 0
    upd = res["inside"].updated & (b == q)
    assert (res["inside"].pts[upd, 2].astype(F64) - K["inside"].zmin < 2.5e-4).all()


# ------------------------------------------------------------------------------------------------ scenes B, C, D
def test_scene_b_conditions():
    sc = sr.scene_b()
    assert sc.nodes.shape[0] == 65534 and 5000 < 65534 - sc.first < 9000
    a, w, v = sr.skin_b()
    assert v.mean() > 0.9
    pals = sr.brick_palettes(a, v, sc.dims)
    ids = np.concatenate(pals)
    assert ids.min() >= 32768 and ids.max() == 65533             # uint16 ids that are negative as int16; the last id
    assert max(len(p) for p in pals) > sr.PAL and (a[v] >= sc.first).all()
    r = sr.two_frame_fusion(sc, (a, w, v), sc.state, 0.5)
    assert r.n > 1000 and 65533 in a[r.updated]


def test_scene_c_conditions():
    sc = sr.scene_c()
    straddle, on_cut = sr.scene_c_ties(sc)
    a, w, v = sr.dense_skin(sc.origin, sc.dims, sc.vs, sc.nodes, sc.cov)
    print("valid:", int(v.sum()), "tie across the K-th slot:", int((straddle & v).sum()), "on the cut-off:",
          int((on_cut & v).sum()))
    assert (straddle & v).sum() >= 100
    assert (on_cut & v).sum() >= 10            # valid although at the cut-off: the comparison is strict
    assert len(np.unique(sc.nodes, axis=0)) == sc.nodes.shape[0] - 24
    # the grid and the distances are exact: the f32 squared distances are the integers / 4096
    world = fo.world_points(sc.origin, sc.dims, sc.vs)
    i, j, k = np.indices(sc.dims).reshape(3, -1)
    np.testing.assert_array_equal(world.astype(F64), sc.origin.astype(F64) + np.stack([i, j, k], 1) / 64.0)
    assert F32(4.0 * sc.cov) == np.sqrt(F32(sr.C_CUT2 / 4096.0))
    # a voxel on the cut-off keeps its 4th anchor at exactly that distance
    d = np.sqrt(((world[on_cut & v][:, None, :] - sc.nodes[a[on_cut & v]]) ** 2).sum(-1, dtype=F32))
    assert (d.max(1) == F32(4.0 * sc.cov)).all()
    r = sr.two_frame_fusion(sc, (a, w, v), sc.state, 0.5)
    assert (r.updated & straddle).sum() >= 100 and (r.updated & on_cut).sum() >= 10
    # K = 3
    s3 = sr.scene_c3()
    a3, w3, v3 = sr.dense_skin(s3.origin, s3.dims, s3.vs, s3.nodes, s3.cov)
    assert a3.shape[1] == 3 and 100 < v3.sum() < v3.size
    np.testing.assert_array_equal(a3[v3][:, :2].min(1) >= 0, True)
    assert (a3[v3] == np.array([0, 1, 2])).all(1).sum() > 50        # the coincident pair in id order, nearest
    r3 = sr.two_frame_fusion(s3, (a3, w3, v3), s3.state, 0.5)
    assert r3.n > 100


def test_scene_d_conditions():
    sc = sr.scene_d()
    print("voxel columns on a pixel tie: u", sc.ties_u, "v", sc.ties_v, "principal point", sc.intr[2:])
    assert sc.ties_u >= 1 and sc.ties_v >= 1
    assert abs(sc.intr[2] - 41.3) < 8 and abs(sc.intr[3] - 30.1) < 8
    # an updated voxel sits on such a tie
    r = sr.two_frame_fusion(sc, None, sc.state, 1.0)
    p = r.pts[r.updated].astype(F64)
    su, sv = p[:, 0] * 70.0 / p[:, 2] + sc.intr[2], p[:, 1] * 70.0 / p[:, 2] + sc.intr[3]
    tie = lambda s: int((np.abs((s - np.floor(s)) - 0.5) < 1e-9).sum())
    print("updated voxels on a tie: u", tie(su), "v", tie(sv))
    assert tie(su) >= 1 and tie(sv) >= 1
    assert F32(sc.intr[2]) == sc.intr[2] and F32(sc.intr[3]) == sc.intr[3]
    for o in (0.3, 1.0):
        r = sr.two_frame_fusion(sc, None, sc.state, o)
        assert r.n > 5000
        assert sr.mixed_wave_groups(sc.dims, r.updated, sc.state[1], o) >= 10
