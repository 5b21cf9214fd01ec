"""GPU: the skin cache (k_brick_cull / k_skin_volume / k_skin_palette), the warped integrate kernels that consume it
(k_integrate_pal4, k_integrate<1,1,0>, k_integrate<1,0,0>) with their per-frame brick cull (k_tile_max / k_brick_cull),
and the source-frame kernel (k_integrate_src), at their edges and bit for bit against the numpy restatement of tests/
skin_cache_ref.py: a ragged volume, palettes that overflow naturally next to ones that do not, large per-node
rotations, NaN / inf / negative / zero depth, obs_weight != 1 on a random old state, 65534 nodes with ids >= 32768,
exact k-NN ties and a distance exactly on the cut-off, pixel ties of the projection tables, and the keep rules of the
cull. tests/test_skin_cache_ref.py asserts on the CPU that the scenes reach those edges."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cache_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
eq = np.testing.assert_array_equal
OBS = (1.0, 0.5, 0.3)


class _Opt:
    source_frame = 0
    skip_rate = 1


def _volume(sc, cuda):
    from occlusionfusion_amd import TSDFVolume
    return TSDFVolume.from_grid(sc.origin, sc.vs, sc.dims, sc.intr, _Opt(), device=cuda)


def _warpfield(sc, vol):
    from occlusionfusion_amd import EDGraph, WarpField
    N = sc.nodes.shape[0]
    wf = WarpField(EDGraph(sc.nodes, -np.ones((N, 8), np.int32), node_coverage=sc.cov), vol)
    wf.frame_id = 1
    wf.set_node_transforms(sc.R, sc.T)
    return wf


def _load(vol, state):
    D = tuple(int(d) for d in vol._vol_dim)
    t, w, c = state
    buf = io.BytesIO()
    np.save(buf, np.stack([t.reshape(D), c.reshape(D), w.reshape(D)]))
    buf.seek(0)
    vol.load_volume(buf)


def _fuse(vol, state, im, obs, intr=None, frame=1):
    """Load the old state, integrate `im` as frame `frame` (0: the source frame) -> (tsdf, weight, colour) flat and the
    raw per-workgroup update counts."""
    _load(vol, state)
    if intr is not None:
        vol.cam_intr[0, 0], vol.cam_intr[1, 1], vol.cam_intr[0, 2], vol.cam_intr[1, 2] = intr
    vol.frame_id = frame - 1
    vol.update(im, frame)
    vol.n_updated.fill_(-1)
    vol.integrate_device(obs, count_updates=True)
    torch.cuda.synchronize()
    t, c, w = (x.reshape(-1) for x in vol.get_volume())
    return t, w, c, vol.n_updated.cpu().numpy()


def _brick_counts(vol, cache, raw):
    nb = vol.n_bricks
    out = np.zeros(nb, np.int64)
    out[cache.brick_list[:cache.n_list].cpu().numpy()] = raw[:cache.n_list]
    return out


def _check(got, ref, counts=None):
    t, w, c = got[:3]
    eq(w, ref.weight)
    eq(t, ref.tsdf)
    eq(c, ref.color)
    if counts is not None:
        eq(counts, ref.counts)


def _cache_arrays(c):
    P = sr.PAL
    n = c.n_list
    return sr.SimpleNamespace(
        blist=c.brick_list[:n].cpu().numpy().astype(np.int64),
        an=c.anchors.view(torch.uint16).cpu().numpy().astype(np.int64).reshape(-1, 512, 4)[:n, :, :c.k],
        loc=c.local.cpu().numpy().astype(np.int64).reshape(-1, 512, 4)[:n, :, :c.k],
        pid=c.pal_ids.view(torch.uint16).cpu().numpy().astype(np.int64).reshape(-1, P)[:n],
        pn=c.pal_n.cpu().numpy()[:n])


def _check_skin_dense(wf, sc, skin, blist):
    """skin_tsdf() against the restatement: every voxel of a listed brick (valid or not), and -1 / 0 / invalid in the
    unlisted ones, which hold no skin-valid voxel."""
    a_ref, w_ref, v_ref = skin
    a, w, v = wf.skin_tsdf()
    b, _, nb = sr.brick_index(sc.dims)
    listed = np.zeros(nb, bool)
    listed[blist] = True
    m = listed[b]
    eq(v, v_ref)
    eq(a[m], a_ref[m])
    eq(w[m], w_ref[m])
    assert (a[~m] == -1).all() and (w[~m] == 0).all() and not v[~m].any()
    assert a.min() >= -1            # ids are unsigned: nothing sign-extended


def _check_palette(ca, skin, dims):
    a_ref, _, v_ref = skin
    pals = sr.brick_palettes(a_ref, v_ref, dims)
    b, l, nb = sr.brick_index(dims)
    assert (np.diff(ca.blist) > 0).all()                                  # ascending
    has = np.array([len(p) > 0 for p in pals])
    assert has[ca.blist].sum() == has.sum()                               # every brick with a skin-valid voxel is listed
    n_over = 0
    for s, q in enumerate(ca.blist):
        pal = pals[q]
        assert ca.pn[s] == len(pal), (s, q)                               # the distinct count, beyond the palette too
        m = min(len(pal), sr.PAL)
        eq(ca.pid[s, :m], pal[:m])
        sel = b == q
        valid = np.zeros(512, bool)
        valid[l[sel]] = v_ref[sel]
        anch = np.full((512, a_ref.shape[1]), -1, np.int64)
        anch[l[sel]] = a_ref[sel]
        eq(ca.an[s][valid], anch[valid])
        inside = np.zeros(512, bool)
        inside[l[sel]] = True
        assert (ca.an[s][~inside] == 0xFFFF).all()                        # lanes past the volume's end: no voxels
        assert (ca.loc[s][~valid] == 0xFF).all()
        if len(pal) <= sr.PAL:
            eq(ca.pid[s][ca.loc[s][valid]], anch[valid])
        else:
            n_over += 1
            rank = np.searchsorted(pal, anch[valid])
            eq(ca.loc[s][valid], np.where(rank < sr.PAL, rank, 0xFF))     # ranks past the palette: no local id
    return n_over


# ------------------------------------------------------------------------------------------------ scene A
@pytest.fixture(scope="module")
def A(cuda):
    sc = sr.scene_a()
    vol = _volume(sc, cuda)
    wf = _warpfield(sc, vol)
    cache = wf.skin_tsdf_cache()
    return sr.SimpleNamespace(sc=sc, vol=vol, wf=wf, cache=cache, ca=_cache_arrays(cache), skin=sr.skin_a(), ref={})


def _ref_a(A, obs):
    if obs not in A.ref:
        A.ref[obs] = sr.two_frame_fusion(A.sc, A.skin, A.sc.state, obs)
    return A.ref[obs]


def test_a_skin_equals_dense_skin(A):
    _check_skin_dense(A.wf, A.sc, A.skin, A.ca.blist)


def test_a_brick_list_and_palette(A):
    n_over = _check_palette(A.ca, A.skin, A.sc.dims)
    assert n_over >= 20 and A.ca.pn.max() > 2 * sr.PAL


@pytest.mark.parametrize("config", ["cull", "nocull", "global", "generic"])
def test_a_warped_integrate(A, config, monkeypatch):
    """k_integrate_pal4 with and without the brick cull, the global-anchor kernel (use_palette = False) and the generic
    palette kernel (OFX_INT_GENERIC=1), each at obs_weight 1, 0.5 and 0.3 on the random old state."""
    vol = A.vol
    if config == "generic":
        monkeypatch.setenv("OFX_INT_GENERIC", "1")
    vol.brick_cull = config == "cull"
    vol.use_palette = config != "global"
    try:
        for obs in OBS:
            ref = _ref_a(A, obs)
            got = _fuse(vol, A.sc.state, A.sc.im, obs, A.sc.intr)
            _check(got, ref, _brick_counts(vol, A.cache, got[3]))
            if config == "cull":
                active = vol._cull[1][:A.cache.n_list].cpu().numpy()
                idle = ref.counts[A.ca.blist] == 0
                assert idle[active == 0].all()           # every skipped brick updates nothing
                assert (active == 0).sum() >= 1
                assert active[A.ca.pn > sr.PAL].all()     # an overflowing palette bounds nothing: kept
    finally:
        vol.brick_cull, vol.use_palette = True, True


def _twin(A, k, ref, obs=1.0):
    """Cull on, cull off and the oracle on a variant frame / transform set of scene A -> the cull's flags."""
    vol = A.vol
    A.wf.set_node_transforms(getattr(k, "R", A.sc.R), getattr(k, "T", A.sc.T))
    try:
        for cull in (False, True):
            vol.brick_cull = cull
            got = _fuse(vol, A.sc.state, k.im, obs, getattr(k, "intr", A.sc.intr))
            _check(got, ref, _brick_counts(vol, A.cache, got[3]))
        active = vol._cull[1][:A.cache.n_list].cpu().numpy()
        assert (ref.counts[A.ca.blist] == 0)[active == 0].all()
        return active
    finally:
        vol.brick_cull = True
        A.wf.set_node_transforms(A.sc.R, A.sc.T)
        vol.cam_intr[0, 0], vol.cam_intr[1, 1], vol.cam_intr[0, 2], vol.cam_intr[1, 2] = A.sc.intr


def test_a_second_camera_vector_tiles(A):
    """84 x 62: W % 4 == 0, so k_tile_max takes its 16-byte path, with a partial last tile column and row."""
    s2 = sr.scene_a(84, 62)
    ref = sr.two_frame_fusion(s2, A.skin, A.sc.state, 0.5)
    active = _twin(A, s2, ref, 0.5)
    assert (active == 0).sum() >= 1


def test_a_depth_on_last_tile_rows_only(A):
    """Depth only on the 8th row of every tile: a tile maximum that stops a row short sees nothing."""
    rows = sr.scene_rows()
    ref = sr.two_frame_fusion(A.sc, A.skin, A.sc.state, 1.0, depth=rows.depth, color_im=rows.color_im)
    _twin(A, rows, ref)


@pytest.mark.parametrize("case", ["behind", "wide", "empty", "inside", "outside"])
def test_a_cull_keep_rules(A, case):
    k = sr.keep_rule_scenes()[case]
    ref = sr.two_frame_fusion(A.sc, A.skin, A.sc.state, 1.0, R=k.R, T=k.T, depth=k.depth, color_im=k.color_im,
                              intr=k.intr)
    active = _twin(A, k, ref)
    small = A.ca.pn <= sr.PAL
    if case == "empty":
        assert ref.n == 0 and not active[small].any() and active[~small].all()
    if case in ("inside", "outside"):
        s = int(np.nonzero(A.ca.blist == k.brick)[0][0])
        assert small[s]
        if case == "inside":
            assert active[s] == 1 and ref.counts[k.brick] > 0
        assert (active[small] == 0).sum() >= 1


# ------------------------------------------------------------------------------------------------ scene B
OFX_ERR_RANGE = -3


@pytest.fixture(scope="module")
def B(cuda):
    sc = sr.scene_b()
    vol = _volume(sc, cuda)
    wf = _warpfield(sc, vol)
    cache = wf.skin_tsdf_cache()
    return sr.SimpleNamespace(sc=sc, vol=vol, wf=wf, cache=cache, ca=_cache_arrays(cache), skin=sr.skin_b())


def test_b_high_ids_cache_and_palette(B):
    assert B.wf.num_nodes == 65534
    _check_skin_dense(B.wf, B.sc, B.skin, B.ca.blist)
    assert _check_palette(B.ca, B.skin, B.sc.dims) >= 1
    ids = np.concatenate([B.ca.pid[s, :min(n, sr.PAL)] for s, n in enumerate(B.ca.pn)])
    assert ids.min() >= 32768
    a = B.wf.skin_tsdf()[0]
    assert a.max() == 65533 and (a[a >= 0] >= B.sc.first).all()


def test_b_high_ids_integrate(B):
    ref = sr.two_frame_fusion(B.sc, B.skin, B.sc.state, 0.5)
    for cull in (True, False):
        B.vol.brick_cull = cull
        got = _fuse(B.vol, B.sc.state, B.sc.im, 0.5)
        _check(got, ref, _brick_counts(B.vol, B.cache, got[3]))
    B.vol.brick_cull = True


def test_b_surface_points_report_unsigned_ids(B):
    """A plane through the volume, every voxel observed: the sampler's anchors are the cache's, as unsigned ids."""
    sc = B.sc
    z = sr.fo.world_points(sc.origin, sc.dims, sc.vs)[:, 2]
    V = z.shape[0]
    _load(B.vol, (np.clip((0.561 - z) / 0.04, -1, 1).astype(F32), np.ones(V, F32), np.zeros(V, F32)))
    m = B.wf.surface_points(4096)
    assert m["emitted"] > 100
    valid = m["valid"].cpu().numpy().astype(bool)
    vox = m["voxel"].cpu().numpy()[valid]
    an = m["anchors"].cpu().numpy()[valid]
    assert valid.sum() > 100 and an.min() >= 32768
    eq(an, B.skin[0][vox])
    eq(m["weights"].cpu().numpy()[valid], B.skin[1][vox])


def test_b_one_node_more_is_refused(B, cuda):
    """65535 nodes: refused with OFX_ERR_RANGE before any launch, the outputs untouched."""
    from occlusionfusion_amd import _lib
    from occlusionfusion_amd._lib import byref, ptr, stream_ptr
    vol = B.vol
    nodes = torch.cat([B.wf.nodes_t, B.wf.nodes_t[:1]]).contiguous()
    assert nodes.shape[0] == 65535
    blist = torch.full((vol.n_bricks,), -7, dtype=torch.int32, device=cuda)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    st = _lib.lib.ofx_skin_volume_bricks(byref(vol.desc), ptr(nodes), 65535, B.sc.cov, 4, ptr(blist), ptr(cnt),
                                         stream_ptr())
    assert st == OFX_ERR_RANGE and b"65534" in _lib.lib.ofx_last_error()
    n = B.cache.n_list
    anchors = torch.full((n * 2048,), -7, dtype=torch.int16, device=cuda)
    weights = torch.full((n * 2048,), -7.0, dtype=torch.float32, device=cuda)
    st = _lib.lib.ofx_skin_volume(byref(vol.desc), ptr(nodes), 65535, B.sc.cov, 4, ptr(B.cache.brick_list), n,
                                  ptr(anchors), ptr(weights), stream_ptr())
    assert st == OFX_ERR_RANGE
    torch.cuda.synchronize()
    assert (blist == -7).all() and int(cnt.item()) == -7 and (anchors == -7).all() and (weights == -7).all()
    with pytest.raises(_lib.OfxError):
        _lib.call("ofx_skin_volume_bricks", byref(vol.desc), ptr(nodes), 65535, B.sc.cov, 4, ptr(blist), ptr(cnt),
                  stream_ptr())
    # the cache and the volume's warp field still serve
    eq(_cache_arrays(B.wf.skin_tsdf_cache()).pn, B.ca.pn)


# ------------------------------------------------------------------------------------------------ scene C
def test_c_exact_ties(cuda):
    sc = sr.scene_c()
    skin = sr.dense_skin(sc.origin, sc.dims, sc.vs, sc.nodes, sc.cov)
    vol = _volume(sc, cuda)
    wf = _warpfield(sc, vol)
    cache = wf.skin_tsdf_cache()
    ca = _cache_arrays(cache)
    _check_skin_dense(wf, sc, skin, ca.blist)
    _check_palette(ca, skin, sc.dims)
    ref = sr.two_frame_fusion(sc, skin, sc.state, 0.5)
    got = _fuse(vol, sc.state, sc.im, 0.5)
    _check(got, ref, _brick_counts(vol, cache, got[3]))


@pytest.mark.parametrize("palette", [True, False])
def test_c_three_nodes(cuda, palette):
    """K = 3 (a 3-node graph, two of them coincident): the generic palette kernel k_integrate<1,1,0> and the
    global-anchor one."""
    sc = sr.scene_c3()
    skin = sr.dense_skin(sc.origin, sc.dims, sc.vs, sc.nodes, sc.cov)
    assert skin[0].shape[1] == 3
    vol = _volume(sc, cuda)
    wf = _warpfield(sc, vol)
    cache = wf.skin_tsdf_cache()
    assert cache.k == 3
    ca = _cache_arrays(cache)
    _check_skin_dense(wf, sc, skin, ca.blist)
    _check_palette(ca, skin, sc.dims)
    vol.use_palette = palette
    ref = sr.two_frame_fusion(sc, skin, sc.state, 0.5)
    got = _fuse(vol, sc.state, sc.im, 0.5)
    _check(got, ref, _brick_counts(vol, cache, got[3]))


# ------------------------------------------------------------------------------------------------ scene D
@pytest.mark.parametrize("kernel", ["src", "generic"])
def test_d_source_frame(cuda, kernel, monkeypatch):
    """k_integrate_src (per-brick pixel tables, f64 rint on a tie) and the generic source-frame kernel on the ragged
    volume, hostile depth, random old state."""
    if kernel == "generic":
        monkeypatch.setenv("OFX_INT_GENERIC", "1")
    sc = sr.scene_d()
    vol = _volume(sc, cuda)
    for obs in (0.3, 1.0):
        ref = sr.two_frame_fusion(sc, None, sc.state, obs)
        got = _fuse(vol, sc.state, sc.im, obs, frame=0)
        _check(got, ref, got[3][:vol.n_bricks])
        assert int(got[3][:vol.n_bricks].sum()) == ref.n
