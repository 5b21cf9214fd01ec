"""GPU: the observation-weight map (k_observation_weights) and the weighted integrate (the WT instantiations of
k_integrate_pal4 with and without the brick cull, k_integrate<1,1,0> and <1,0,0>, k_integrate_src, the generic source
kernel and k_integrate_points) bit for bit against the numpy restatement of tests/weighted_ref.py, on the scenes of tests/
skin_cache_ref.py: a ragged volume, overflowing palettes, hostile depth, a random old state, and a weight image of
non-dyadic weights with zeros, negatives, NaN, +inf and subnormals. Then the degenerate form (a weight image of ones and
no cap is the unweighted call, byte for byte) and the pipeline's fusion_weights keyword."""
import io
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fusion_oracle as fo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cache_ref as sr  # noqa: E402
import weighted_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
eq = np.testing.assert_array_equal
INF = float("inf")
# (w_max, obs_weight, with colour): both caps, both scalar weights, with and without colour
CASES = [(INF, 1.0, True), (2.5, 0.3, True), (2.5, 1.0, False), (INF, 0.3, False)]


class _Opt:
    source_frame = 0
    skip_rate = 1


def _volume(sc, cuda):
    from occlusionfusion_amd import TSDFVolume
    return TSDFVolume.from_grid(sc.origin, sc.vs, sc.dims, sc.intr, _Opt(), device=cuda)


def _load(vol, state):
    D = tuple(int(d) for d in vol._vol_dim)
    t, w, c = state
    buf = io.BytesIO()
    np.save(buf, np.stack([t.reshape(D), c.reshape(D), w.reshape(D)]))
    buf.seek(0)
    vol.load_volume(buf)


def _fuse(vol, state, im, obs, frame=1, **kw):
    """Load the old state, integrate `im` as frame `frame` (0: the source frame) with integrate_device(**kw) ->
    (tsdf, weight, colour) flat and the raw per-workgroup update counts."""
    _load(vol, state)
    vol.frame_id = frame - 1
    vol.update(im, frame)
    vol.n_updated.fill_(-1)
    vol.integrate_device(obs, count_updates=True, **kw)
    torch.cuda.synchronize()
    t, c, w = (x.reshape(-1) for x in vol.get_volume())
    return t, w, c, vol.n_updated.cpu().numpy()


def _check(got, ref, counts=None):
    t, w, c = got[:3]
    eq(w, ref.weight)
    eq(t, ref.tsdf)
    eq(c, ref.color)
    if counts is not None:
        eq(counts, ref.counts)


# ------------------------------------------------------------------------------------------------ the weight map
def _maps_from_depth(cuda, depth, intr, radius):
    from occlusionfusion_amd.image_proc import prepare_depth_device
    out = prepare_depth_device(torch.from_numpy(depth).to(cuda), *intr, radius=radius, edge_max=0.03)
    return out["point_image"], out["normals"]


@pytest.mark.parametrize("source", ["hostile", "hostile_filtered", "tilted"])
def test_weight_map_bit_for_bit(cuda, source):
    """Scene A's 83 x 61 camera (a width that is no multiple of the wave): the vertex and normal maps ofx_prepare_depth
    makes of the hostile depth (holes, NaN, +inf, negative, a step beyond edge_max), raw and filtered, and a plane tilted
    by 60 degrees in closed form; every cos_power, z_ref = 0 and two values > 0, non-default floor and edge weight."""
    sc = sr.scene_a()
    if source == "tilted":
        p, n = (torch.from_numpy(x).to(cuda) for x in wr.plane_maps(sc.height, sc.width, sc.intr, 0.9, 60.0))
    else:
        d = sc.depth.copy()
        d[:, 64:] += F32(0.1)                         # a depth step of 10 cm: beyond edge_max
        p, n = _maps_from_depth(cuda, d, sc.intr, 0 if source == "hostile" else 3)
    pn, nn = p.cpu().numpy(), n.cpu().numpy()
    has_n = (nn != 0).any(0)
    assert has_n.sum() > 500 and ((pn[2] > 0) & ~has_n).sum() > 100
    if source != "tilted":
        assert (~(pn[2] > 0)).sum() > 500
    from occlusionfusion_amd import TSDFVolume
    vol = TSDFVolume.__new__(TSDFVolume)
    vol.device = cuda
    seen = set()
    for cos_power in (0, 1, 2):
        for z_ref, w_floor, edge_weight in ((0.0, 0.05, 0.0), (0.5, 0.05, 0.0), (0.7, 0.3, 0.125)):
            got = vol.observation_weights(p, n, cos_power=cos_power, z_ref=z_ref, w_floor=w_floor,
                                          edge_weight=edge_weight).cpu().numpy()
            ref = wr.observation_weights(pn, nn, cos_power, z_ref, w_floor, edge_weight)
            assert got.dtype == F32 and got.shape == (sc.height, sc.width)
            eq(got.view(np.uint32), ref.view(np.uint32))
            seen.add(got.tobytes())
    assert len(seen) == 9      # every parameter acts (the surfaces lie beyond both z_ref values)


# ------------------------------------------------------------------------------------------------ scene A
@pytest.fixture(scope="module")
def A(cuda):
    from occlusionfusion_amd import EDGraph, WarpField
    sc = sr.scene_a()
    vol = _volume(sc, cuda)
    N = sc.nodes.shape[0]
    wf = WarpField(EDGraph(sc.nodes, -np.ones((N, 8), np.int32), node_coverage=sc.cov), vol)
    wf.frame_id = 1
    wf.set_node_transforms(sc.R, sc.T)
    cache = wf.skin_tsdf_cache()
    wim = wr.weight_image(np.random.default_rng(20250101), sc.height, sc.width)
    return sr.SimpleNamespace(sc=sc, vol=vol, wf=wf, cache=cache, skin=sr.skin_a(), wim=wim,
                              wim_t=torch.from_numpy(wim).to(cuda), ref={},
                              blist=cache.brick_list[:cache.n_list].cpu().numpy().astype(np.int64),
                              pn=cache.pal_n.cpu().numpy()[:cache.n_list])


def _ref_a(A, case):
    if case not in A.ref:
        w_max, obs, col = case
        A.ref[case] = wr.two_frame_weighted(A.sc, A.skin, A.sc.state, obs, A.wim, w_max, with_color=col)
    return A.ref[case]


def _brick_counts(A, raw):
    out = np.zeros(A.vol.n_bricks, np.int64)
    out[A.blist] = raw[:A.cache.n_list]
    return out


@pytest.mark.parametrize("config", ["cull", "nocull", "global", "generic"])
def test_a_weighted_warped_integrate(A, config, monkeypatch):
    """The four configurations of test_a_warped_integrate with the weight image: k_integrate_pal4's weighted form with
    and without the brick cull (>= 20 overflowing palettes), the global-anchor kernel and the generic palette kernel."""
    vol = A.vol
    if config == "generic":
        monkeypatch.setenv("OFX_INT_GENERIC", "1")
    vol.brick_cull = config == "cull"
    vol.use_palette = config != "global"
    assert (A.pn > sr.PAL).sum() >= 20
    try:
        for case in CASES:
            w_max, obs, col = case
            ref = _ref_a(A, case)
            assert ref.n > 1000
            vol.with_color = col
            got = _fuse(vol, A.sc.state, A.sc.im, obs, weight_image=A.wim_t, max_weight=None if w_max == INF else w_max)
            _check(got, ref, _brick_counts(A, got[3]))
            if config == "cull":
                active = vol._cull[1][:A.cache.n_list].cpu().numpy()
                idle = ref.counts[A.blist] == 0
                assert idle[active == 0].all()           # every skipped brick updates nothing in the restatement
                assert (active == 0).sum() >= 1
    finally:
        vol.brick_cull, vol.use_palette, vol.with_color = True, True, True


def test_a_integrate_timing_hook(A, cuda, points_case, monkeypatch):
    """TSDFVolume.integrate_timing (ofx_integrate_timing: what bench.py divides its kernel time by). Armed, every warped
    integrate_device — with the cull (three kernels, one event pair), without it, with global anchors and through the
    generic palette kernel, plain and with the weight image — records exactly one launch with a finite time > 0; the
    source frame and integrate_points record none; disarmed, a warped integrate records none."""
    from occlusionfusion_amd import TSDFVolume
    vol, sc, timing = A.vol, A.sc, TSDFVolume.integrate_timing
    assert (A.pn > sr.PAL).sum() >= 20
    timing(True)                                         # arm, and drop whatever was recorded before
    try:
        for config in ("cull", "nocull", "global", "generic"):
            with monkeypatch.context() as m:
                if config == "generic":
                    m.setenv("OFX_INT_GENERIC", "1")
                vol.brick_cull, vol.use_palette = config == "cull", config != "global"
                for kw in ({}, dict(weight_image=A.wim_t)):
                    _fuse(vol, sc.state, sc.im, 1.0, **kw)
                    ms, n = timing(True)
                    print(f"integrate_timing {config} {'weighted' if kw else 'plain'}: {ms:.4f} ms, {n} launch(es)")
                    assert n == 1 and 0 < ms < INF, (config, sorted(kw), ms, n)
        d = sr.scene_d()
        for kw in ({}, dict(weight_image=torch.ones((d.height, d.width), dtype=torch.float32, device=cuda))):
            _fuse(_volume(d, cuda), d.state, d.im, 1.0, frame=0, **kw)
            assert timing(True) == (0.0, 0)
        c = points_case
        for kw in ({}, dict(weight_image=torch.from_numpy(c.wim).to(cuda))):
            _points_volume(c, cuda).integrate_points(c.pts, c.vox, c.valid, **kw)
            torch.cuda.synchronize()
            assert timing(True) == (0.0, 0)
        assert timing(False) == (0.0, 0)
        vol.brick_cull, vol.use_palette = True, True
        _fuse(vol, sc.state, sc.im, 1.0)
        assert timing(False) == (0.0, 0)
    finally:
        timing(False)
        vol.brick_cull, vol.use_palette = True, True


def test_a_restatement_reaches_the_edges(A):
    """The weighted scene-A reference really has what the comparison is about: skipped voxels of every bad kind,
    subnormal weights that update, capped and uncapped weights, waves that mix w_new == 1 with other weights."""
    plain = sr.two_frame_fusion(A.sc, A.skin, A.sc.state, 1.0)
    ref = _ref_a(A, CASES[0])
    o = A.wim[plain.py, plain.px]
    for bad in (o == 0, o < 0, np.isnan(o), np.isposinf(o)):
        assert (plain.updated & bad).sum() > 50 and not (ref.updated & bad).any()
    assert (ref.updated & (o == wr.SUBNORMAL)).sum() > 50
    capped = _ref_a(A, CASES[1])
    assert (capped.weight[capped.updated] == F32(2.5)).sum() > 50 and (capped.weight[capped.updated] < F32(2.5)).sum() > 50


@pytest.mark.parametrize("kernel", ["src", "generic"])
def test_d_weighted_source_frame(cuda, kernel, monkeypatch):
    """Scene D's source-frame kernels (k_integrate_src with its pixel tables on a tie, and the generic one), weighted."""
    if kernel == "generic":
        monkeypatch.setenv("OFX_INT_GENERIC", "1")
    sc = sr.scene_d()
    vol = _volume(sc, cuda)
    wim = wr.weight_image(np.random.default_rng(4), sc.height, sc.width)
    wim_t = torch.from_numpy(wim).to(cuda)
    for w_max, obs, col in CASES:
        ref = wr.two_frame_weighted(sc, None, sc.state, obs, wim, w_max, with_color=col)
        vol.with_color = col
        got = _fuse(vol, sc.state, sc.im, obs, frame=0, weight_image=wim_t, max_weight=None if w_max == INF else w_max)
        _check(got, ref, got[3][:vol.n_bricks])
        assert int(got[3][:vol.n_bricks].sum()) == ref.n > 1000


# ------------------------------------------------------------------------------------------------ explicit points
@pytest.fixture(scope="module")
def points_case():
    """test_gpu_integrate_edges.py's adversarial points, depth and old state (48 x 64 x 40)."""
    from occlusionfusion_amd import synthetic as S
    from test_gpu_integrate_edges import adversarial_points
    rng = np.random.default_rng(7)
    cam = S.bench_camera()
    D = (48, 64, 40)
    V = int(np.prod(D))
    pts = adversarial_points(cam, V, rng)
    vox = rng.permutation(V).astype(np.int64)
    valid = rng.random(V) < 0.97
    depth = rng.uniform(0.2, 3.6, (cam.height, cam.width)).astype(F32)
    depth[rng.random(depth.shape) < 0.05] = 0.0
    zz = pts[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        u = np.rint(pts[:, 0].astype(np.float64) * np.float64(F32(cam.fx)) / zz + np.float64(F32(cam.cx)))
        v = np.rint(pts[:, 1].astype(np.float64) * np.float64(F32(cam.fy)) / zz + np.float64(F32(cam.cy)))
    ok = np.isfinite(u) & np.isfinite(v) & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height) & (zz > 0)
    sel = np.nonzero(ok)[0][::3]
    depth[v[sel].astype(int), u[sel].astype(int)] = (zz[sel] + rng.choice([-0.05, -0.04, -0.0399999, 0.0, 0.01, 0.04,
                                                                          0.3], sel.size)).astype(F32)
    state = (rng.uniform(-1, 1, V).astype(F32), rng.choice(np.array([0, 1, 2, 3, 7, 0.5, 1.25], F32), V),
             np.floor(rng.uniform(0, 2 ** 24 - 1, V)).astype(F32))
    P = np.zeros((V, 3), F32)
    P[vox] = pts
    vm = np.zeros(V, bool)
    vm[vox] = valid
    return sr.SimpleNamespace(cam=cam, D=D, V=V, pts=pts, vox=vox, valid=valid, im=S.make_image(depth), state=state,
                              P=P, vm=vm, intr=(cam.fx, cam.fy, cam.cx, cam.cy),
                              wim=wr.weight_image(np.random.default_rng(8), cam.height, cam.width))


def _points_volume(c, cuda):
    from occlusionfusion_amd import TSDFVolume
    vol = TSDFVolume.from_grid((-0.5, -0.5, 0.5), 0.01, c.D, c.intr, _Opt(), device=cuda)
    _load(vol, c.state)
    vol.update(c.im, 3)
    return vol


def test_integrate_points_weighted_bitexact(cuda, points_case):
    c = points_case
    wim_t = torch.from_numpy(c.wim).to(cuda)
    for w_max, obs, col in CASES:
        vol = _points_volume(c, cuda)
        vol.with_color = col
        cnt = vol.integrate_points(c.pts, c.vox, c.valid, obs_weight=obs, count_updates=True, weight_image=wim_t,
                                   max_weight=None if w_max == INF else w_max)
        t, col_gpu, w = (a.reshape(-1) for a in vol.get_volume())
        ref = wr.fuse_points(c.state, c.P, c.vm, fo.depth_of(c.im), fo.pack_color(c.im), c.intr, c.wim, obs, w_max,
                             with_color=col)
        assert ref.n > c.V // 30 and int(cnt.item()) == ref.n
        eq(w, ref.weight)
        eq(t, ref.tsdf)
        eq(col_gpu, ref.color)


# ------------------------------------------------------------------------------------------------ the degenerate form
def test_ones_and_no_cap_is_the_unweighted_call(A, cuda, points_case):
    """A constant weight image of 1.0 and w_max = +inf: byte-identical volumes and update counts to the unweighted call
    on the same inputs, both on the GPU — the warped palette kernel with the cull, the source-frame kernel, the points."""
    sc = A.sc
    ones = torch.ones((sc.height, sc.width), dtype=torch.float32, device=cuda)
    for obs in (1.0, 0.3):
        a = _fuse(A.vol, sc.state, sc.im, obs)
        b = _fuse(A.vol, sc.state, sc.im, obs, weight_image=ones)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        assert not np.array_equal(a[0], sc.state[0].reshape(-1))
    d = sr.scene_d()
    vol = _volume(d, cuda)
    a = _fuse(vol, d.state, d.im, 0.3, frame=0)
    b = _fuse(vol, d.state, d.im, 0.3, frame=0, weight_image=ones)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = points_case
    out = []
    for kw in ({}, dict(weight_image=torch.ones((c.cam.height, c.cam.width), dtype=torch.float32, device=cuda))):
        vol = _points_volume(c, cuda)
        cnt = vol.integrate_points(c.pts, c.vox, c.valid, obs_weight=0.3, count_updates=True, **kw)
        out.append([x.tobytes() for x in vol.get_volume()] + [int(cnt.item())])
    assert out[0] == out[1]
    # a cap alone (no weight image): the unweighted update with the stored weight cut at the cap
    a = _fuse(A.vol, sc.state, sc.im, 1.0)
    b = _fuse(A.vol, sc.state, sc.im, 1.0, max_weight=2.5)
    upd = a[1] != sc.state[1].reshape(-1)
    eq(b[0], a[0]), eq(b[2], a[2]), eq(b[3], a[3])
    eq(b[1], np.where(upd, np.minimum(a[1], F32(2.5)), a[1]))


# ------------------------------------------------------------------------------------------------ the benefit scenario
def _benefit_on_device(cuda, fusion_weights):
    """wr.benefit_scene() fused on the device — the source frame, then the eight frames under their ground-truth node
    transforms, through TSDFVolume.integrate (with fusion_weights the volume builds each frame's map itself, from the
    filtered frame) — and raycast from the camera -> the scenario's RMS depth error in metres."""
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.tsdf import fusion_weight_params
    b = wr.benefit_scene()
    vol = TSDFVolume.from_grid(b.origin, b.vs, b.dims, b.intr, _Opt(), device=cuda)
    vol.with_color = False
    vol.fusion_weights = fusion_weight_params(fusion_weights)
    N = b.nodes.shape[0]
    wf = WarpField(EDGraph(b.nodes, -np.ones((N, 8), np.int32), node_coverage=b.cov), vol)
    for t, d in enumerate(b.frames):
        im = np.zeros((6, b.height, b.width), F32)
        im[5] = d
        if t:
            wf.frame_id = t
            wf.set_node_transforms(b.R[t], b.T[t])
        vol.integrate({"im": im, "id": t})
    depth = vol.raycast()[0].cpu().numpy()
    return wr.benefit_error(b, depth)


def test_benefit_scenario_on_the_device(cuda):
    """The CPU restatement's scenario on the device. The bars come from the restatement's recorded errors (wr.E_U, wr.E_W
    = 1.130 mm, 0.980 mm), not from the code under test: the weighted run must keep at least half of the recorded gain,
    e_w_gpu <= e_u - (e_u - e_w) / 2, and the unweighted run's error lies within 2 % of e_u."""
    e_u_gpu = _benefit_on_device(cuda, None)
    e_w_gpu = _benefit_on_device(cuda, True)
    print(f"benefit scenario on the device: e_u = {1e3 * e_u_gpu:.4f} mm (restatement {1e3 * wr.E_U:.4f}), "
          f"e_w = {1e3 * e_w_gpu:.4f} mm (restatement {1e3 * wr.E_W:.4f})")
    assert abs(e_u_gpu - wr.E_U) <= 0.02 * wr.E_U
    assert e_w_gpu <= wr.E_U - 0.5 * (wr.E_U - wr.E_W)


# ------------------------------------------------------------------------------------------------ the pipeline
def _pipeline(cuda, seq, overlap=False, fusion_weights=None):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"), overlap=overlap, fusion_weights=fusion_weights)
    pipe.integrate_source(pipe.prepare(0))
    return pipe


def _run(pipe, frames=(1, 2, 3), **kw):
    outs = [pipe.track_step(pipe.prepare(t), t, model="volume", max_model_points=16384, **kw) for t in frames]
    pipe.flush()
    torch.cuda.synchronize()
    return outs, [x.cpu().numpy() for x in pipe.vol.get_volume_device()], torch.stack(pipe.model_counts).cpu()


def test_pipeline_fusion_weights(cuda):
    """Config 1, three frames of track_step(model="volume", fusion_weights=True): every sampling accepts points with
    w_min left at its default (the weights' floor: 1.0 would empty the model after the source frame), the weighted
    volume differs from the plain one, overlap=True gives the sequential run byte for byte, and the keyword on
    track_step alone does what the constructor's does."""
    from occlusionfusion_amd import synthetic as S
    seq = S.config_sequence(1, device=cuda)
    outs, vol, counts = _run(_pipeline(cuda, seq, fusion_weights=True))
    print("model counts [accepted, emitted] per sampling:", counts.tolist())
    assert all(o["valid_solve"] == 1 for o in outs)
    assert counts.shape == (4, 2) and bool((counts[:, 0] > 0).all())
    w = vol[2]
    frac = w[(w > 0) & (w != np.floor(w))]
    assert frac.size > 1000                                    # fractional accumulated weights: the map was used
    outs_o, vol_o, counts_o = _run(_pipeline(cuda, seq, overlap=True, fusion_weights=True))
    for a, b in zip(outs, outs_o):
        assert torch.equal(a["node_rotations"], b["node_rotations"])
        assert torch.equal(a["node_translations"], b["node_translations"])
    for a, b in zip(vol, vol_o):
        assert a.tobytes() == b.tobytes()
    assert counts_o.tolist() == counts.tolist()
    outs_k, vol_k, _ = _run(_pipeline(cuda, seq), fusion_weights=True)     # the source frame unweighted, then the keyword
    assert all(o["valid_solve"] == 1 for o in outs_k)
    wk = vol_k[2]
    assert wk[(wk > 0) & (wk != np.floor(wk))].size > 1000
    # fusion_weights=None is the loop as it was: integer weights, and an explicit None on every call changes nothing
    outs_p, vol_p, counts_p = _run(_pipeline(cuda, seq), frames=(1, 2))
    outs_n, vol_n, counts_n = _run(_pipeline(cuda, seq, fusion_weights=None), frames=(1, 2), fusion_weights=None, w_min=1.0)
    assert (vol_p[2] == np.floor(vol_p[2])).all()
    for a, b in zip(vol_p, vol_n):
        assert a.tobytes() == b.tobytes()
    assert counts_p.tolist() == counts_n.tolist()
    # a cap below the model's w_min is refused before any device work
    with pytest.raises(ValueError, match="max_weight"):
        _pipeline(cuda, seq).track_step(None, 1, model="volume", fusion_weights=dict(max_weight=0.5), w_min=1.0)
