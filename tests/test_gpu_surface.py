"""GPU: skinned surface points of the TSDF (ofx_surface_points, torch.ops.ofx.surface_points, SurfaceSampler,
WarpField.surface_points, Registration.update_from_volume, FusionPipeline.track_step(model="volume")).

* the kernel equals the numpy restatement (tests/surface_ref.py) bit for bit — points, normals, anchors, weights, voxel,
  valid, code and count; max_points above / at / below the accepted count; w_min 1.0 and 0.5 — on a (20, 18, 22) volume
  (3x3x3 bricks, no dim a multiple of 8) with random weights, a partly skinned band and planted degenerate voxels;
* emitted skins are skin_tsdf() at the voxel, and a point moves as its voxel does;
* empty inputs, refused arguments, operator == C ABI, opcheck, determinism, padded rows straight into the associator;
* Registration.update_from_volume + track follows frame 20 of config 1; track_step(model="volume") re-samples per frame
  and leaves the default model's path untouched.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import surface_ref as sr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
DIMS, H_VOX, TRUNC = (20, 18, 22), 0.01, 0.04
ORIGIN = np.zeros(3, F32)
CENTRE, RADIUS = np.array([0.095, 0.085, 0.105]), 0.06
COVERAGE = 0.02                        # 4 sigma = 0.08 m: the nodes sit on one side of the sphere, the far band is unskinned
V = int(np.prod(DIMS))
# planted voxels, all in the (1, 1, 1) corner where the sphere's tsdf is 1 (more than trunc away)
P_MIRROR, P_LONG, P_NEGZERO, P_NAN, P_NANNB, P_BOUNDARY = (2, 2, 2), (2, 2, 6), (2, 6, 2), (6, 2, 2), (5, 5, 2), (0, 5, 5)


def _nbrs(v):
    return [tuple(np.add(v, d)) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]


def _plant(phi, v, centre, values):
    """values: the six face neighbours' tsdf in the order +x -x +y -y +z -z."""
    phi[v] = centre
    for n, x in zip(_nbrs(v), values):
        phi[n] = x


def scene_arrays():
    """(tsdf, weight, nodes): the analytic sphere over trunc, weights drawn from {0, 0.5, 1, 2, 3.5} (about 10 % zeros),
    14 nodes on the sphere's (-1, -1, -1) side, and the planted voxels with fully observed neighbourhoods."""
    rng = np.random.default_rng(77)
    c = fo.world_points(ORIGIN, DIMS, H_VOX).reshape(DIMS + (3,)).astype(np.float64)
    phi = np.clip((np.linalg.norm(c - CENTRE, axis=-1) - RADIUS) / TRUNC, -1, 1).astype(F32)
    w = rng.choice(np.array([0, 0.5, 1, 2, 3.5], F32), size=DIMS, p=[0.1, 0.05, 0.3, 0.3, 0.25])
    d = np.array([-1.0, -1.0, -1.0]) / np.sqrt(3) + 0.9 * rng.normal(size=(14, 3))
    nodes = (CENTRE + RADIUS * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    _plant(phi, P_MIRROR, 0.5, (-0.2, -0.2, 0.3, 0.3, 0.1, 0.1))        # g = 0
    _plant(phi, P_LONG, 0.9, (-0.05, 0.0, 0.4, 0.4, 0.4, 0.4))          # len = 0.05 < phi
    _plant(phi, P_NEGZERO, -0.0, (0.0, 0.0, 0.0, 0.0, -0.3, 0.3))       # phi = -0.0 is >= 0: accepted, t = -0
    _plant(phi, P_NAN, np.nan, (0.3, 0.3, 0.3, 0.3, 0.3, 0.3))          # NaN fails code 3's test
    _plant(phi, P_NANNB, 0.2, (np.nan, 0.1, 0.2, 0.2, 0.2, -0.1))       # a NaN neighbour: NaN gradient
    phi[P_BOUNDARY] = 0.2
    for v in (P_MIRROR, P_LONG, P_NEGZERO, P_NAN, P_NANNB):
        w[v] = 2.0
        for n in _nbrs(v):
            w[n] = 1.0
    w[P_BOUNDARY] = 1.0
    return phi, w, nodes


def _upload(vol, dense, dst):
    src = torch.from_numpy(np.ascontiguousarray(dense, F32)).to(vol.device)
    call("ofx_volume_from_dense", byref(vol.desc), ptr(src), ptr(dst), stream_ptr())


def _volume(cuda, phi, w, nodes, coverage=COVERAGE):
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.synthetic import euclidean_edges
    vol = TSDFVolume.from_grid(ORIGIN, H_VOX, DIMS, (100.0, 100.0, 20.0, 16.0), SimpleNamespace(source_frame=0, skip_rate=1),
                               device=cuda)
    _upload(vol, phi, vol.tsdf_b)
    _upload(vol, w, vol.weight_b)
    e, ew = euclidean_edges(nodes, 8)
    wf = WarpField(EDGraph(nodes, e, ew, node_coverage=coverage), vol)
    return vol, wf


@pytest.fixture(scope="module")
def scene(cuda):
    phi, w, nodes = scene_arrays()
    vol, wf = _volume(cuda, phi, w, nodes)
    cache = wf.skin_tsdf_cache()
    a, sw, sv = wf.skin_tsdf()
    blist = cache.brick_list[:cache.n_list].cpu().numpy()
    assert cache.k == 4 and cache.n_list > 8
    return dict(phi=phi, w=w, nodes=nodes, vol=vol, wf=wf, cache=cache, skin_a=a, skin_w=sw, skin_v=sv, blist=blist,
                ref={})


def _ref(s, w_min, M):
    """The restatement for (w_min, max_points), computed once and shared (never modified)."""
    key = (float(w_min), int(M))
    if key not in s["ref"]:
        s["ref"][key] = sr.surface_points(s["phi"], s["w"], ORIGIN, H_VOX, s["blist"], s["skin_a"], s["skin_w"], w_min, M)
    return s["ref"][key]


class _Handle:
    def __init__(self, max_bricks):
        self.h = _lib.c_void_p()
        call("ofx_surface_create", max_bricks, byref(self.h))

    def __del__(self):
        _lib.lib.ofx_surface_destroy(self.h)


def _buffers(M, n_list, dev, fill=-3):
    return [torch.full((M, 3), float(fill), device=dev), torch.full((M, 3), float(fill), device=dev),
            torch.full((M, 4), fill, dtype=torch.int32, device=dev), torch.full((M, 4), float(fill), device=dev),
            torch.full((M,), fill, dtype=torch.int32, device=dev), torch.full((M,), 99, dtype=torch.uint8, device=dev),
            torch.full((max(1, n_list) * 512,), 99, dtype=torch.uint8, device=dev),
            torch.full((2,), -7, dtype=torch.int32, device=dev)]


def _direct(handle, s, w_min, M, n_list=None, desc=None, k=4, status=False, with_code=True):
    """ofx_surface_points through ctypes; every output prefilled with garbage."""
    vol, c = s["vol"], s["cache"]
    n_list = c.n_list if n_list is None else n_list
    out = _buffers(M, n_list, vol.device)
    args = (handle.h, byref(desc if desc is not None else vol.desc), ptr(vol.tsdf_b), ptr(vol.weight_b), ptr(c.brick_list),
            n_list, ptr(c.anchors), ptr(c.weights), k, float(w_min), M, *[ptr(t) for t in out[:6]],
            ptr(out[6]) if with_code else None, ptr(out[7]), stream_ptr())
    if status:
        return _lib.lib.ofx_surface_points(*args)
    call("ofx_surface_points", *args)
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


KEYS = ("points", "normals", "anchors", "weights", "voxel", "valid", "code", "count")


def _assert_equals_ref(out, ref, n_list):
    got = dict(zip(KEYS, (t.cpu().numpy() for t in out)))
    assert got["count"].tolist() == ref["count"].tolist()
    assert np.array_equal(got["code"][:n_list * 512], ref["code"])
    for k in KEYS[:6]:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k          # the padding rows included


def test_scene_reaches_every_code(scene):
    ref = _ref(scene, 1.0, V)
    hist = np.bincount(ref["code"], minlength=8)
    print("codes 0..7:", hist.tolist(), "listed bricks:", scene["cache"].n_list)
    assert np.all(hist > 0) and hist[0] > 50
    code = {}
    i, j, k, inside = sr.listed_voxels(DIMS, scene["blist"])
    flat = {(a, b, c): q for q, (a, b, c, ok) in enumerate(zip(i.ravel(), j.ravel(), k.ravel(), inside.ravel())) if ok}
    for name, v in (("mirror", P_MIRROR), ("long", P_LONG), ("negzero", P_NEGZERO), ("nan", P_NAN), ("nannb", P_NANNB),
                    ("boundary", P_BOUNDARY)):
        code[name] = int(ref["code"][flat[v]])
    assert code == dict(mirror=6, long=6, negzero=0, nan=3, nannb=6, boundary=1), code
    # phi = -0.0: the Newton step is -0, the point is the voxel itself
    row = int(np.nonzero(ref["voxel"] == np.ravel_multi_index(P_NEGZERO, DIMS))[0][0])
    assert np.array_equal(ref["points"][row], (np.array(P_NEGZERO) * H_VOX).astype(F32))
    assert np.array_equal(ref["normals"][row], np.array([0, 0, -1], F32))
    # some band voxels are skin-invalid, most are not
    assert 20 < hist[7] < hist[0] * 4


@pytest.mark.parametrize("w_min", [1.0, 0.5])
@pytest.mark.parametrize("mm", ["above", "exact", "below"])
def test_kernel_equals_restatement(scene, mm, w_min):
    n_acc = int(_ref(scene, w_min, 0)["count"][0])
    assert n_acc > 50
    M = {"above": n_acc + 37, "exact": n_acc, "below": 40}[mm]
    ref = _ref(scene, w_min, M)
    assert ref["count"].tolist() == [n_acc, min(n_acc, M)]
    n_list = scene["cache"].n_list
    _assert_equals_ref(_direct(_Handle(n_list), scene, w_min, M), ref, n_list)


def test_more_bricks_than_one_scan_trip(scene):
    """The scan of the per-brick counts takes 4096 entries a trip, four per thread: 4110 slots (the 16 listed bricks
    over and over, each slot with its brick's cached skin) run two trips and a ragged last group of two."""
    from types import SimpleNamespace
    c = scene["cache"]
    n = 4110
    reps = -(-n // c.n_list)
    big = SimpleNamespace(brick_list=c.brick_list[:c.n_list].repeat(reps)[:n].contiguous(), n_list=n, k=4,
                          anchors=c.anchors[:c.n_list * 2048].repeat(reps)[:n * 2048].contiguous(),
                          weights=c.weights[:c.n_list * 2048].repeat(reps)[:n * 2048].contiguous())
    s = dict(scene, cache=big, blist=big.brick_list.cpu().numpy(), ref={})
    for M in (50000, 1000):
        ref = _ref(s, 1.0, M)
        assert ref["count"][0] > 18000 and ref["count"][1] == min(M, ref["count"][0])
        _assert_equals_ref(_direct(_Handle(n), s, 1.0, M), ref, n)


def test_more_points_with_a_lower_w_min(scene):
    assert _ref(scene, 0.5, 0)["count"][0] > _ref(scene, 1.0, 0)["count"][0]


def test_emitted_skin_is_the_voxels_cached_skin(scene):
    out = _direct(_Handle(64), scene, 1.0, V)
    n = int(out[7][1])
    vox = out[4][:n].cpu().numpy()
    assert n > 50 and np.all(np.diff(vox) != 0)
    assert np.array_equal(out[2][:n].cpu().numpy(), scene["skin_a"][vox])
    assert np.array_equal(_bits(out[3][:n].cpu().numpy()), _bits(scene["skin_w"][vox]))
    assert np.all(scene["skin_v"][vox])


def test_a_point_moves_as_its_voxel_does(scene, cuda):
    """Identity rotations, arbitrary translations: ofx_deform_points of an emitted point with its row minus the point
    equals the same warp of its voxel's position minus that position. Exactly, W(x) - x = Σ w_k t_k - (1 - Σw)·x: the
    blend of the translations, the same for both, and a term from the skin weights' normalisation by Σ + 1e-6, which
    differs between the two arguments by (1 - Σw)·|p - c| per row. The two sides are separately rounded sums of four
    terms ((x - g) + g + t)·w over coordinates below 0.25, each within 8 ulp(0.25) = 8·2^-25 of the exact value. So per
    row |difference| <= (1 - Σw)·|p - c|_inf + 2^-21, against translations of centimetres."""
    from occlusionfusion_amd.association import pack_transforms
    out = _direct(_Handle(64), scene, 1.0, V)
    n = int(out[7][1])
    p, a, w, vox = out[0][:n], out[2][:n], out[3][:n], out[4][:n].long()
    T = torch.from_numpy(np.random.default_rng(3).normal(0, 0.02, (14, 3)).astype(F32)).to(cuda)
    packed = pack_transforms(torch.from_numpy(scene["nodes"]).to(cuda), None, T, cuda)
    c = torch.from_numpy(fo.world_points(ORIGIN, DIMS, H_VOX)).to(cuda)[vox]
    dp = torch.ops.ofx.deform_points(p.contiguous(), a.contiguous(), w.contiguous(), None, packed, False) - p
    dc = torch.ops.ofx.deform_points(c.contiguous(), a.contiguous(), w.contiguous(), None, packed, False) - c
    diff = (dp.double() - dc.double()).abs().max(dim=1).values
    bound = (1.0 - w.double().sum(1)).abs() * (p.double() - c.double()).abs().max(dim=1).values + 2.0 ** -21
    print(f"max |(W(p) - p) - (W(c) - c)| = {diff.max().item():.3e} (largest bound {bound.max().item():.3e}), "
          f"max |W(c) - c| = {dc.abs().max().item():.3e}")
    assert dc.abs().max().item() > 5e-3 and bound.max().item() < 5e-5
    assert bool((diff <= bound).all())


def test_empty_list_and_no_zero_level(scene, cuda):
    h = _Handle(64)
    out = _direct(h, scene, 1.0, 50, n_list=0)
    ref0 = sr.surface_points(scene["phi"], scene["w"], ORIGIN, H_VOX, scene["blist"][:0], scene["skin_a"], scene["skin_w"],
                             1.0, 50)
    assert out[7].tolist() == [0, 0]
    _assert_equals_ref(out, ref0, 0)
    for level in (1.0, 0.5):                  # all outside the band / inside it but nowhere near a sign change
        flat = np.full(DIMS, level, F32)
        vol, wf = _volume(cuda, flat, np.ones(DIMS, F32), scene["nodes"])
        wf.skin_tsdf_cache()
        m = wf.surface_points(64, with_codes=True, sync=False)
        assert m["count"].tolist() == [0, 0] and m["points"].shape == (64, 3)
        assert not m["valid"].any() and bool((m["voxel"] == -1).all())
        for k in ("points", "normals", "anchors", "weights"):
            assert not m[k].any()
        assert set(m["code"].unique().tolist()) <= ({1, 3} if level == 1.0 else {1, 5})
        s = wf.surface_points(64, with_codes=True)
        assert (s["accepted"], s["emitted"]) == (0, 0) and s["points"].shape == (0, 3) and s["histogram"][0] == 0


def test_refused_arguments(scene):
    c = scene["cache"]
    small = _Handle(c.n_list - 1)
    assert _direct(small, scene, 1.0, 10, status=True) == -1
    assert b"max_bricks" in _lib.lib.ofx_last_error()
    h = _Handle(c.n_list)
    shard = _lib.VolumeDesc.from_buffer_copy(scene["vol"].desc)
    shard.brick_x0, shard.brick_x1 = 1, 3
    assert _direct(h, scene, 1.0, 10, desc=shard, status=True) == -1
    assert b"whole volume" in _lib.lib.ofx_last_error()
    shard.brick_x0, shard.brick_x1 = 0, 2
    assert _direct(h, scene, 1.0, 10, desc=shard, status=True) == -1
    assert b"whole volume" in _lib.lib.ofx_last_error()
    assert _direct(h, scene, 1.0, 10, k=3, status=True) == -1
    assert b"K = 4" in _lib.lib.ofx_last_error()
    out = _direct(h, scene, 1.0, 10, with_code=False)           # code may be NULL
    assert out[7].tolist()[1] == 10 and bool((out[6] == 99).all())
    from types import SimpleNamespace
    from occlusionfusion_amd import TSDFVolume, WarpField
    with pytest.raises(RuntimeError, match="skin cache"):
        WarpField(scene["wf"].graph, scene["vol"]).surface_points(10)
    scene["vol"].warpfield = scene["wf"]
    slab = TSDFVolume.from_grid(ORIGIN, H_VOX, DIMS, (100.0, 100.0, 20.0, 16.0), SimpleNamespace(source_frame=0, skip_rate=1),
                                device=scene["vol"].device, shard=(0, 2))
    wf = WarpField(scene["wf"].graph, slab)
    wf.skin_tsdf_cache()
    with pytest.raises(ValueError, match="sharded"):
        wf.surface_points(10)


def test_op_equals_c_abi_and_opcheck(scene, cuda):
    vol, c = scene["vol"], scene["cache"]
    h = _Handle(c.n_list)
    st = torch.zeros(1, dtype=torch.int32, device=cuda)
    geo = ([int(v) for v in DIMS], [0.0, 0.0, 0.0], H_VOX, TRUNC)
    for w_min, M, with_code in ((1.0, 40, True), (0.5, 3000, False)):
        ref = _direct(h, scene, w_min, M)
        out = _buffers(M, c.n_list, cuda, fill=5)
        r = torch.ops.ofx.surface_points(st, h.h.value, vol.tsdf_b, vol.weight_b, c.brick_list, c.n_list, c.anchors,
                                         c.weights, 4, *geo, w_min, *out[:6], out[6] if with_code else None, out[7])
        assert r is None
        for q, (x, y) in enumerate(zip(out, ref)):
            if q != 6 or with_code:
                assert x.dtype == y.dtype and torch.equal(x, y), KEYS[q]
    out = _buffers(64, c.n_list, cuda)
    torch.library.opcheck(torch.ops.ofx.surface_points.default,
                          (st, h.h.value, vol.tsdf_b, vol.weight_b, c.brick_list, c.n_list, c.anchors, c.weights, 4, *geo,
                           1.0, *out))


def test_determinism_across_calls_and_handles(scene):
    n_list = scene["cache"].n_list
    h1, h2 = _Handle(n_list), _Handle(n_list + 100)
    a = _direct(h1, scene, 1.0, 40)
    _direct(h1, scene, 0.5, 7)                                  # other work on the handle in between
    b = _direct(h1, scene, 1.0, 40)
    c = _direct(h2, scene, 1.0, 40)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_sampler_and_warpfield_layers(scene):
    wf = scene["wf"]
    n_acc = int(_ref(scene, 1.0, 0)["count"][0])
    ref = _ref(scene, 1.0, n_acc + 37)
    m = wf.surface_points(n_acc + 37, with_codes=True)
    assert (m["accepted"], m["emitted"]) == (n_acc, n_acc)
    assert m["histogram"] == np.bincount(ref["code"], minlength=8).tolist()
    for k in KEYS[:6]:
        assert m[k].shape[0] == n_acc and np.array_equal(_bits(m[k].cpu().numpy()), _bits(ref[k][:n_acc])), k
    p = wf.surface_points(n_acc + 37, sync=False)
    assert p["points"].shape[0] == n_acc + 37 and p["count"].is_cuda and p["code"] is None
    for k in KEYS[:6]:
        assert np.array_equal(_bits(p[k].cpu().numpy()), _bits(ref[k])), k


def test_padded_rows_go_straight_to_the_associator(scene, cuda):
    """The padded arrays with their valid mask give the association of the emitted rows; padding rows are code 1."""
    from occlusionfusion_amd.association import ProjectiveAssociator
    from occlusionfusion_amd.image_proc import backproject_depth_device
    wf = scene["wf"]
    n_acc = int(_ref(scene, 1.0, 0)["count"][0])
    M = n_acc + 37
    m = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in wf.surface_points(M, sync=False).items()}
    intr = (6.0, 6.0, 19.5, 15.5)
    vm = backproject_depth_device(torch.full((32, 40), 0.1, device=cuda), *intr)
    wf.set_node_transforms(np.tile(np.eye(3, dtype=F32), (14, 1, 1)), np.zeros((14, 3), F32))
    prm = dict(dist_max=0.06, cos_min=0.0, edge_max=0.03, mode="plane", max_matches=5000)
    pa = ProjectiveAssociator(M, cuda)
    full = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in
            pa.associate(m["points"], m["normals"], m["anchors"], m["weights"], m["valid"], wf, vm, intr, **prm).items()}
    cut = pa.associate(m["points"][:n_acc], m["normals"][:n_acc], m["anchors"][:n_acc], m["weights"][:n_acc], None, wf,
                       vm, intr, **prm)
    assert 0 < full["accepted"] <= n_acc and full["emitted"] == cut["emitted"] and full["accepted"] == cut["accepted"]
    assert bool((full["code"][n_acc:] == 1).all()) and torch.equal(full["code"][:n_acc], cut["code"])
    for k in ("match_idx", "src", "tgt", "anchors", "weights"):
        assert torch.equal(full[k], cut[k]), k


# ------------------------------------------------------------------------------------------------ tracking end to end
@pytest.fixture(scope="module")
def tracker(cuda):
    """test_gpu_assoc.py's tracker fixture (config 1, exact direct solve), with the source frame integrated and the skin
    cache built; the model is not given: Registration starts from a handful of canonical points and takes the volume's."""
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.registration import Registration
    c = S.BASELINE_CONFIGS[1]
    seq = S.config_sequence(1, device=cuda)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = c["dims"]
    vol = TSDFVolume.from_grid(c["origin"], c["voxel"], (D, D, D), intr, SimpleNamespace(source_frame=0, skip_rate=1),
                               device=cuda)
    graph = EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage)
    wf = WarpField(graph, vol)
    vol.integrate({"im": seq.frame(0), "id": 0})
    wf.skin_tsdf_cache()
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(seq.canonical_points[:64], graph, wf, K, max_matches=20000, precond="direct")
    return seq, reg, intr


def test_tracking_follows_a_depth_frame_with_the_volume_model(tracker, cuda):
    """Config 1, frame 0 -> frame 20 from the identity, 3 ICP iterations, plane mode, the model sampled from the volume
    (Registration.update_from_volume) and gated with its own normals. The project's tracking criterion: the depth
    residual (assoc_ref.depth_residual) of the warped model must close three quarters of the gap that one solve on the
    ground-truth matches (seq.solver_inputs(20, 3000)) closes, and every association accepts at least 0.8 of the emitted
    model points. Frame 20 is the frame used: under the identity the CPU chain (oracle integrate, surface_ref,
    assoc_ref; test_surface_ref.py) accepts 0.852 of the model there (0.935 at frame 10, 0.942 at frame 5)."""
    seq, reg, intr = tracker
    t = 20
    frame = seq.frame(t)
    depth = frame[5]
    n_pts = reg.update_from_volume()
    assert n_pts == reg.source_pcd.shape[0] == reg.source_normals.shape[0] > 5000
    assert reg.valid_source_verts.all() and reg.valid_source_verts.shape == (n_pts,)
    assert reg.point_anchors.dtype == torch.int32 and bool((reg.point_anchors >= 0).all())
    src_pcd = reg.source_pcd
    r_id = ar.depth_residual(src_pcd.cpu().numpy(), depth, intr)
    src, tgt, tpos, _ = seq.solver_inputs(t, 3000)
    a, w, v = reg.warpfield.skin_device(src)
    src_t, tgt_t = torch.from_numpy(src).to(cuda)[v], torch.from_numpy(tgt).to(cuda)[v]
    gt = reg.solver.optimize(seq.nodes, seq.edges, seq.edge_weights, tpos, np.zeros(len(seq.nodes), np.float32), src_t,
                             a[v], w[v], tgt_t, intr)
    assert gt["valid_solve"] == 1
    reg.warpfield.set_node_transforms(gt["node_rotations"], gt["node_translations"])
    r_gt = ar.depth_residual(reg.warpfield.deform_device(src_pcd, reg.point_anchors, reg.anchor_weight).cpu().numpy(),
                             depth, intr)
    assert reg.prev_rot is None and reg.prev_trans is None
    out = reg.track({"im": frame, "id": t}, icp_iters=3, mode="plane")
    r_icp = ar.depth_residual(out["warped_verts"].cpu().numpy(), depth, intr)
    shares = [x["accepted"] / n_pts for x in out["assoc"]]
    print(f"volume model, frame {t}: {n_pts} points, r_id = {1e3 * r_id:.3f} mm, r_gt = {1e3 * r_gt:.3f} mm, "
          f"r_icp = {1e3 * r_icp:.3f} mm, accepted shares = {[round(x, 4) for x in shares]}, "
          f"histograms = {[x['histogram'] for x in out['assoc']]}")
    assert out["valid_solve"] == 1
    assert len(out["assoc"]) == 3 and out["target_frame_id"] == t
    assert all(sum(x["histogram"]) == n_pts and x["histogram"][0] == x["accepted"] for x in out["assoc"])
    assert min(shares) >= 0.8, shares
    assert r_gt < r_id
    assert r_icp <= r_gt + 0.25 * (r_id - r_gt), (r_id, r_gt, r_icp)


def _pipeline(cuda, seq, overlap=False):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"), overlap=overlap)
    pipe.integrate_source(pipe.prepare(0))
    return pipe


def test_pipeline_tracks_with_the_volume_model(tracker, cuda):
    """Three frames of track_step(model="volume"): every solve valid, the model re-sampled after every integrate (the
    device counts are read once, at the end), and the default model's path untouched: the next default track_step gives
    the transforms a pipeline that never used the volume model gives from the same state."""
    seq = tracker[0]
    pipe = _pipeline(cuda, seq)
    fis = [pipe.prepare(t) for t in (1, 2, 3, 4)]
    outs = [pipe.track_step(fis[t - 1], t, model="volume", max_model_points=16384) for t in (1, 2, 3)]
    status = torch.stack([o["_status"] for o in outs]).cpu()
    counts = torch.stack(pipe.model_counts).cpu()                 # the one read of the model's counts
    print("model counts [accepted, emitted] per sampling:", counts.tolist(),
          "accepted by the associations:", [[x["accepted"] for x in o["assoc"]] for o in outs])
    assert all(o["valid_solve"] == 1 for o in outs) and bool((status[:, 0] == 1).all())
    assert counts.shape == (4, 2) and bool((counts[:, 0] > 5000).all()) and bool((counts[:, 1] <= 16384).all())
    assert len(set(counts[:, 0].tolist())) > 1                    # the integrates changed the sampled surface
    assert pipe._vmodel["points"].shape == (16384, 3)
    for o in outs:
        assert all(x["accepted"] >= 0.8 * min(int(c) for c in counts[:, 1]) for x in o["assoc"])
    rot, trans = pipe.prev_rot.clone(), pipe.prev_trans.clone()
    a = pipe.track_step(fis[3], 4)
    fresh = _pipeline(cuda, seq)
    fresh.prev_rot, fresh.prev_trans, fresh.vol.frame_id = rot, trans, 3
    b = fresh.track_step(fresh.prepare(4), 4)
    assert a["valid_solve"] == b["valid_solve"] == 1
    assert torch.equal(a["node_rotations"], b["node_rotations"])
    assert torch.equal(a["node_translations"], b["node_translations"])
    assert len(pipe.model_counts) == 4 and fresh._vmodel is None
    # overlap=True: the integrate and the re-sampling run on the integrate stream, the next association waits for them
    ov = _pipeline(cuda, seq, overlap=True)
    for t in (1, 2):
        o = ov.track_step(ov.prepare(t), t, model="volume", max_model_points=16384)
        assert torch.equal(o["node_rotations"], outs[t - 1]["node_rotations"])
        assert torch.equal(o["node_translations"], outs[t - 1]["node_translations"])
    assert torch.stack(ov.model_counts).cpu().tolist() == counts[:3].tolist()
