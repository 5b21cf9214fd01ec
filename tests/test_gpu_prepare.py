"""GPU: depth-frame preparation (ofx_prepare_depth, torch.ops.ofx.prepare_depth, prepare_depth_device, depth_filter).

* the filtered depth, the vertex map and the normal map equal the numpy restatement (tests/prepare_ref.py) bit for bit —
  radius 0 / 1 / 3 / 4, f32 and u16 input, with and without the normal map — at 40x32 (test_gpu_assoc's scene with noise
  and NaN, +inf, 0, negative and subnormal depths sprinkled over it: tile edges in both directions), 17x33 (partial tiles
  in both directions), 3x5 (smaller than the window) and 1x1; the outputs, prefilled with garbage, come back fully
  overwritten and the input is untouched;
* radius 0 is backproject_depth_device bit for bit; the operator equals the C-ABI call and passes opcheck; two calls
  give the same bytes;
* config 1's frame 20 (320x224) is bit-exact too, and the CPU test's denoising conditions hold for the device's output;
* end to end: test_gpu_assoc's tracking scene with depth_filter=True meets the same bar, depth_filter=None is the loop
  as it was, bit for bit, and a volume-model track_step integrates the raw frame.

The one place where bits are not compared is the payload of a NaN: a +inf depth passes D > 0 and filters to +inf on its
own, but two of them inside one window meet as diff = inf - inf, and the NaN that follows carries the sign the host's or
the device's subtraction gives it. Where the restatement has a NaN the device must have one; everywhere else the bits
must agree.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import prepare_ref as pr  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
INTR = (30.0, 30.0, 19.5, 15.5)
SHAPES = [(32, 40), (17, 33), (3, 5), (1, 1)]     # (H, W)
EDGE = 0.03


def _depth(shape):
    """(H, W) f32 depth: test_gpu_assoc's surface (tilted, gently curved, a 5 cm step at column 28, a block of holes —
    cut to the shape) with seeded 1 mm noise, and NaN, +inf, 0, negative and subnormal depths sprinkled over it."""
    H, W = shape
    rng = np.random.default_rng(2024 + 100 * H + W)
    fx, fy, cx, cy = INTR
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    depth = 1.0 + 0.004 * (u - cx) + 0.02 * np.sin(0.3 * v)
    depth[:, 28:] += 0.05
    depth[12:17, 8:13] = 0.0
    depth = (depth + np.where(depth > 0, rng.normal(0, 0.001, depth.shape), 0.0)).astype(F32)
    if H * W >= 15:
        bad = [np.nan, np.inf, 0.0, -1.0, 1e-41]
        n = max(1, H * W // 100)
        idx = rng.choice(H * W, size=len(bad) * n, replace=False)
        depth.reshape(-1)[idx] = np.repeat(np.array(bad, F32), n)
    return depth


def _u16(depth):
    with np.errstate(all="ignore"):
        mm = np.where(np.isfinite(depth) & (depth > 0), np.rint(depth.astype(np.float64) * 1000.0), 0.0)
    return np.clip(mm, 0, 65535).astype(np.uint16)


_INPUTS, _REFS = {}, {}


def _input(shape, u16):
    """The shared input of a shape: numpy and device copies, made once and never modified."""
    key = (shape, u16)
    if key not in _INPUTS:
        d = _u16(_depth(shape)) if u16 else _depth(shape)
        t = torch.from_numpy(d.view(np.int16) if u16 else d).cuda()
        _INPUTS[key] = (d, t, t.clone())
    return _INPUTS[key]


def _ref(shape, u16, **kw):
    """The restatement's outputs (with normals), computed once per case and shared."""
    key = (shape, u16, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = pr.prepare(_input(shape, u16)[0], INTR, edge_max=EDGE, **kw)
    return _REFS[key]


def _direct(t, intr, radius=3, sigma_s=2.0, sigma_r=0.01, range_cut=None, edge_max=EDGE, normals=True, fill=7.5):
    """ofx_prepare_depth through ctypes, every output prefilled with `fill`."""
    H, W = t.shape
    range_cut = 3.0 * sigma_r if range_cut is None else range_cut
    out = torch.full((H, W), fill, device=t.device)
    pimg = torch.full((3, H, W), fill, device=t.device)
    nimg = torch.full((3, H, W), fill, device=t.device) if normals else None
    cam = _lib.Camera(*intr, W, H)
    prm = _lib.PrepareParams(radius, sigma_s, sigma_r, range_cut, edge_max, 1000.0)
    call("ofx_prepare_depth", ptr(t), 0 if t.dtype == torch.float32 else 1, H, W, byref(cam), byref(prm), ptr(out),
         ptr(pimg), ptr(nimg), stream_ptr())
    return out, pimg, nimg


def _same(got, want):
    """Bit equality, except that a NaN need only be a NaN (module docstring)."""
    got = np.ascontiguousarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, F32)
    want = np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def _assert_equals_ref(out, ref, normals=True):
    assert _same(out[0], ref["depth"])
    assert not np.isnan(ref["point_image"]).any() and _same(out[1], ref["point_image"])
    if normals:
        assert not np.isnan(ref["normals"]).any() and _same(out[2], ref["normals"])


def test_scene_has_what_the_kernel_can_get_wrong():
    d = _depth((32, 40))
    assert np.isnan(d).any() and np.isposinf(d).any() and (d < 0).any() and (d == 0).sum() >= 25
    assert ((d > 0) & (d < 1e-38)).any()
    ref = _ref((32, 40), False, radius=3)
    n = np.abs(ref["normals"]).sum(0) > 0
    print("valid", int((d > 0).sum()), "filtered valid", int((ref["depth"] > 0).sum()), "with a normal", int(n.sum()),
          "NaN out", int(np.isnan(ref["depth"]).sum()))
    assert n.sum() > 400 and (~n & (ref["depth"] > 0)).sum() > 100      # depth edges and hole rims carry no normal
    assert np.isposinf(ref["depth"]).any()                               # a lone +inf depth stays +inf
    assert np.array_equal(np.isposinf(ref["depth"]) | np.isnan(ref["depth"]), np.isposinf(d))
    assert not np.array_equal(ref["depth"].view(np.uint32), np.where(d > 0, d, F32(0)).view(np.uint32))


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no-normals"])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("radius", [0, 1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_restatement(cuda, shape, radius, u16, normals):
    _, t, keep = _input(shape, u16)
    out = _direct(t, INTR, radius=radius, normals=normals, fill=-3.25)
    _assert_equals_ref(out, _ref(shape, u16, radius=radius), normals)
    for o in out[:2] + ((out[2],) if normals else ()):
        assert not bool((o == -3.25).any())                              # every element was written
    assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8))     # the input is only read


@pytest.mark.parametrize("kw", [dict(radius=3, sigma_s=1.5, sigma_r=0.0037, range_cut=0.2),   # f32-subnormal weights
                                dict(radius=2, sigma_s=0.7, sigma_r=0.02, range_cut=0.01),
                                dict(radius=4, sigma_s=3.0, sigma_r=0.01, range_cut=0.06)],
                         ids=["wide-cut", "tight-cut", "across-the-step"])
def test_other_parameters_equal_restatement(cuda, kw):
    for shape in ((32, 40), (17, 33)):
        out = _direct(_input(shape, False)[1], INTR, **kw)
        _assert_equals_ref(out, _ref(shape, False, **kw))


def test_radius_0_is_backproject_depth_device(cuda):
    from occlusionfusion_amd.image_proc import backproject_depth_device, prepare_depth_device
    for u16 in (False, True):
        d, t, _ = _input((32, 40), u16)
        vm = backproject_depth_device(t, *INTR)                          # zero-filled where the depth is not > 0
        out = prepare_depth_device(t, *INTR, radius=0)
        assert torch.equal(out["point_image"].view(torch.int32), vm.view(torch.int32))
        pos = torch.from_numpy(pr.depth_f32(d) > 0).cuda()
        assert torch.equal(out["depth"][pos].view(torch.int32), vm[2][pos].view(torch.int32))
        assert not bool(out["depth"][~pos].any())
        assert int(pos.sum()) > 1000


def test_op_equals_c_abi_and_opcheck(cuda):
    for u16, normals, radius in ((False, True, 3), (True, False, 4), (False, False, 1)):
        _, t, keep = _input((17, 33), u16)
        ref = _direct(t, INTR, radius=radius, normals=normals)
        out = torch.ops.ofx.prepare_depth(t, list(INTR), radius, 2.0, 0.01, 3.0 * 0.01, EDGE, 1000.0, normals)
        assert len(out) == 3 and out[2].shape == ((3 if normals else 0), 17, 33)
        for x, y in zip(out, ref):
            if y is not None:
                assert x.dtype == y.dtype and _same(x, y.cpu().numpy())
        assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8))
    clean = torch.from_numpy(np.where(_depth((17, 33)) > 0, _depth((17, 33)), 0).astype(F32)).cuda()
    torch.library.opcheck(torch.ops.ofx.prepare_depth.default, (clean, list(INTR), 3, 2.0, 0.01, 0.03, EDGE, 1000.0, True))
    torch.library.opcheck(torch.ops.ofx.prepare_depth.default,
                          (_input((17, 33), True)[1], list(INTR), 2, 2.0, 0.01, 0.03, EDGE, 1000.0, False))


def test_python_wrapper_and_its_defaults(cuda):
    from occlusionfusion_amd.image_proc import prepare_depth_device
    d, t, keep = _input((32, 40), False)
    out = prepare_depth_device(t, *INTR)
    _assert_equals_ref((out["depth"], out["point_image"], out["normals"]), _ref((32, 40), False, radius=3))
    out = prepare_depth_device(t, *INTR, radius=4, normals=False)
    assert out["normals"] is None and _same(out["depth"], _ref((32, 40), False, radius=4)["depth"])
    out = prepare_depth_device(_input((32, 40), True)[1].view(torch.uint16), *INTR, radius=1)
    _assert_equals_ref((out["depth"], out["point_image"], out["normals"]), _ref((32, 40), True, radius=1))
    with pytest.raises(_lib.OfxError, match="radius"):
        prepare_depth_device(t, *INTR, radius=5)
    assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8))


def test_two_calls_give_the_same_bytes(cuda):
    _, t, _ = _input((32, 40), False)
    a = _direct(t, INTR, radius=3)
    _direct(_input((17, 33), True)[1], INTR, radius=4)                   # other work in between
    b = _direct(t, INTR, radius=3)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------ config 1, frame 20
def test_config_1_frame_20_is_bit_exact_and_denoised(cuda):
    from occlusionfusion_amd.image_proc import prepare_depth_device
    intr, noisy, clean = pr.config1_frame(20)
    assert noisy.shape == (224, 320)
    t = torch.from_numpy(noisy).cuda()
    out = prepare_depth_device(t, *intr, radius=3, sigma_s=2.0, sigma_r=0.01)
    ref = pr.prepare(noisy, intr, radius=3, sigma_s=2.0, sigma_r=0.01)
    _assert_equals_ref((out["depth"], out["point_image"], out["normals"]), ref)
    raw = prepare_depth_device(t, *intr, radius=0)
    cr = pr.clean_reference(clean, intr)
    dev = [pr.measures(o["depth"].cpu().numpy(), o["point_image"].cpu().numpy(), o["normals"].cpu().numpy(), cr, intr)
           for o in (raw, out)]
    pr.check_denoising(*dev)
    assert np.array_equal(out["depth"].cpu().numpy() > 0, noisy > 0)


# ------------------------------------------------------------------------------------------------ tracking end to end
@pytest.fixture(scope="module")
def tracker(cuda):
    """test_gpu_assoc's tracking scene: config 1 (199 nodes, 320x224), 8229 canonical points, the exact direct solve."""
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
    cp = seq.canonical_points
    pts = cp[np.sort(np.random.default_rng(5).choice(cp.shape[0], 2 * 4096 + 37, replace=False))]
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    return seq, Registration(pts, graph, wf, K, precond="direct"), intr


def _fresh(reg):
    reg.prev_rot = reg.prev_trans = None


def test_tracking_with_the_filter_meets_the_bar_of_the_raw_loop(tracker, cuda):
    """Config 1, precond="direct", frame 0 -> 20 from the identity, 3 ICP iterations, plane mode, depth_filter=True.
    The bar is test_gpu_assoc's: r_icp <= r_gt + 0.25·(r_id - r_gt) with the residual (assoc_ref.depth_residual) taken
    against the RAW depth of the frame, and every association accepting at least 0.8 of the points."""
    from occlusionfusion_amd.association import icp_track
    from occlusionfusion_amd.image_proc import prepare_depth_device
    seq, reg, intr = tracker
    t = 20
    frame = seq.frame(t)
    depth = frame[5]
    src_pcd = reg.source_pcd
    n_pts = src_pcd.shape[0]
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
    # the loop as it was, with and without the keyword: the same bytes
    _fresh(reg)
    plain = reg.track({"im": frame, "id": t}, icp_iters=3, mode="plane")
    _fresh(reg)
    none = reg.track({"im": frame, "id": t}, icp_iters=3, mode="plane", depth_filter=None)
    assert np.array_equal(plain["node_rotations"], none["node_rotations"])
    assert torch.equal(plain["node_translations"].view(torch.int32), none["node_translations"].view(torch.int32))
    assert [x["histogram"] for x in plain["assoc"]] == [x["histogram"] for x in none["assoc"]]
    r_raw = ar.depth_residual(plain["warped_verts"].cpu().numpy(), depth, intr)
    # with the filter
    _fresh(reg)
    out = reg.track({"im": frame, "id": t}, icp_iters=3, mode="plane", depth_filter=True)
    r_icp = ar.depth_residual(out["warped_verts"].cpu().numpy(), depth, intr)
    shares = [x["accepted"] / n_pts for x in out["assoc"]]
    print(f"tracking frame {t}: r_id = {1e3 * r_id:.3f} mm, r_gt = {1e3 * r_gt:.3f} mm, raw loop r_icp = "
          f"{1e3 * r_raw:.3f} mm (shares {[round(x['accepted'] / n_pts, 4) for x in plain['assoc']]}), filtered r_icp = "
          f"{1e3 * r_icp:.3f} mm, accepted shares = {[round(x, 4) for x in shares]}, histograms = "
          f"{[x['histogram'] for x in out['assoc']]}")
    assert out["valid_solve"] == 1 and len(out["assoc"]) == 3
    assert min(shares) >= 0.8, shares
    assert r_gt < r_id
    assert r_icp <= r_gt + 0.25 * (r_id - r_gt), (r_id, r_gt, r_icp)
    assert reg.tgt_pcd.shape == (int((depth > 0).sum()), 3)             # tgt_pcd / pix_2_pcd: still the raw depth's
    # icp_track returns the prepared vertex map; a dict overrides the filter's parameters
    dev_depth = torch.from_numpy(depth).cuda()
    for filt, kw in ((True, {}), ({"radius": 2, "sigma_s": 1.5}, {"radius": 2, "sigma_s": 1.5})):
        _, _, vm = icp_track(reg._assoc, reg.solver, reg.graph.nodes, reg.graph.edges, reg.graph.edges_weights,
                             reg.source_pcd, None, reg.point_anchors, reg.anchor_weight, None, depth, intr, icp_iters=1,
                             max_matches=reg.max_matches, depth_filter=filt)
        want = prepare_depth_device(dev_depth, *intr, normals=False, **kw)["point_image"]
        assert torch.equal(vm.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(vm, prepare_depth_device(dev_depth, *intr, radius=0)["point_image"])
    _fresh(reg)


def test_volume_track_step_integrates_the_raw_frame(tracker, cuda):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    seq = tracker[0]
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"))
    pipe.integrate_source(pipe.prepare(0))
    fi = pipe.prepare(1)
    out = pipe.track_step(fi, 1, model="volume", max_model_points=16384, depth_filter=True)
    assert out["valid_solve"] == 1 and len(out["assoc"]) == 3
    torch.cuda.synchronize()
    assert torch.equal(pipe.vol.depth_t.view(torch.int32), fi.im[-1].view(torch.int32))
    with pytest.raises(TypeError, match="bogus"):
        pipe.track_step(fi, 1, model="volume", max_model_points=16384, depth_filter={"bogus": 1})
