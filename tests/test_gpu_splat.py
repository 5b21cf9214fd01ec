"""GPU: the model z-buffer (ofx_splat_points, torch.ops.ofx.splat_points, ModelRenderer) and the occlusion gate of the
tracking loop (icp_track / track_step with occlusion=True, WarpField.render_live).

* depth, index, code, warped and warped_normals equal the numpy restatement (tests/splat_ref.py) bit for bit — the
  two-layer scene under a non-identity warp with and without normals (P = 11 482: 44 workgroups and a ragged one), and
  the hand-made cases: clamp, clip, NaN, bad normals, ties, P = 0;
* two calls and two handles give the same bytes, a permutation of the points leaves the depth unchanged, and a handle
  used at two image sizes gives what a fresh handle gives;
* the operator equals the direct C-ABI call and passes opcheck; refused arguments are refused;
* icp_track on the two-layer scene: occlusion=False is byte-equal to the loop before a renderer ever existed and pulls the
  hidden rear nodes onto the front patch; occlusion=True leaves them where they are and matches no hidden point;
* three frames of track_step(model="volume", occlusion=True) at config 1, then render_live against the last frame.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_ref as sp  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
RHO, MARGIN = 0.004, 0.01
SMALL = dict(intr=(100.0, 100.0, 16.0, 16.0), H=33, W=33)


class _Handle:
    def __init__(self, max_points, max_pixels):
        self.h = _lib.c_void_p()
        call("ofx_splat_create", max_points, max_pixels, byref(self.h))

    def __del__(self):
        _lib.lib.ofx_splat_destroy(self.h)


def _dev(cuda, **arrays):
    return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in arrays.items()}


def _direct(handle, d, intr, H, W, rho=RHO, margin=MARGIN, normals=True, n=None, outputs="dickn", valid=True):
    """ofx_splat_points through ctypes on the first n points (valid=False: a NULL valid); outputs prefilled, those not in
    `outputs` passed as NULL."""
    dev = d["packed"].device
    n = d["pts"].shape[0] if n is None else n
    depth = torch.full((H, W), 7.0, device=dev)
    index = torch.full((H, W), 77, dtype=torch.int32, device=dev)
    code = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    warped, wn = torch.full((n, 3), 7.0, device=dev), torch.full((n, 3), 7.0, device=dev)
    cam = _lib.Camera(*intr, W, H)
    prm = _lib.SplatParams(rho, margin)
    use = lambda c, t: ptr(t) if c in outputs else None   # noqa: E731
    call("ofx_splat_points", handle.h, ptr(d["pts"]), ptr(d["nrm"]) if normals else None, ptr(d["anchors"]),
         ptr(d["weights"]), ptr(d.get("valid")) if valid else None, n, ptr(d["packed"]), d["packed"].shape[0], byref(cam), byref(prm),
         use("d", depth), use("i", index), use("c", code), use("k", warped), use("n", wn) if normals else None,
         stream_ptr())
    return depth, index, code, warped, wn


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_equals_ref(out, ref, normals=True):
    depth, index, code, warped, wn = (t.cpu().numpy() for t in out)
    assert np.array_equal(code, ref["code"]), (np.bincount(code, minlength=5), np.bincount(ref["code"], minlength=5))
    assert np.array_equal(_bits(warped), _bits(ref["warped"]))
    if normals:
        assert np.array_equal(_bits(wn), _bits(ref["warped_normals"]))
    assert np.array_equal(_bits(depth), _bits(ref["depth"]))
    assert np.array_equal(index, ref["index"])


# ------------------------------------------------------------------------------------------------ the two-layer scene
@pytest.fixture(scope="module")
def two(cuda):
    """The two-layer scene; `moved`: its front patch's nodes turned by a few degrees and shifted by centimetres, 3 % of
    the points marked invalid, one with an anchor outside the graph."""
    from occlusionfusion_amd.association import pack_transforms
    sc = sp.two_layer_scene()
    rng = np.random.default_rng(11)
    N, P = sc["nodes"].shape[0], sc["points"].shape[0]
    front = sc["nodes"][:, 2] < 1.02
    R = np.tile(np.eye(3, dtype=F32), (N, 1, 1))
    T = np.zeros((N, 3), F32)
    R[front] = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.05, (int(front.sum()), 3))).astype(F32)
    T[front] = rng.normal(0, 0.015, (int(front.sum()), 3)).astype(F32)
    valid = (rng.random(P) >= 0.03).astype(np.uint8)
    anchors = sc["anchors"].copy()
    anchors[5, 2] = N
    sc.update(R=R, T=T, valid=valid, anchors_bad=anchors)
    d = _dev(cuda, pts=sc["points"], nrm=sc["normals"], anchors=anchors, weights=sc["weights"], valid=valid,
             nodes=sc["nodes"], R=R, T=T)
    d["packed"] = pack_transforms(d["nodes"], d["R"], d["T"], cuda)
    sc["dev"] = d
    sc["ref"] = {nm: sp.splat(sc["points"], sc["normals"] if nm else None, anchors, sc["weights"], valid, R, T,
                              sc["nodes"], sc["intr"], sc["H"], sc["W"], RHO, MARGIN) for nm in (True, False)}
    return sc


@pytest.mark.parametrize("normals,valid", [pytest.param(True, True, id="True"), pytest.param(False, True, id="False"),
                                           pytest.param(True, False, id="True-NULL"),
                                           pytest.param(False, False, id="False-NULL")])
def test_kernel_equals_restatement_on_the_two_layers(two, normals, valid):
    """valid given, and valid = NULL (the kernel's VALID = false): then only the anchor outside the graph is invalid."""
    ref = two["ref"][normals] if valid else sp.splat(
        two["points"], two["normals"] if normals else None, two["anchors_bad"], two["weights"], None, two["R"], two["T"],
        two["nodes"], two["intr"], two["H"], two["W"], RHO, MARGIN)
    hist = np.bincount(ref["code"], minlength=5)
    print("codes 0..4:", hist.tolist(), "covered pixels:", int((ref["depth"] > 0).sum()))
    assert hist[0] > 5000 and (hist[1] > 100 if valid else hist[1] == 1) and hist[4] > 500
    P = two["points"].shape[0]
    assert P % 256 != 0 and P > 256
    out = _direct(_Handle(P, two["H"] * two["W"]), two["dev"], two["intr"], two["H"], two["W"], normals=normals,
                  valid=valid)
    _assert_equals_ref(out, ref, normals)
    if not normals:
        assert torch.all(out[4] == 7.0)                     # warped_normals is not touched without normals


def _hand_cases():
    """The hand-made cases of test_splat_ref under one identity node at the origin (the warp is then exact): a clamped
    radius, footprints clipped at two corners, NaN and behind-the-camera points, NaN / back-facing / tilted normals,
    identical points, an occluded point, invalid rows."""
    x = np.array([[0.0, 0.0, 0.05], [-0.16, -0.16, 1.0], [0.16, 0.16, 1.0], [np.nan, 0, 1], [0, 0.05, -1.0],
                  [5.0, 0, 1], [0.06, 0.1, 1.0], [0.09, 0.1, 1.0], [0.002, -0.101, 1.0], [0.002, -0.101, 1.0],
                  [-0.1, -0.1, 1.0], [-0.1, 0.06, 1.1], [-0.1, 0.061, 1.13], [0.1, -0.05, 0.9], [0.0, 0.1, 1.0],
                  [np.inf, 0, 1]], F32)
    t = np.deg2rad(60.0)
    n = np.tile(np.array([0, 0, -1], F32), (x.shape[0], 1))
    n[6] = [np.nan, 0, -1]
    n[7] = [0, 0, 1]
    n[13] = [np.sin(t), 0, -np.cos(t)]
    n[14] = [0, 2.0, -2.0]                                   # not unit: normalised by the warp
    valid = np.ones(x.shape[0], np.uint8)
    valid[10] = 0
    a = np.zeros((x.shape[0], 4), np.int32)
    w = np.tile(np.array([1, 0, 0, 0], F32), (x.shape[0], 1))
    return x, n, a, w, valid


@pytest.mark.parametrize("normals", [True, False])
def test_hand_made_cases(cuda, normals):
    from occlusionfusion_amd.association import pack_transforms
    x, n, a, w, valid = _hand_cases()
    nodes, R, T = np.zeros((1, 3), F32), np.eye(3, dtype=F32)[None], np.zeros((1, 3), F32)
    d = _dev(cuda, pts=x, nrm=n, anchors=a, weights=w, valid=valid)
    d["packed"] = pack_transforms(nodes, R, T, cuda)
    ref = sp.splat(x, n if normals else None, a, w, valid, R, T, nodes, SMALL["intr"], 33, 33, 0.025, MARGIN)
    want = [0, 0, 0, 2, 2, 2, 3, 3, 0, 0, 1, 0, 4, 0, 0, 2]
    if not normals:
        want[6] = want[7] = 0                                # nothing is back-facing without normals
    assert ref["code"].tolist() == want
    h = _Handle(64, 33 * 33)
    out = _direct(h, d, SMALL["intr"], 33, 33, rho=0.025, normals=normals)
    _assert_equals_ref(out, ref, normals)
    idx = out[1].cpu().numpy()
    assert (idx == 8).sum() > 1 and not (idx == 9).any()     # identical points: the lower index owns the pixels
    assert (idx == 0).sum() == 81                            # the clamped footprint
    # P = 0 on the used handle: depth all 0, index all -1, nothing else touched
    depth, index, code, warped, wn = _direct(h, d, SMALL["intr"], 33, 33, rho=0.025, normals=normals, n=0)
    assert torch.all(depth == 0) and torch.all(index == -1) and code.numel() == 0
    # every output may be NULL: the others are written as before, a NULL one's buffer stays as it was filled
    fill = {"d": 7.0, "i": 77, "c": 99, "k": 7.0, "n": 7.0}
    for keep in ("", "dik", "cn"):
        got = _direct(h, d, SMALL["intr"], 33, 33, rho=0.025, normals=normals, outputs=keep)
        for c, g, r in zip("dickn", got, out):
            if c in keep and (c != "n" or normals):
                assert np.array_equal(_bits(g.cpu().numpy()), _bits(r.cpu().numpy())), (keep, c)
            else:
                assert torch.all(g == fill[c]), (keep, c)


# ------------------------------------------------------------------------------------------------ determinism
def test_determinism_across_calls_handles_and_image_sizes(two):
    d, intr, H, W = two["dev"], two["intr"], two["H"], two["W"]
    P = two["points"].shape[0]
    h1, h2 = _Handle(P, H * W), _Handle(P + 1000, 2 * H * W)
    a = _direct(h1, d, intr, H, W)
    half = tuple(0.5 * v for v in intr)
    s1 = _direct(h1, d, half, H // 2, W // 2)               # the same handle at 80 x 56 ...
    b = _direct(h1, d, intr, H, W)                          # ... and back at 160 x 112
    c = _direct(h2, d, intr, H, W)
    s2 = _direct(_Handle(P, (H // 2) * (W // 2)), d, half, H // 2, W // 2)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           z.view(torch.int32) if z.dtype == torch.float32 else z)
    for x, y in zip(s1, s2):
        assert torch.equal(x, y)
    assert int((s1[0] > 0).sum()) > 0
    ref = sp.splat(two["points"], two["normals"], two["anchors_bad"], two["weights"], two["valid"], two["R"], two["T"],
                   two["nodes"], half, H // 2, W // 2, RHO, MARGIN)
    _assert_equals_ref(s1, ref)


def test_permutation_on_the_device(cuda):
    from occlusionfusion_amd.association import pack_transforms
    x, n, ok = sp.random_cloud()
    P = x.shape[0]
    a = np.zeros((P, 4), np.int32)
    w = np.tile(np.array([1, 0, 0, 0], F32), (P, 1))
    packed = pack_transforms(np.zeros((1, 3), F32), None, None, cuda)
    h = _Handle(P, 33 * 33)

    def run(order):
        d = _dev(cuda, pts=x[order], nrm=n[order], anchors=a, weights=w, valid=ok[order].astype(np.uint8))
        d["packed"] = packed
        return [t.cpu().numpy() for t in _direct(h, d, SMALL["intr"], 33, 33, rho=0.012)]

    ident = np.arange(P)
    depth, index, code, _, _ = run(ident)
    ref = sp.splat(x, n, a, w, ok, np.eye(3, dtype=F32)[None], np.zeros((1, 3), F32), np.zeros((1, 3), F32),
                   SMALL["intr"], 33, 33, 0.012, MARGIN)      # (the device normalises the cloud's f32 normals again)
    assert np.array_equal(_bits(depth), _bits(ref["depth"])) and np.array_equal(index, ref["index"])
    assert np.array_equal(code, ref["code"]) and np.bincount(code, minlength=5).min() > 0
    _, irev, _, _, _ = run(ident[::-1].copy())
    tied = np.where(irev >= 0, P - 1 - irev, -1) != index
    assert 0 < tied.sum() < 0.5 * (index >= 0).sum()
    perm = np.random.default_rng(7).permutation(P)
    d2, i2, c2, _, _ = run(perm)
    assert np.array_equal(_bits(d2), _bits(depth))
    assert np.array_equal(c2, code[perm])
    back = np.where(i2 >= 0, perm[np.maximum(i2, 0)], -1)
    assert np.array_equal(back[~tied], index[~tied])


# ------------------------------------------------------------------------------------------------ operator, arguments
def test_op_equals_c_abi_and_opcheck(two, cuda):
    d, intr, H, W = two["dev"], two["intr"], two["H"], two["W"]
    P = two["points"].shape[0]
    h = _Handle(P, H * W)
    st = torch.zeros(1, dtype=torch.int32, device=cuda)
    for normals in (True, False):
        ref = _direct(h, d, intr, H, W, normals=normals)
        out = torch.ops.ofx.splat_points(st, h.h.value, d["pts"], d["nrm"] if normals else None, d["anchors"],
                                         d["weights"], d["valid"].bool(), d["packed"], list(intr), H, W, RHO, MARGIN)
        assert len(out) == 5 and out[4].shape == ((P, 3) if normals else (0, 3))
        for x, y in list(zip(out, ref))[:4 + int(normals)]:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    small = (st, h.h.value, d["pts"][-300:].contiguous(), d["nrm"][-300:].contiguous(), d["anchors"][-300:].contiguous(),
             d["weights"][-300:].contiguous(), d["valid"][-300:].bool(), d["packed"], list(intr), H, W, RHO, MARGIN)
    torch.library.opcheck(torch.ops.ofx.splat_points.default, small)


def test_refused_arguments(two, cuda):
    d, intr, H, W = two["dev"], two["intr"], two["H"], two["W"]
    h = _Handle(100, H * W)
    with pytest.raises(_lib.OfxError, match="max_points"):
        _direct(h, d, intr, H, W, n=101)
    with pytest.raises(_lib.OfxError, match="max_pixels"):
        _direct(_Handle(100, H * W - 1), d, intr, H, W, n=100)
    with pytest.raises(_lib.OfxError, match="splat_radius"):
        _direct(h, d, intr, H, W, n=100, rho=-1.0)
    with pytest.raises(_lib.OfxError, match="splat_radius"):
        _direct(h, d, intr, H, W, n=100, rho=float("nan"))
    with pytest.raises(_lib.OfxError, match="occl_margin"):
        _direct(h, d, intr, H, W, n=100, margin=float("nan"))
    cam, prm = _lib.Camera(*intr, W, H), _lib.SplatParams(RHO, MARGIN)
    wn = torch.empty((100, 3), device=cuda)
    st = _lib.lib.ofx_splat_points(h.h, ptr(d["pts"]), None, ptr(d["anchors"]), ptr(d["weights"]), None, 100,
                                   ptr(d["packed"]), d["packed"].shape[0], byref(cam), byref(prm), None, None, None, None,
                                   ptr(wn), stream_ptr())
    assert st == -1 and b"warped_normals without normals" in _lib.lib.ofx_last_error()
    mis = torch.zeros(4 * 101 + 1, dtype=torch.int32, device=cuda)[1:]     # 4 bytes off a 16-byte boundary
    st = _lib.lib.ofx_splat_points(h.h, ptr(d["pts"]), None, ptr(mis), ptr(d["weights"]), None, 100, ptr(d["packed"]),
                                   d["packed"].shape[0], byref(cam), byref(prm), None, None, None, None, None,
                                   stream_ptr())
    assert st == -1 and b"16-byte aligned" in _lib.lib.ofx_last_error()
    from occlusionfusion_amd.association import ModelRenderer
    r = ModelRenderer(100, 50 * 50, cuda)
    args = (d["pts"][:100], None, d["anchors"][:100], d["weights"][:100], None, d["packed"], intr)
    with pytest.raises(ValueError, match="pixels exceed"):
        r.render(*args, H, W, RHO)
    with pytest.raises(ValueError, match="points exceed"):
        r.render(d["pts"][:101], None, d["anchors"][:101], d["weights"][:101], None, d["packed"], intr, 50, 50, RHO)
    with pytest.raises(ValueError, match="normal_map"):
        r.render(*args, 50, 50, RHO, normal_map=True)


def test_renderer_returns_the_normal_map(two, cuda):
    from occlusionfusion_amd.association import ModelRenderer
    d, intr, H, W = two["dev"], two["intr"], two["H"], two["W"]
    P = two["points"].shape[0]
    out = ModelRenderer(P, H * W, cuda).render(d["pts"], d["nrm"], d["anchors"], d["weights"], d["valid"], d["packed"],
                                               intr, H, W, RHO, MARGIN, normal_map=True)
    ref = two["ref"][True]
    assert np.array_equal(_bits(out["depth"].cpu().numpy()), _bits(ref["depth"]))
    assert np.array_equal(out["visible"].cpu().numpy(), (ref["code"] == 0).astype(np.uint8))
    want = np.where((ref["index"] >= 0)[..., None], ref["warped_normals"][np.maximum(ref["index"], 0)], 0)
    assert out["normals"].shape == (3, H, W)
    assert np.array_equal(_bits(out["normals"].permute(1, 2, 0).contiguous().cpu().numpy()), _bits(want.astype(F32)))


# ------------------------------------------------------------------------------------------------ tracking
def test_occlusion_gate_keeps_the_hidden_layer_in_place(cuda):
    """icp_track on the two-layer scene from the identity, three iterations, the exact direct solve. Without the gate the
    nine hidden rear nodes end on the front patch (>= 2 cm); with it they stay (<= 1 mm) and no hidden point is among the
    emitted matches of any iteration. occlusion=False gives the same bytes before and after a renderer exists."""
    from occlusionfusion_amd.association import ModelRenderer, ProjectiveAssociator, icp_track
    from occlusionfusion_amd.registration import GaussNewtonSolver
    sc = sp.two_layer_scene()
    P, N = sc["points"].shape[0], sc["nodes"].shape[0]
    solver = GaussNewtonSolver(N, 10000, cuda, precond="direct")
    assoc = ProjectiveAssociator(P, cuda)
    emitted = []
    inner = assoc.associate

    def recording(*a, **k):
        m = inner(*a, **k)
        emitted.append(m["match_idx"].clone())
        return m
    assoc.associate = recording

    def run(**kw):
        emitted.clear()
        out, log, _ = icp_track(assoc, solver, sc["nodes"], sc["edges"], sc["edge_weights"], sc["points"],
                                sc["normals"], sc["anchors"], sc["weights"], None, sc["depth"], sc["intr"], icp_iters=3,
                                **kw)
        assert out["valid_solve"] == 1
        return out, [m.cpu().numpy() for m in emitted]

    before, m_before = run()
    renderer = ModelRenderer(P, sc["H"] * sc["W"], cuda)
    after, _ = run(occlusion=False, renderer=renderer, splat_radius=RHO)
    for k in ("node_rotations", "node_translations"):
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32))
    assert "render" not in after
    gated, m_gated = run(occlusion=True, renderer=renderer, splat_radius=RHO, occl_margin=MARGIN)
    hn, hidden = sc["hidden_nodes"], sc["hidden"]
    t_un = np.linalg.norm(before["node_translations"].cpu().numpy()[hn], axis=1)
    t_g = np.linalg.norm(gated["node_translations"].cpu().numpy()[hn], axis=1)
    print("hidden nodes |T|: ungated", t_un.min(), t_un.max(), "gated", t_g.max(), "hidden points matched: ungated",
          [int(hidden[m].sum()) for m in m_before], "gated", [int(hidden[m].sum()) for m in m_gated])
    assert t_un.min() >= 0.02
    assert t_g.max() <= 1e-3
    assert len(m_gated) == 3 and all(not hidden[m].any() for m in m_gated)
    assert any(hidden[m].any() for m in m_before)
    code = gated["render"]["code"].cpu().numpy()
    assert np.all(code[hidden] == 4) and (code[~hidden] == 4).sum() <= 0.05 * (~hidden).sum()
    with pytest.raises(ValueError, match="ModelRenderer"):
        run(occlusion=True, splat_radius=RHO)
    with pytest.raises(ValueError, match="splat_radius"):
        run(occlusion=True, renderer=renderer)


# ------------------------------------------------------------------------------------------------ pipeline
def _pipeline(cuda, seq):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"))
    pipe.integrate_source(pipe.prepare(0))
    return pipe


def test_pipeline_tracks_with_the_gate_and_renders_the_live_model(cuda):
    """Config 1, three frames of track_step(model="volume") with and without occlusion=True: every solve valid, every
    association emits (and accepts) at least 0.75 of what the ungated run does. Then render_live(): the live depth image
    covers at least 0.9 of the last frame's pixels whose surface lies inside the volume, and agrees with the frame's
    depth within test_splat_ref's bounds (share beyond 2 cm <= 0.02, mean <= 5 mm)."""
    from occlusionfusion_amd import synthetic as S
    seq = S.config_sequence(1, device=cuda)
    c = S.BASELINE_CONFIGS[1]
    pipes = {occ: _pipeline(cuda, seq) for occ in (False, True)}
    outs = {occ: [p.track_step(p.prepare(t), t, model="volume", max_model_points=16384, occlusion=occ)
                  for t in (1, 2, 3)] for occ, p in pipes.items()}
    for occ in (False, True):
        assert all(o["valid_solve"] == 1 for o in outs[occ])
        assert all(("render" in o) == occ for o in outs[occ])
    em = {occ: [[x["emitted"] for x in o["assoc"]] for o in outs[occ]] for occ in outs}
    acc = {occ: [[x["accepted"] for x in o["assoc"]] for o in outs[occ]] for occ in outs}
    occluded = [int((o["render"]["code"] == 4).sum()) for o in outs[True]]
    print("emitted without the gate", em[False], "with it", em[True], "accepted without", acc[False], "with",
          acc[True], "occluded model points in the last render of each frame", occluded)
    for g, u in zip(sum(em[True], []) + sum(acc[True], []), sum(em[False], []) + sum(acc[False], [])):
        assert g >= 0.75 * u                                  # (emitted is capped by max_matches: accepted as well)
    pipe = pipes[True]
    assert pipe._renderer.max_points == 16384
    live = pipe.wf.render_live(max_points=16384)
    H, W = seq.cam.height, seq.cam.width
    assert live["depth"].shape == (H, W) and live["normals"].shape == (3, H, W) and live["index"].shape == (H, W)
    assert live["index"].dtype == torch.int32 and live["code"].shape == (16384,)
    depth, index = live["depth"].cpu().numpy(), live["index"].cpu().numpy()
    nrm = live["normals"].cpu().numpy()
    cov = depth > 0
    assert np.array_equal(cov, index >= 0)
    ln = np.linalg.norm(nrm, axis=0)
    assert np.all(ln[~cov] == 0) and np.abs(ln[cov] - 1).max() < 1e-5
    d3 = seq.frame(3)[5]
    # the frame's pixels whose surface lies inside the volume (its box without the boundary layer, which carries no model)
    seen = d3 > 0
    vm = fo.backproject_depth(d3, *pipe.intr)
    lo = np.asarray(c["origin"], np.float64) + c["voxel"]
    hi = np.asarray(c["origin"], np.float64) + (c["dims"] - 2) * c["voxel"]
    box = seen & np.all((vm >= lo[:, None, None]) & (vm <= hi[:, None, None]), axis=0)
    coverage = float((cov & box).sum() / box.sum())
    both = cov & seen
    err = np.abs(depth[both].astype(np.float64) - d3[both])
    print(f"render_live: {int(cov.sum())} covered pixels, {coverage:.4f} of the frame's {int(box.sum())} pixels inside the "
          f"volume; share > 2 cm {float((err > 0.02).mean()):.4f}, mean |dz| {err.mean() * 1e3:.2f} mm")
    assert box.sum() > 10000 and coverage >= 0.9
    assert (err > 0.02).mean() <= 0.02 and err.mean() <= 0.005
