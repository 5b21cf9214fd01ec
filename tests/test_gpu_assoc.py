"""GPU: projective data association (ofx_associate, torch.ops.ofx.associate, ProjectiveAssociator, Registration.track).

* the kernel and its compaction equal the numpy restatement (tests/assoc_ref.py) bit for bit — both modes, with and
  without normals, max_matches above / at / below the accepted count, P = 8229 (two full 4096-flag scan tiles + 37), 1, 0;
* `warped` is ofx_deform_points' output bit for bit, and the pixel is ofx_visibility_f32's;
* the operator equals the direct C-ABI call and passes opcheck; two calls and two handles agree;
* Registration.track follows a depth frame 20 frames away without given matches, to within a quarter of the gap the
  ground-truth-match solve closes; an empty depth frame raises before any solve.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 32, 40
INTR = (30.0, 30.0, 19.5, 15.5)
P_FULL = 2 * 4096 + 37
PRM = dict(dist_max=0.05, cos_min=0.2, edge_max=0.03)
COVERAGE = 0.3


def _rot(axis_angle):
    return fo.angle_axis_to_rotation_matrix(axis_angle).astype(np.float32)


def _scene():
    """40x32 depth image (a tilted, gently curved surface with a block of holes and a 5 cm step), 24 nodes on it with
    rotations of a few degrees and translations of a few mm, 8229 points near the surface."""
    rng = np.random.default_rng(2024)
    fx, fy, cx, cy = INTR
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    depth = 1.0 + 0.004 * (u - cx) + 0.02 * np.sin(0.3 * v)
    depth[:, 28:] += 0.05
    depth[12:17, 8:13] = 0.0
    depth = depth.astype(np.float32)
    gu, gv = np.meshgrid(np.linspace(3, W - 4, 6), np.linspace(3, H - 4, 4))
    gz = 1.0 + 0.004 * (gu - cx) + 0.02 * np.sin(0.3 * gv)
    nodes = np.stack([(gu - cx) * gz / fx, (gv - cy) * gz / fy, gz], -1).reshape(-1, 3).astype(np.float32)
    N = nodes.shape[0]
    assert N == 24
    R = _rot(rng.normal(0, 0.02, (N, 3)))
    T = rng.normal(0, 0.004, (N, 3)).astype(np.float32)
    pu, pv = rng.uniform(-2.5, W + 1.5, P_FULL), rng.uniform(-2.5, H + 1.5, P_FULL)   # some leave the image
    pz = 1.0 + 0.004 * (pu - cx) + 0.02 * np.sin(0.3 * pv) + np.where(pu >= 27.5, 0.05, 0.0) + rng.normal(0, 0.02, P_FULL)
    pts = np.stack([(pu - cx) * pz / fx, (pv - cy) * pz / fy, pz], 1).astype(np.float32)
    nrm = rng.normal(size=(P_FULL, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return dict(depth=depth, nodes=nodes, R=R, T=T, pts=pts, nrm=nrm, rng_seed=7)


@pytest.fixture(scope="module")
def scene(cuda):
    s = _scene()
    dev = {k: torch.from_numpy(s[k]).to(cuda) for k in ("depth", "nodes", "R", "T", "pts", "nrm")}
    a, w, v = torch.ops.ofx.skin_points(dev["pts"], dev["nodes"], COVERAGE, 4)
    rng = np.random.default_rng(s["rng_seed"])
    v = v.cpu().numpy()
    v[rng.random(P_FULL) < 0.05] = False                     # some rows marked invalid
    pts = s["pts"].copy()
    behind = rng.random(P_FULL) < 0.03
    pts[behind, 2] = -pts[behind, 2]                          # some points pushed behind the camera (skin kept)
    s["pts"], dev["pts"] = pts, torch.from_numpy(pts).to(cuda)
    s["anchors"], s["weights"], s["valid"] = a.cpu().numpy(), w.cpu().numpy(), v.astype(np.uint8)
    dev["anchors"], dev["weights"], dev["valid"] = a, w, torch.from_numpy(s["valid"]).to(cuda)
    from occlusionfusion_amd.association import pack_transforms
    from occlusionfusion_amd.image_proc import backproject_depth_device
    dev["packed"] = pack_transforms(dev["nodes"], dev["R"], dev["T"], cuda)
    dev["vmap"] = backproject_depth_device(dev["depth"], *INTR)
    s["vmap"] = fo.backproject_depth(s["depth"], *INTR)
    assert np.array_equal(dev["vmap"].cpu().numpy(), s["vmap"])
    s["dev"] = dev
    s["ref"] = {}
    return s


def _ref(s, mode, normals, max_matches, n=None, valid=True):
    """The restatement's outputs, its gate computed once per (mode, normals, n, valid) and shared (never modified)."""
    key = (mode, normals, n, valid)
    if key not in s["ref"]:
        sl = slice(0, n)
        s["ref"][key] = ar.gate(s["pts"][sl], s["nrm"][sl] if normals else None, s["anchors"][sl], s["weights"][sl],
                                s["valid"][sl] if valid else None, s["R"], s["T"], s["nodes"], INTR, s["vmap"],
                                mode=mode, **PRM)
    code, tgt, warped = s["ref"][key]
    acc = np.nonzero(code == 0)[0]
    idx = acc[ar.emitted_ranks(acc.shape[0], max_matches)].astype(np.int32)
    sl = slice(0, n)
    return {"code": code, "tgt": tgt, "warped": warped, "match_idx": idx, "src": s["pts"][sl][idx], "tgt_out": tgt[idx],
            "anchors": s["anchors"][sl][idx], "weights": s["weights"][sl][idx],
            "count": np.array([acc.shape[0], idx.shape[0]], np.int32)}


class _Handle:
    def __init__(self, max_points):
        self.h = _lib.c_void_p()
        call("ofx_assoc_create", max_points, byref(self.h))

    def __del__(self):
        _lib.lib.ofx_assoc_destroy(self.h)


def _direct(handle, d, mode, normals, max_matches, n=None, fill=0, valid=True):
    """ofx_associate through ctypes on the first n points (valid=False: a NULL valid); compacted buffers prefilled with
    `fill`."""
    dev = d["pts"].device
    n = d["pts"].shape[0] if n is None else n
    M = max_matches
    code = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    tgt, warped = torch.full((n, 3), 7.0, device=dev), torch.full((n, 3), 7.0, device=dev)
    midx = torch.full((M,), fill, dtype=torch.int32, device=dev)
    src_o, tgt_o = torch.full((M, 3), float(fill), device=dev), torch.full((M, 3), float(fill), device=dev)
    a_o = torch.full((M, 4), fill, dtype=torch.int32, device=dev)
    w_o = torch.full((M, 4), float(fill), device=dev)
    count = torch.full((2,), -1, dtype=torch.int32, device=dev)
    cam = _lib.Camera(*INTR, W, H)
    prm = _lib.AssocParams(PRM["dist_max"], PRM["cos_min"], PRM["edge_max"], mode, M, 0)
    call("ofx_associate", handle.h, ptr(d["pts"]), ptr(d["nrm"]) if normals else None, ptr(d["anchors"]),
         ptr(d["weights"]), ptr(d["valid"]) if valid else None, n, ptr(d["packed"]), d["packed"].shape[0], byref(cam),
         ptr(d["vmap"]), H, W,
         byref(prm), ptr(code), ptr(tgt), ptr(warped), ptr(midx), ptr(src_o), ptr(tgt_o), ptr(a_o), ptr(w_o), ptr(count),
         stream_ptr())
    return code, tgt, warped, midx, src_o, tgt_o, a_o, w_o, count


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_equals_ref(out, ref, fill=0):
    code, tgt, warped, midx, src_o, tgt_o, a_o, w_o, count = (t.cpu().numpy() for t in out)
    assert count.tolist() == ref["count"].tolist()
    assert np.array_equal(code, ref["code"])
    assert np.array_equal(_bits(tgt), _bits(ref["tgt"]))
    assert np.array_equal(_bits(warped), _bits(ref["warped"]))
    e = int(count[1])
    for got, want in ((midx, ref["match_idx"]), (src_o, ref["src"]), (tgt_o, ref["tgt_out"]), (a_o, ref["anchors"]),
                      (w_o, ref["weights"])):
        assert np.array_equal(_bits(got[:e]), _bits(want))
        assert np.all(got[e:] == fill)                      # rows past the emitted count are left untouched


def test_scene_reaches_every_code(scene):
    code = _ref(scene, ar.PLANE, True, 10)["code"]
    hist = np.bincount(code, minlength=7)
    print("codes 0..6:", hist.tolist())
    assert np.all(hist > 0) and hist[0] > 1000
    assert np.bincount(_ref(scene, ar.POINT, False, 10)["code"], minlength=7)[6] == 0


# every (mode, normals, mm) with valid given, and valid = NULL (the kernels' VALID = false) in plane mode, thinned
_KERNEL_CASES = [pytest.param(mode, normals, mm, True, id=f"{mode}-{normals}-{mm}") for mm in ("above", "exact", "below")
                 for normals in (True, False) for mode in (ar.POINT, ar.PLANE)]
_KERNEL_CASES += [pytest.param(ar.PLANE, normals, "below", False, id=f"{ar.PLANE}-{normals}-below-NULL")
                  for normals in (True, False)]


@pytest.mark.parametrize("mode,normals,mm,valid", _KERNEL_CASES)
def test_kernel_equals_restatement(scene, mode, normals, mm, valid):
    n_acc = int(_ref(scene, mode, normals, 0, valid=valid)["count"][0])
    assert n_acc > 1000
    M = {"above": n_acc + 5, "exact": n_acc, "below": 1000}[mm]
    ref = _ref(scene, mode, normals, M, valid=valid)
    assert ref["count"].tolist() == [n_acc, min(n_acc, M)]
    assert valid or (ref["code"] == 1).sum() < (scene["valid"] == 0).sum()   # the rows marked invalid are gated now
    out = _direct(_Handle(P_FULL), scene["dev"], mode, normals, M, fill=-3, valid=valid)
    _assert_equals_ref(out, ref, fill=-3)


@pytest.mark.parametrize("n", [1, 0, 257, 4096, 4097])
def test_small_and_tile_edge_sizes(scene, n):
    """P = 1 and P = 0 (count [0, 0], nothing touched), one full workgroup and a lone thread in the next, and one full
    scan tile with and without a ragged flag."""
    h = _Handle(P_FULL)
    for M in (3, 5000):
        ref = _ref(scene, ar.PLANE, True, M, n=n)
        out = _direct(h, scene["dev"], ar.PLANE, True, M, n=n, fill=-3)
        _assert_equals_ref(out, ref, fill=-3)
    if n == 0:
        assert out[8].tolist() == [0, 0]
    with pytest.raises(_lib.OfxError):       # more points than the handle was sized for
        _direct(_Handle(8), scene["dev"], ar.PLANE, True, 10, n=9)


def test_warped_is_deform_points_and_pixel_is_visibility_f32(scene, cuda):
    d = scene["dev"]
    out = _direct(_Handle(P_FULL), d, ar.POINT, True, 10)
    code, tgt, warped = out[0], out[1], out[2]
    assert torch.equal(warped, torch.ops.ofx.deform_points(d["pts"], d["anchors"], d["weights"], d["valid"].bool(),
                                                           d["packed"], False))
    # ofx_visibility_f32 on the warped points: depth_diff = f64(depth at its pixel, 0 off the image) - z. Codes 2 and 3
    # are exactly the points it finds no depth for; an accepted point's target (point mode) is that pixel's vertex.
    vis = torch.empty(P_FULL, dtype=torch.uint8, device=cuda)
    dd = torch.empty(P_FULL, dtype=torch.float64, device=cuda)
    cam = _lib.Camera(*INTR, W, H)
    call("ofx_visibility_f32", ptr(warped), P_FULL, byref(cam), ptr(d["depth"]), 0.1, ptr(vis), ptr(dd), stream_ptr())
    z = warped[:, 2].double()
    live = code != 1
    assert torch.equal((dd == -z) & live, ((code == 2) | (code == 3)) & live)
    acc = code == 0
    assert torch.equal(dd[acc], tgt[acc, 2].double() - z[acc])


def test_op_equals_c_abi_and_opcheck(scene, cuda):
    d = scene["dev"]
    h = _Handle(P_FULL)
    st = torch.zeros(1, dtype=torch.int32, device=cuda)
    for mode, normals, M in ((ar.PLANE, True, 1000), (ar.POINT, False, 9000)):
        ref = _direct(h, d, mode, normals, M, fill=0)
        args = (st, h.h.value, d["pts"], d["nrm"] if normals else None, d["anchors"], d["weights"], d["valid"].bool(),
                d["packed"], d["vmap"], list(INTR), PRM["dist_max"], PRM["cos_min"], PRM["edge_max"], mode, M)
        out = torch.ops.ofx.associate(*args)
        assert len(out) == 9
        for x, y in zip(out, ref):
            assert x.dtype == y.dtype and torch.equal(x, y)
    small = (st, h.h.value, d["pts"][:300], d["nrm"][:300], d["anchors"][:300], d["weights"][:300],
             d["valid"][:300].bool(), d["packed"], d["vmap"], list(INTR), 0.05, 0.2, 0.03, 1, 50)
    torch.library.opcheck(torch.ops.ofx.associate.default, small)


def test_determinism_across_calls_and_handles(scene):
    d = scene["dev"]
    h1, h2 = _Handle(P_FULL), _Handle(P_FULL + 1000)
    a = _direct(h1, d, ar.PLANE, True, 1000)
    _direct(h1, d, ar.POINT, False, 77, n=5000)            # other work on the handle in between
    b = _direct(h1, d, ar.PLANE, True, 1000)
    c = _direct(h2, d, ar.PLANE, True, 1000)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_associator_slices_to_the_count(scene, cuda):
    from occlusionfusion_amd.association import ProjectiveAssociator
    d = scene["dev"]
    pa = ProjectiveAssociator(P_FULL, cuda)
    m = pa.associate(d["pts"], d["nrm"], d["anchors"], d["weights"], d["valid"], d["packed"], d["vmap"], INTR,
                     mode="plane", max_matches=1000, **PRM)
    ref = _ref(scene, ar.PLANE, True, 1000)
    assert (m["accepted"], m["emitted"]) == tuple(ref["count"].tolist()) and m["emitted"] == 1000
    assert m["histogram"] == np.bincount(ref["code"], minlength=7).tolist()
    for k, r in (("match_idx", "match_idx"), ("src", "src"), ("tgt", "tgt_out"), ("anchors", "anchors"),
                 ("weights", "weights")):
        assert m[k].shape[0] == 1000 and np.array_equal(_bits(m[k].cpu().numpy()), _bits(ref[r]))


# ------------------------------------------------------------------------------------------------ tracking end to end
@pytest.fixture(scope="module")
def tracker(cuda):
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
    pts = cp[np.sort(np.random.default_rng(5).choice(cp.shape[0], P_FULL, replace=False))]
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(pts, graph, wf, K, precond="direct")
    return seq, reg, intr


def test_tracking_follows_a_depth_frame_without_matches(tracker, cuda):
    """Config 1 (199 nodes, 320x224, exact direct solve), frame 0 -> frame 20 from the identity, 3 ICP iterations, plane
    mode, no motion data. Residual: mean |depth at the pixel - z| of the warped canonical points (assoc_ref.
    depth_residual). The yardstick is one optimize on the ground-truth matches (seq.solver_inputs(20, 3000), confidence
    0): tracking must close at least three quarters of the gap it closes, with every association accepting at least
    0.8 of the points. The 3-D error against the ground-truth motion is deliberately not asserted: geometry-only
    association leaves tangential motion on a sphere undetermined."""
    seq, reg, intr = tracker
    t = 20
    frame = seq.frame(t)
    depth = frame[5]
    src_pcd = reg.source_pcd
    n_pts = src_pcd.shape[0]
    r_id = ar.depth_residual(src_pcd.cpu().numpy(), depth, intr)
    # ground-truth-match solve
    src, tgt, tpos, _ = seq.solver_inputs(t, 3000)
    a, w, v = reg.warpfield.skin_device(src)
    src_t, tgt_t = torch.from_numpy(src).to(cuda)[v], torch.from_numpy(tgt).to(cuda)[v]
    gt = reg.solver.optimize(seq.nodes, seq.edges, seq.edge_weights, tpos, np.zeros(len(seq.nodes), np.float32), src_t,
                             a[v], w[v], tgt_t, intr)
    assert gt["valid_solve"] == 1
    reg.warpfield.set_node_transforms(gt["node_rotations"], gt["node_translations"])
    r_gt = ar.depth_residual(reg.warpfield.deform_device(src_pcd, reg.point_anchors, reg.anchor_weight).cpu().numpy(),
                             depth, intr)
    # tracking
    assert reg.prev_rot is None and reg.prev_trans is None
    out = reg.track({"im": frame, "id": t}, icp_iters=3, mode="plane")
    r_icp = ar.depth_residual(out["warped_verts"].cpu().numpy(), depth, intr)
    shares = [x["accepted"] / n_pts for x in out["assoc"]]
    print(f"tracking frame {t}: r_id = {1e3 * r_id:.3f} mm, r_gt = {1e3 * r_gt:.3f} mm, r_icp = {1e3 * r_icp:.3f} mm, "
          f"accepted shares = {[round(x, 4) for x in shares]}, emitted = {[x['emitted'] for x in out['assoc']]}, "
          f"histograms = {[x['histogram'] for x in out['assoc']]}")
    assert out["valid_solve"] == 1
    assert len(out["assoc"]) == 3 and out["target_frame_id"] == t
    assert all(sum(x["histogram"]) == n_pts and x["histogram"][0] == x["accepted"] for x in out["assoc"])
    assert min(shares) >= 0.8, shares
    assert r_gt < r_id
    assert r_icp <= r_gt + 0.25 * (r_id - r_gt), (r_id, r_gt, r_icp)
    assert reg.tgt_pcd.shape == (int((depth > 0).sum()), 3) and reg.prev_rot is not None


def test_too_few_matches_raises_before_any_solve(tracker, monkeypatch):
    from occlusionfusion_amd.association import TooFewMatches
    seq, reg, _ = tracker
    calls = []
    monkeypatch.setattr(reg.solver, "optimize", lambda *a, **k: calls.append(1))
    empty = np.zeros((6, seq.cam.height, seq.cam.width), np.float32)
    with pytest.raises(TooFewMatches, match="at least 16"):
        reg.track({"im": empty}, icp_iters=3)
    assert not calls
