"""GPU: the photometric correspondence search (ofx_photo_associate, torch.ops.ofx.photo_associate, ProjectiveAssociator.
associate_photo, the photo= keyword of the tracking layers).

* the kernel and its compaction equal the numpy restatement (tests/photo_ref.py) byte for byte on the 40x32 case: radius
  0 / 1 / 4 / 8, normals and valid given and NULL, n_points of 0, 1, 3, 63, 64, 65 and 257 (partial lane groups, partial
  waves, more than one workgroup); two calls and two handles agree; radius 0 equals torch.ops.ofx.associate in point
  mode; the operator equals the direct C-ABI call and passes opcheck;
* tracking a spinning sphere — motion that depth alone cannot see — closes at least three quarters of the gap between
  the geometric tracker and a solve on ground-truth matches;
* on the breathing scene photo=True does not harm the depth residual;
* FusionPipeline.track_step(model="volume", photo=True) runs over textured frames, and the volume's colours are the
  texture's.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import photo_ref as pr  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 32, 40
INTR = (30.0, 30.0, 19.5, 15.5)
EDGE = 0.03
P_CASE = 300
PRM = dict(dist_max=0.15, cos_min=0.7, color_max=0.15, geo_weight=1.0)
SIZES = (0, 1, 3, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def case(cuda):
    from occlusionfusion_amd.association import pack_transforms
    from occlusionfusion_amd.image_proc import prepare_depth_device
    c = pr.small_case(P_CASE)
    d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(cuda)
         for k in ("points", "normals", "colors", "anchors", "weights", "valid", "color_image", "depth", "nodes",
                   "node_R", "node_T")}
    prep = prepare_depth_device(d["depth"], *INTR, radius=0, edge_max=EDGE, normals=True)
    d["point_image"], d["normal_image"] = prep["point_image"], prep["normals"]
    assert np.array_equal(d["point_image"].cpu().numpy(), c["point_image"])
    c["normal_image"] = d["normal_image"].cpu().numpy()     # the device's own map (prepare_ref pins it elsewhere)
    d["packed"] = pack_transforms(d["nodes"], d["node_R"], d["node_T"], cuda)
    c["dev"], c["ref"] = d, {}
    return c


def _ref(c, radius, normals, valid, n, M, **over):
    """The restatement's outputs; the search is computed once per case and shared (never modified)."""
    prm = dict(PRM, **over)
    key = (radius, normals, valid, n, tuple(sorted(prm.items())))
    if key not in c["ref"]:
        sl = slice(0, n)
        c["ref"][key] = pr.search(c["points"][sl], c["normals"][sl] if normals else None, c["colors"][sl],
                                  c["anchors"][sl], c["weights"][sl], c["valid"][sl] if valid else None, c["node_R"],
                                  c["node_T"], c["nodes"], INTR, c["point_image"], c["normal_image"], c["color_image"],
                                  radius=radius, **prm)
    out = dict(c["ref"][key])
    sl = slice(0, n)
    acc = np.nonzero(out["code"] == 0)[0]
    idx = acc[ar.emitted_ranks(acc.shape[0], M)].astype(np.int32)
    out.update(match_idx=idx, src=c["points"][sl][idx], tgt_out=out["tgt"][idx], anchors=c["anchors"][sl][idx],
               weights=c["weights"][sl][idx], pixel_out=out["pixel"][idx].astype(np.float32),
               count=np.array([acc.shape[0], idx.shape[0]], np.int32))
    return out


class _Handle:
    def __init__(self, max_points):
        self.h = _lib.c_void_p()
        call("ofx_assoc_create", max_points, byref(self.h))

    def __del__(self):
        _lib.lib.ofx_assoc_destroy(self.h)


def _direct(handle, d, radius, normals, valid, n, M, fill=0, **over):
    """ofx_photo_associate through ctypes on the first n points; every output prefilled."""
    prm = dict(PRM, **over)
    dev = d["points"].device
    f, i = torch.float32, torch.int32
    code = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    tgt, warped = torch.full((n, 3), 7.0, device=dev), torch.full((n, 3), 7.0, device=dev)
    pixel = torch.full((n, 2), 77, dtype=i, device=dev)
    cost = torch.full((n,), 7.0, device=dev)
    midx = torch.full((M,), fill, dtype=i, device=dev)
    src_o, tgt_o = torch.full((M, 3), float(fill), device=dev), torch.full((M, 3), float(fill), device=dev)
    a_o = torch.full((M, 4), fill, dtype=i, device=dev)
    w_o = torch.full((M, 4), float(fill), device=dev)
    px_o = torch.full((M, 2), float(fill), dtype=f, device=dev)
    count = torch.full((2,), -1, dtype=i, device=dev)
    cam = _lib.Camera(*INTR, W, H)
    p = _lib.PhotoParams(prm["dist_max"], prm["cos_min"], prm["color_max"], prm["geo_weight"], radius, M)
    call("ofx_photo_associate", handle.h, ptr(d["points"]), ptr(d["normals"]) if normals else None, ptr(d["colors"]),
         ptr(d["anchors"]), ptr(d["weights"]), ptr(d["valid"]) if valid else None, n, ptr(d["packed"]),
         d["packed"].shape[0], byref(cam), ptr(d["point_image"]), ptr(d["normal_image"]), ptr(d["color_image"]), H, W,
         byref(p), ptr(code), ptr(tgt), ptr(warped), ptr(pixel), ptr(cost), ptr(midx), ptr(src_o), ptr(tgt_o), ptr(a_o),
         ptr(w_o), ptr(px_o), ptr(count), stream_ptr())
    return code, tgt, warped, pixel, cost, midx, src_o, tgt_o, a_o, w_o, px_o, count


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _assert_equals_ref(out, ref, fill=0):
    code, tgt, warped, pixel, cost, midx, src_o, tgt_o, a_o, w_o, px_o, count = (t.cpu().numpy() for t in out)
    assert count.tolist() == ref["count"].tolist()
    for got, want in ((code, "code"), (tgt, "tgt"), (warped, "warped"), (pixel, "pixel"), (cost, "cost")):
        assert np.array_equal(_bits(got), _bits(ref[want])), want
    e = int(count[1])
    for got, want in ((midx, "match_idx"), (src_o, "src"), (tgt_o, "tgt_out"), (a_o, "anchors"), (w_o, "weights"),
                      (px_o, "pixel_out")):
        assert np.array_equal(_bits(got[:e]), _bits(ref[want])), want
        assert np.all(got[e:] == fill), want                 # rows past the emitted count are left untouched


def test_case_reaches_every_code(case):
    seen = set()
    for r in (0, 4):
        seen |= set(_ref(case, r, True, True, P_CASE, 10)["code"].tolist())
    assert seen == set(range(8))


@pytest.mark.parametrize("valid", [True, False], ids=["valid", "validNULL"])
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "normalsNULL"])
@pytest.mark.parametrize("radius", [0, 1, 4, 8])
def test_kernel_equals_restatement(case, radius, normals, valid):
    h = _Handle(P_CASE)
    full = _ref(case, radius, normals, valid, P_CASE, 10000)
    n_acc = int(full["count"][0])
    assert n_acc > (20 if radius else 3)
    for M in (n_acc + 5, n_acc, max(n_acc // 3, 1)):          # above, at and below the accepted count
        ref = _ref(case, radius, normals, valid, P_CASE, M)
        _assert_equals_ref(_direct(h, case["dev"], radius, normals, valid, P_CASE, M, fill=-3), ref, fill=-3)


@pytest.mark.parametrize("n", SIZES)
def test_partial_groups_and_waves(case, n):
    h = _Handle(P_CASE)
    for radius, M in ((8, 5), (1, 400)):
        out = _direct(h, case["dev"], radius, True, True, n, M, fill=-3)
        _assert_equals_ref(out, _ref(case, radius, True, True, n, M), fill=-3)
    if n == 0:
        assert out[11].tolist() == [0, 0]
    with pytest.raises(_lib.OfxError, match="n_points"):      # more points than the handle was sized for
        _direct(_Handle(2), case["dev"], 1, True, True, 3, 10)


def test_geo_weight_and_colour_gate_variants(case):
    h = _Handle(P_CASE)
    for over in (dict(geo_weight=0.0), dict(geo_weight=10.0, color_max=float("inf")), dict(color_max=0.05)):
        out = _direct(h, case["dev"], 4, True, True, P_CASE, 100, fill=-3, **over)
        _assert_equals_ref(out, _ref(case, 4, True, True, P_CASE, 100, **over), fill=-3)


def test_determinism_across_calls_and_handles(case):
    d = case["dev"]
    h1, h2 = _Handle(P_CASE), _Handle(P_CASE + 1000)
    a = _direct(h1, d, 8, True, True, P_CASE, 40)
    _direct(h1, d, 1, False, False, 65, 7)                    # other work on the handle in between
    b = _direct(h1, d, 8, True, True, P_CASE, 40)
    c = _direct(h2, d, 8, True, True, P_CASE, 40)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8),
                                                                                      z.view(torch.uint8))


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "normalsNULL"])
def test_radius_0_is_associate_in_point_mode(case, cuda, normals):
    """radius 0, the colour gate off, any geo_weight: code, tgt, warped, count and every compacted array are
    torch.ops.ofx.associate's in point mode on the same vertex map, byte for byte (NaN colours taken out: they are the one
    thing associate cannot see)."""
    d = dict(case["dev"])
    d["colors"] = torch.nan_to_num(d["colors"], nan=0.5)
    d["color_image"] = torch.nan_to_num(d["color_image"], nan=0.5)
    h = _Handle(P_CASE)
    st = torch.zeros(1, dtype=torch.int32, device=cuda)
    for M in (50, 1000):
        got = _direct(h, d, 0, normals, True, P_CASE, M, color_max=float("inf"), geo_weight=3.0)
        want = torch.ops.ofx.associate(st, h.h.value, d["points"], d["normals"] if normals else None, d["anchors"],
                                       d["weights"], d["valid"].bool(), d["packed"], d["point_image"], list(INTR),
                                       PRM["dist_max"], PRM["cos_min"], EDGE, ar.POINT, M)
        assert int(want[8][0]) > 50
        code, tgt, warped, pixel, cost, midx, src_o, tgt_o, a_o, w_o, px_o, count = got
        for x, y in zip((code, tgt, warped, midx, src_o, tgt_o, a_o, w_o, count), want):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_op_equals_c_abi_and_opcheck(case, cuda):
    d = case["dev"]
    h = _Handle(P_CASE)
    st = torch.zeros(1, dtype=torch.int32, device=cuda)
    for radius, normals, M in ((4, True, 40), (8, False, 1000)):
        ref = _direct(h, d, radius, normals, True, P_CASE, M, fill=0)
        out = torch.ops.ofx.photo_associate(st, h.h.value, d["points"], d["normals"] if normals else None, d["colors"],
                                            d["anchors"], d["weights"], d["valid"].bool(), d["packed"], d["point_image"],
                                            d["normal_image"], d["color_image"], list(INTR), PRM["dist_max"],
                                            PRM["cos_min"], PRM["color_max"], PRM["geo_weight"], radius, M)
        assert len(out) == 12
        for x, y in zip(out, ref):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    sl = slice(10, 75)        # past the case's NaN point: opcheck compares outputs by value, and NaN != NaN
    small = (st, h.h.value, d["points"][sl], d["normals"][sl], d["colors"][sl], d["anchors"][sl], d["weights"][sl],
             d["valid"][sl].bool(), d["packed"], d["point_image"], d["normal_image"], d["color_image"], list(INTR),
             0.15, 0.7, 0.15, 1.0, 2, 20)
    torch.library.opcheck(torch.ops.ofx.photo_associate.default, small)


def test_associator_slices_to_the_count(case, cuda):
    from occlusionfusion_amd.association import PHOTO_CODE_NAMES, ProjectiveAssociator
    d = case["dev"]
    pa = ProjectiveAssociator(P_CASE, cuda)
    m = pa.associate_photo(d["points"], d["normals"], d["colors"], d["anchors"], d["weights"], d["valid"], d["packed"],
                           d["point_image"], d["normal_image"], d["color_image"], INTR, radius=4, max_matches=30, **PRM)
    ref = _ref(case, 4, True, True, P_CASE, 30)
    assert (m["accepted"], m["emitted"]) == tuple(ref["count"].tolist()) and m["emitted"] == 30
    assert len(PHOTO_CODE_NAMES) == 8 and m["histogram"] == np.bincount(ref["code"], minlength=8).tolist()
    for k, r in (("match_idx", "match_idx"), ("src", "src"), ("tgt", "tgt_out"), ("anchors", "anchors"),
                 ("weights", "weights"), ("pixel", "pixel_out"), ("pixel_all", "pixel"), ("cost", "cost")):
        assert np.array_equal(_bits(m[k].cpu().numpy()), _bits(ref[r])), k


# ------------------------------------------------------------------------------------------------ tracking end to end
N_MODEL = 2 * 4096 + 37
T_SPIN = 2          # frames 0 -> 2 of the spin scene: 3 degrees about the sphere's own centre


def _registration(cuda, scene, seed):
    """Config 1's volume and camera (128^3, 320x224) around `scene` on its depth-mesh graph, the exact direct solve, and
    N_MODEL of the canonical points with the textured source frame's colours at their own pixels."""
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.registration import Registration
    c = S.BASELINE_CONFIGS[1]
    cam = S.bench_camera(c["cam_scale"])
    seq = S.SyntheticSequence.build(c["nodes"], cam=cam, seed=seed, coverage=c["coverage"], scene=scene,
                                    graph="geodesic", device=cuda)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = c["dims"]
    vol = TSDFVolume.from_grid(c["origin"], c["voxel"], (D, D, D), intr, SimpleNamespace(source_frame=0, skip_rate=1),
                               device=cuda)
    graph = EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage)
    wf = WarpField(graph, vol)
    im0 = S.textured_frame(scene, cam, seed, 0)
    cp = seq.canonical_points                                   # the source depth's valid pixels, row-major
    col = im0[:3][:, im0[5] > 0].T
    assert col.shape == cp.shape
    sel = np.sort(np.random.default_rng(5).choice(cp.shape[0], N_MODEL, replace=False))
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(cp[sel], graph, wf, K, precond="direct")
    reg.update(cp[sel], colors=col[sel])
    assert reg.source_colors.shape == reg.source_pcd.shape
    return seq, reg, intr


def _reset(reg):
    reg.prev_rot = reg.prev_trans = None


def _gt_solve(seq, reg, intr, t, cuda):
    """One solve on 3000 ground-truth matches (confidence 0: no motion term), as test_gpu_assoc does -> the warped
    model points."""
    src, tgt, tpos, _ = seq.solver_inputs(t, 3000)
    a, w, v = reg.warpfield.skin_device(src)
    src_t, tgt_t = torch.from_numpy(src).to(cuda)[v], torch.from_numpy(tgt).to(cuda)[v]
    gt = reg.solver.optimize(seq.nodes, seq.edges, seq.edge_weights, tpos, np.zeros(len(seq.nodes), np.float32), src_t,
                             a[v], w[v], tgt_t, intr)
    assert gt["valid_solve"] == 1
    reg.warpfield.set_node_transforms(gt["node_rotations"], gt["node_translations"])
    return reg.warpfield.deform_device(reg.source_pcd, reg.point_anchors, reg.anchor_weight).cpu().numpy()


def test_tracking_follows_a_spin_that_depth_cannot_see(cuda):
    """SphereScene(motion="spin", occluder=False): the sphere spins 3 degrees about its own centre between frame 0 and
    frame 2, so the depth does not change at all. Tracked from the identity, 3 ICP iterations, no motion data. Error:
    the mean 3-D distance of the warped canonical sphere points to scene.deform_points, over the points whose outward
    normal makes more than about 107 degrees with the view ray (n.d < -0.3) both at frame 0 and at frame 2. e_id: the
    identity; e_geo: track(); e_gt: one solve on 3000 ground-truth matches; e_photo: track(photo=True). Geometry alone
    does not see the spin (e_geo >= 0.5 e_id, a condition on the scene); the photometric search must close three
    quarters of the gap between e_geo and e_gt, and match at least 0.8 of the front-facing points.
    Measured on the MI355X (2420 front-facing points of 8229): e_id 16.445 mm, e_geo 16.439 mm, e_gt 0.822 mm, e_photo
    1.064 mm against a bar of 4.726 mm, every front-facing point matched. The CPU restatement with the oracle's sparse
    GN (tools/photo_cpu_check.py, Euclidean graph) gave 16.445 / 16.461 / 0.668 / 1.184 mm, bar 4.617 mm."""
    from occlusionfusion_amd import synthetic as S
    scene = S.SphereScene(motion="spin", occluder=False)
    seq, reg, intr = _registration(cuda, scene, 1)
    t = T_SPIN
    frame = S.textured_frame(scene, seq.cam, 1, t)
    src = reg.source_pcd.cpu().numpy().astype(np.float64)
    gt = scene.deform_points(src, t)
    c = np.array(scene.center)

    def facing(p):
        n = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
        return (n * p).sum(1) / np.linalg.norm(p, axis=1) < -0.3
    sphere = (np.linalg.norm(src - c, axis=1) < scene.radius + 0.01) & (src[:, 2] < scene.plane_z - 0.02)
    front = sphere & facing(src) & facing(gt)
    assert front.sum() > 1000

    def err(w):
        return float(np.linalg.norm(np.asarray(w, np.float64) - gt, axis=1)[front].mean())
    e_id = err(src)
    e_gt = err(_gt_solve(seq, reg, intr, t, cuda))
    _reset(reg)
    geo = reg.track({"im": frame, "id": t}, icp_iters=3)
    e_geo = err(geo["warped_verts"].cpu().numpy())
    _reset(reg)
    out = reg.track({"im": frame, "id": t}, icp_iters=3, photo=True)
    e_photo = err(out["warped_verts"].cpu().numpy())
    code = reg._assoc.last["code"].cpu().numpy()
    share = float((code[front] == 0).mean())
    print(f"spin, frame 0 -> {t}: {int(front.sum())} front-facing points of {src.shape[0]}, e_id = {1e3 * e_id:.3f} mm, "
          f"e_geo = {1e3 * e_geo:.3f} mm, e_gt = {1e3 * e_gt:.3f} mm, e_photo = {1e3 * e_photo:.3f} mm, "
          f"bar = {1e3 * (e_gt + 0.25 * (e_geo - e_gt)):.3f} mm, matched share of the front-facing points = {share:.4f}, "
          f"histograms = {[x['histogram'] for x in out['assoc']]}")
    assert out["valid_solve"] == 1 and geo["valid_solve"] == 1
    assert all(len(x["histogram"]) == 8 for x in out["assoc"]) and all(len(x["histogram"]) == 7 for x in geo["assoc"])
    assert e_geo >= 0.5 * e_id, (e_id, e_geo)
    assert e_photo <= e_gt + 0.25 * (e_geo - e_gt), (e_id, e_geo, e_gt, e_photo)
    assert share >= 0.8, share


def test_photo_does_no_harm_on_the_breathing_scene(cuda):
    """Config 1's breathing scene with textured frames, frame 0 -> 20: the depth residual of test_gpu_assoc (mean |depth
    at the pixel - z| of the warped model points) under photo=True meets that test's own bound, r_gt + 0.25 (r_id -
    r_gt). Measured on the MI355X: r_id 9.249 mm, r_gt 1.602 mm, r_photo 2.173 mm (bound 3.514 mm)."""
    from occlusionfusion_amd import synthetic as S
    scene, seed = S.config_scene(1)
    seq, reg, intr = _registration(cuda, scene, seed)
    t = 20
    frame = S.textured_frame(scene, seq.cam, seed, t)
    depth = frame[5]
    r_id = ar.depth_residual(reg.source_pcd.cpu().numpy(), depth, intr)
    r_gt = ar.depth_residual(_gt_solve(seq, reg, intr, t, cuda), depth, intr)
    _reset(reg)
    out = reg.track({"im": frame, "id": t}, icp_iters=3, photo=True)
    r_photo = ar.depth_residual(out["warped_verts"].cpu().numpy(), depth, intr)
    print(f"breathing scene, frame {t}, photo=True: r_id = {1e3 * r_id:.3f} mm, r_gt = {1e3 * r_gt:.3f} mm, "
          f"r_photo = {1e3 * r_photo:.3f} mm, accepted = {[x['accepted'] for x in out['assoc']]}")
    assert out["valid_solve"] == 1 and r_gt < r_id
    assert r_photo <= r_gt + 0.25 * (r_id - r_gt), (r_id, r_gt, r_photo)


def test_pipeline_tracks_textured_frames_with_the_volume_model(cuda):
    """FusionPipeline.track_step(model="volume", photo=True) over three textured spin frames: every solve valid, every
    frame integrated and the model re-sampled. Before that, after the source frame alone: TSDFVolume.voxel_rgb of the
    sampled voxels is the texture where the integrate read it — surface_texture at the canonical point of the pixel that
    the voxel's centre projects to — within 1/255 (the source frame carries no colour noise here; the 8-bit image
    leaves half of that; measured 0.500/255). The distance to the texture at the sampled surface points themselves, a
    few mm away from that pixel's ray, is the texture's own variation over that offset (measured: mean 6.96/255, up to
    145/255 at the silhouette); it is printed, not asserted."""
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    scene = S.SphereScene(motion="spin", occluder=False)
    cam = S.bench_camera(c["cam_scale"])
    seq = S.SyntheticSequence.build(c["nodes"], cam=cam, seed=1, coverage=c["coverage"], scene=scene, graph="geodesic",
                                    device=cuda)
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"))

    def inputs(t, noise=0.01):
        fi = pipe.prepare(t)
        fi.im = torch.from_numpy(S.textured_frame(scene, cam, 1, t, color_noise=noise)).to(cuda)
        return fi
    pipe.integrate_source(inputs(0, 0.0))
    m = pipe.wf.surface_points(16384)
    assert pipe.wf.surface_colors(m) is m["colors"]
    assert m["emitted"] > 5000 and m["colors"].shape == (m["emitted"], 3)
    rgb = m["colors"].cpu().numpy().astype(np.float64)
    assert torch.equal(m["colors"], pipe.vol.voxel_rgb(m["voxel"]))
    vox = m["voxel"].cpu().numpy().astype(np.int64)
    D = c["dims"]
    ijk = np.stack([vox // (D * D), (vox // D) % D, vox % D], 1)
    centre = np.asarray(c["origin"], np.float32).astype(np.float64) + c["voxel"] * ijk
    u = np.rint(centre[:, 0] * cam.fx / centre[:, 2] + cam.cx).astype(int)
    v = np.rint(centre[:, 1] * cam.fy / centre[:, 2] + cam.cy).astype(int)
    z = scene.render(cam, 0, None, 0.0)[v, u].astype(np.float64)
    assert np.all(z > 0)
    ray = np.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], 1)
    d_pixel = np.abs(rgb - S.surface_texture(ray)).max()
    d_point = np.abs(rgb - S.surface_texture(m["points"].cpu().numpy()))
    print(f"voxel_rgb after the source frame, {m['emitted']} points: max |rgb - texture| at the integrate's pixel = "
          f"{255 * d_pixel:.3f}/255; at the sampled surface points mean {255 * d_point.mean():.2f}/255, max "
          f"{255 * d_point.max():.2f}/255")
    assert d_pixel <= 1.0 / 255.0
    outs = [pipe.track_step(inputs(t), t, model="volume", max_model_points=16384, motion=False, photo=True)
            for t in (1, 2, 3)]
    counts = torch.stack(pipe.model_counts).cpu()
    print("model counts per sampling:", counts.tolist(), "matched:", [[x["accepted"] for x in o["assoc"]] for o in outs])
    assert all(o["valid_solve"] == 1 for o in outs)
    assert counts.shape == (4, 2) and bool((counts[:, 0] > 5000).all())
    assert pipe.vol.frame_id == 3 and "colors" not in pipe._vmodel     # integrated, and re-sampled after the last frame
    for o in outs:
        assert all(len(x["histogram"]) == 8 and x["accepted"] >= 0.8 * int(counts[:, 1].min()) for x in o["assoc"])
    # the canonical model takes the source frame's rgb at the canonical points' own pixels
    o = pipe.track_step(inputs(4), 4, motion=False, photo={"radius": 6})
    n_can = seq.canonical_points.shape[0]
    assert pipe._canonical_colors().shape == (n_can, 3)
    im0 = pipe._source_rgb                                  # canonical_points are the source depth's valid pixels, row-major
    assert torch.equal(pipe._canonical_colors(), im0[:, inputs(0, 0.0).im[5] > 0].t())
    assert o["valid_solve"] == 1 and all(len(x["histogram"]) == 8 and x["accepted"] >= 0.8 * n_can for x in o["assoc"])
