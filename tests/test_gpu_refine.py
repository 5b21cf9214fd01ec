"""GPU: the sub-pixel refinement of the photometric matches (ofx_photo_refine, torch.ops.ofx.photo_refine,
ProjectiveAssociator.refine_photo, the photo_refine= keyword of the tracking layers).

* the kernel equals the numpy restatement (tests/refine_ref.py) on the 40x32 case for half 1, 3 and 4: every status, the
  refined pixel within 2 f32 ulp, the target within 4, the residual within 1e-6 relative (only the f64 summation order
  differs between the lane tree and the restatement); rows past the count untouched;
* two calls are byte-identical, a count of 0 and a count of max_rows work, the operator equals the direct C-ABI call
  and passes opcheck;
* on the default spin scene, frame 0 -> 1, the refined matches' median pixel error is at most a quarter of the
  whole-pixel matches', and at least 90 % of the front-facing matches are refined;
* tracking that frame with photo_refine=True closes at least a third of the gap that photo=True leaves to a solve on
  ground-truth matches; photo_refine=None is photo=True byte for byte;
* FusionPipeline.track_step(model="canonical", photo_refine=...) builds its template from the source frame and refines
  every iteration's matches; model="volume" is refused.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as rr  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("template_image", "template_mask", "color_image", "point_image", "template_px", "init_px", "tgt_in", "count")


@pytest.fixture(scope="module")
def cases(cuda):
    """small_case for half 1, 3 and 4 with the restatement's outputs (computed once, never modified) and the device
    copies of the inputs."""
    out = {}
    for half in (1, 3, 4):
        c = rr.small_case(half)
        R = c["init_px"].shape[0]
        c["ref"] = rr.refine(*(c[k] for k in KEYS), c["edge_max"], outputs=_prefill_np(R), **c["params"])
        c["dev"] = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(cuda) for k in KEYS}
        out[half] = c
    return out


def _prefill_np(R):
    return dict(px_out=np.full((R, 2), -7.0, np.float32), tgt_out=np.full((R, 3), -7.0, np.float32),
                status=np.full(R, 99, np.uint8), ssd=np.full(R, -7.0, np.float32))


def _prefill(R, dev):
    return tuple(torch.from_numpy(v).to(dev) for v in _prefill_np(R).values())


def _direct(d, edge_max, prm, count=None, rows=None, mask=True):
    """ofx_photo_refine through ctypes on the first `rows` rows; every output prefilled."""
    R = d["init_px"].shape[0] if rows is None else rows
    _, H, W = d["color_image"].shape
    out = _prefill(R, d["init_px"].device)
    p = _lib.RefineParams(prm["half"], prm["iters"], prm["eps"], prm["max_shift"], prm["min_eig"], prm["ssd_max"],
                          edge_max, 0)
    call("ofx_photo_refine", ptr(d["template_image"]), ptr(d["template_mask"]) if mask else None,
         ptr(d["color_image"]), ptr(d["point_image"]), ptr(d["template_px"]), ptr(d["init_px"]), ptr(d["tgt_in"]),
         ptr(d["count"] if count is None else count), R, H, W, byref(p), *(ptr(t) for t in out), stream_ptr())
    return out


def _same_bytes(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _ulps(got, want):
    """|got - want| in units of want's f32 spacing; equal bits (NaN inputs copied through) count as 0."""
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
    with np.errstate(invalid="ignore"):
        u = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return np.where(same, 0.0, np.where(np.isnan(u), np.inf, u))


@pytest.mark.parametrize("half", [1, 3, 4])
def test_kernel_equals_restatement(cases, half):
    c = cases[half]
    ref = c["ref"]
    n = int(c["count"][1])
    px, tgt, status, ssd = (t.cpu().numpy() for t in _direct(c["dev"], c["edge_max"], c["params"]))
    # a row may be left out of the status comparison only if the restatement itself sits on a threshold (none does:
    # test_refine_ref asserts it on the CPU); at most 1 % of the rows
    close = ref["margin"][:n] < 1e-6
    assert close.sum() <= 0.01 * n
    keep = ~close
    assert np.array_equal(status[:n][keep], ref["status"][:n][keep])
    assert set(status[:n].tolist()) == set(range(8))
    u_px, u_tgt = _ulps(px[:n], ref["px_out"][:n])[keep], _ulps(tgt[:n], ref["tgt_out"][:n])[keep]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(ssd[:n].astype(np.float64) - ref["ssd"][:n]) / np.abs(ref["ssd"][:n].astype(np.float64))
    rel = np.where(ssd[:n] == ref["ssd"][:n], 0.0, rel)[keep]
    print(f"half {half}: {int(keep.sum())} rows compared, px_out max {u_px.max():.2f} ulp, tgt_out max {u_tgt.max():.2f} "
          f"ulp, ssd max rel {rel.max():.2e}, status histogram {np.bincount(status[:n], minlength=8).tolist()}")
    assert u_px.max() <= 2 and u_tgt.max() <= 4 and rel.max() <= 1e-6
    # rows at or past the count keep the prefill
    assert np.all(px[n:] == -7) and np.all(tgt[n:] == -7) and np.all(status[n:] == 99) and np.all(ssd[n:] == -7)


def test_repeatability_counts_op_and_opcheck(cases, cuda):
    c = cases[3]
    d, prm, edge = c["dev"], c["params"], c["edge_max"]
    R = d["init_px"].shape[0]
    a = _direct(d, edge, prm)
    _direct(d, edge, dict(prm, half=4), rows=65)               # other work in between
    b = _direct(d, edge, prm)
    assert _same_bytes(a, b)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=cuda)  # noqa: E731
    # a count of 0 (and a negative one) writes nothing; a count at or above max_rows writes every row
    for cnt in (i32(0, 0), i32(7, -2)):
        assert _same_bytes(_direct(d, edge, prm, count=cnt), _prefill(R, cuda))
    full = _direct(d, edge, prm, count=i32(R, R))
    over = _direct(d, edge, prm, count=i32(R + 5, R + 5))
    assert _same_bytes(full, over) and bool((full[2] != 99).all())
    n = int(c["count"][1])
    assert _same_bytes([t[:n] for t in full], [t[:n] for t in a])
    for rows in (1, 7, 8, 9, 63, 65):                           # partial lane groups and waves: max_rows clamps
        part = _direct(d, edge, prm, rows=rows)
        assert _same_bytes(part, [t[:rows] for t in a])
    nomask = _direct(d, edge, prm, mask=False)
    assert not torch.equal(nomask[2], a[2])                     # the mask's hole decides some rows
    # the operator: the same bytes as the C ABI, in place
    for half, mask in ((3, True), (4, False), (1, True)):
        p = dict(prm, half=half)
        want = _direct(d, edge, p, mask=mask)
        got = _prefill(R, cuda)
        r = torch.ops.ofx.photo_refine(d["template_image"], d["template_mask"] if mask else None, d["color_image"],
                                       d["point_image"], d["template_px"], d["init_px"], d["tgt_in"], d["count"],
                                       p["half"], p["iters"], p["eps"], p["max_shift"], p["min_eig"], p["ssd_max"], edge,
                                       *got)
        assert r is None and _same_bytes(got, want)
    # a bool mask is taken as well
    got = _prefill(R, cuda)
    torch.ops.ofx.photo_refine(d["template_image"], d["template_mask"].bool(), d["color_image"], d["point_image"],
                               d["template_px"], d["init_px"], d["tgt_in"], d["count"], prm["half"], prm["iters"],
                               prm["eps"], prm["max_shift"], prm["min_eig"], prm["ssd_max"], edge, *got)
    assert _same_bytes(got, a)
    sl = slice(24, 89)        # past the case's NaN rows: opcheck compares by value, and NaN != NaN
    small = (d["template_image"], d["template_mask"], d["color_image"], d["point_image"], d["template_px"][sl],
             d["init_px"][sl], d["tgt_in"][sl], i32(65, 61), 3, 8, 1e-3, 2.5, 1e-6, 0.05, edge,
             *(t.zero_() for t in _prefill(65, cuda)))
    torch.library.opcheck(torch.ops.ofx.photo_refine.default, small)


# ------------------------------------------------------------------------------------------------ the spin scene
N_MODEL = 2 * 4096 + 37
T_SPIN = 1          # frames 0 -> 1 of the default spin scene: 1.5 degrees about the sphere's own centre


@pytest.fixture(scope="module")
def spin(cuda):
    """test_gpu_photo's set-up — config 1's volume and camera around the default spin scene, the exact direct solve,
    N_MODEL canonical points with the textured source frame's colours — plus the template: the source frame's rgb and
    every point's own projection into it."""
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.registration import Registration
    scene, seed = S.SphereScene(motion="spin", occluder=False), 1
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
    sel = np.sort(np.random.default_rng(5).choice(cp.shape[0], N_MODEL, replace=False))
    px = np.stack([cp[:, 0] * cam.fx / cp[:, 2] + cam.cx, cp[:, 1] * cam.fy / cp[:, 2] + cam.cy], 1)
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    reg = Registration(cp[sel], graph, wf, K, precond="direct")
    reg.update(cp[sel], colors=col[sel], template=(im0[:3], px[sel], None))
    assert reg.source_template[1].shape == (reg.source_pcd.shape[0], 2)
    frame = S.textured_frame(scene, cam, seed, T_SPIN)
    src = reg.source_pcd.cpu().numpy().astype(np.float64)
    gt = scene.deform_points(src, T_SPIN)
    ctr = np.array(scene.center)

    def facing(p):
        n = (p - ctr) / np.linalg.norm(p - ctr, axis=1, keepdims=True)
        return (n * p).sum(1) / np.linalg.norm(p, axis=1) < -0.3
    sphere = (np.linalg.norm(src - ctr, axis=1) < scene.radius + 0.01) & (src[:, 2] < scene.plane_z - 0.02)
    front = sphere & facing(src) & facing(gt)
    assert front.sum() > 1000
    return SimpleNamespace(seq=seq, reg=reg, intr=intr, cam=cam, frame=frame, src=src, gt=gt, front=front)


def test_refined_matches_are_sub_pixel(spin, cuda):
    """associate_photo at the identity, then refine_photo against the source frame. The pixel error of a match is its
    distance to the projection of scene.deform_points of its model point; over the front-facing matches the refined
    median must be at most a quarter of the whole-pixel median measured here, and at least 90 % of them must have
    status 0. Measured on the MI355X (2438 front-facing matches): median / p90 0.634 / 1.584 px -> 0.069 / 0.154 px, 99.5 %
    refined (13 rows stop at max_shift). The f64 CPU prototype: median 0.63 px -> 0.069 px, 98-100 % refined."""
    from occlusionfusion_amd.association import ASSOC_DEFAULTS, PHOTO_DEFAULTS, ProjectiveAssociator, pack_transforms
    from occlusionfusion_amd.image_proc import prepare_depth_device
    reg, cam = spin.reg, spin.cam
    P = reg.source_pcd.shape[0]
    depth = torch.from_numpy(np.ascontiguousarray(spin.frame[5])).to(cuda)
    cim = torch.from_numpy(np.ascontiguousarray(spin.frame[:3])).to(cuda)
    prep = prepare_depth_device(depth, *spin.intr, radius=0, edge_max=ASSOC_DEFAULTS["edge_max"], normals=True)
    pa = ProjectiveAssociator(P, cuda)
    packed = pack_transforms(reg.graph.nodes, None, None, cuda)
    m = pa.associate_photo(reg.source_pcd, None, reg.source_colors, reg.point_anchors, reg.anchor_weight, None, packed,
                           prep["point_image"], prep["normals"], cim, spin.intr, dist_max=ASSOC_DEFAULTS["dist_max"],
                           cos_min=ASSOC_DEFAULTS["cos_min"], max_matches=P, **PHOTO_DEFAULTS)
    t_im, t_px, t_mask = reg.source_template
    idx = m["match_idx"].long()
    r = pa.refine_photo(m, t_im, t_px[idx], cim, prep["point_image"], ASSOC_DEFAULTS["edge_max"], t_mask)
    assert r["pixel"].shape == m["pixel"].shape and r["tgt"].shape == m["tgt"].shape
    assert r["refine_status"].dtype == torch.uint8 and r["refine_ssd"].shape == (m["emitted"],)
    assert torch.equal(r["match_idx"], m["match_idx"]) and r["src"] is m["src"]
    idx = idx.cpu().numpy()
    want = np.stack([spin.gt[idx, 0] * cam.fx / spin.gt[idx, 2] + cam.cx,
                     spin.gt[idx, 1] * cam.fy / spin.gt[idx, 2] + cam.cy], 1)
    f = spin.front[idx]
    assert f.sum() > 1000
    e_whole = np.linalg.norm(m["pixel"].cpu().numpy().astype(np.float64) - want, axis=1)[f]
    e_fine = np.linalg.norm(r["pixel"].cpu().numpy().astype(np.float64) - want, axis=1)[f]
    st = r["refine_status"].cpu().numpy()[f]
    share = float((st == 0).mean())
    print(f"spin, frame 0 -> {T_SPIN}: {int(f.sum())} front-facing matches; pixel error median / p90: whole-pixel "
          f"{np.median(e_whole):.3f} / {np.percentile(e_whole, 90):.3f} px, refined {np.median(e_fine):.3f} / "
          f"{np.percentile(e_fine, 90):.3f} px; refined share {share:.4f}, status histogram "
          f"{np.bincount(st, minlength=8).tolist()}")
    assert np.median(e_fine) <= 0.25 * np.median(e_whole)
    assert share >= 0.9
    # a refined row's target is the vertex map at its pixel; a fallback row keeps the search's
    fb = torch.from_numpy(r["refine_status"].cpu().numpy() != 0).to(cuda)
    assert torch.equal(r["tgt"][fb], m["tgt"][fb]) and torch.equal(r["pixel"][fb], m["pixel"][fb])


def test_tracking_with_refined_matches(spin, cuda):
    """The spin scene of test_gpu_photo and its loop (from the identity, 3 ICP iterations, no motion data), frame 0 -> 1:
    1.5 degrees, a frame-to-frame motion. Error: the mean 3-D distance of the warped canonical points to
    scene.deform_points over the front-facing points. e_id: the identity; e_gt: one solve on 3000 ground-truth matches;
    e_photo: track(photo=True); e_ref: track(photo=True, photo_refine=True). The refinement must close a third of the
    gap photo=True leaves to e_gt. Measured on the MI355X (2438 front-facing points of 8229): e_id 8.218 mm, e_gt 0.498 mm,
    e_photo 1.005 mm, e_ref 0.784 mm against a bar of 0.836 mm. The f64 CPU prototype (Euclidean graph): 8.218 / 0.366 /
    1.297 / 0.740 mm against a bar of 0.987 mm. photo_refine=None is photo=True byte for byte."""
    from test_gpu_photo import _gt_solve, _reset
    reg = spin.reg
    frame = {"im": spin.frame, "id": T_SPIN}

    def err(w):
        return float(np.linalg.norm(np.asarray(w, np.float64) - spin.gt, axis=1)[spin.front].mean())
    e_id = err(spin.src)
    e_gt = err(_gt_solve(spin.seq, reg, spin.intr, T_SPIN, cuda))
    _reset(reg)
    pho = reg.track(frame, icp_iters=3, photo=True)
    e_photo = err(pho["warped_verts"].cpu().numpy())
    _reset(reg)
    off = reg.track(frame, icp_iters=3, photo=True, photo_refine=None)
    _reset(reg)
    ref = reg.track(frame, icp_iters=3, photo=True, photo_refine=True)
    e_ref = err(ref["warped_verts"].cpu().numpy())
    bar = e_photo - (e_photo - e_gt) / 3.0
    print(f"spin, frame 0 -> {T_SPIN}: {int(spin.front.sum())} front-facing points of {spin.src.shape[0]}, e_id = "
          f"{1e3 * e_id:.3f} mm, e_gt = {1e3 * e_gt:.3f} mm, e_photo = {1e3 * e_photo:.3f} mm, e_ref = "
          f"{1e3 * e_ref:.3f} mm, bar = {1e3 * bar:.3f} mm")
    assert pho["valid_solve"] == 1 and ref["valid_solve"] == 1 and off["valid_solve"] == 1
    for k in ("node_rotations", "node_translations", "warped_verts"):
        x, y = (np.ascontiguousarray(torch.as_tensor(o[k]).cpu().numpy()) for o in (off, pho))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert [x["histogram"] for x in off["assoc"]] == [x["histogram"] for x in pho["assoc"]]
    assert e_gt < e_photo
    assert e_ref <= bar, (e_id, e_gt, e_photo, e_ref)


def test_pipeline_refines_the_canonical_model(cuda, monkeypatch):
    """FusionPipeline.track_step(model="canonical", photo=True, photo_refine=...) on the spin scene's frame 1: the
    template is the source frame's rgb and every canonical point's own pixel (integer pixel centres: the points are the
    source depth's backprojected pixels); each of the three ICP iterations refines its matches (most of them: status
    0) before a valid solve. model="volume" is refused before anything is touched."""
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.association import ProjectiveAssociator
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
    src = inputs(0, 0.0)
    pipe.integrate_source(src)
    t_im, t_px, t_mask = pipe._canonical_template()
    n_can = seq.canonical_points.shape[0]
    assert t_mask is None and torch.equal(t_im, src.im[:3]) and t_px.shape == (n_can, 2)
    v, u = torch.nonzero(src.im[5] > 0, as_tuple=True)             # canonical_points: the valid pixels, row-major
    assert float((t_px - torch.stack([u, v], 1).float()).abs().max()) < 1e-2
    calls = []
    orig = ProjectiveAssociator.refine_photo

    def spy(self, *a, **k):
        r = orig(self, *a, **k)
        calls.append((k, r))
        return r
    monkeypatch.setattr(ProjectiveAssociator, "refine_photo", spy)
    o = pipe.track_step(inputs(1), 1, motion=False, photo=True, photo_refine={"half": 2})
    assert o["valid_solve"] == 1 and len(o["assoc"]) == 3 and len(calls) == 3
    for k, r in calls:
        assert k["half"] == 2 and k["iters"] == 8
        st = r["refine_status"]
        assert st.shape[0] == r["tgt"].shape[0] == r["pixel"].shape[0] == r["src"].shape[0] > 1000
        assert float((st == 0).float().mean()) > 0.5
    with pytest.raises(ValueError, match="not built"):
        pipe.track_step(inputs(2), 2, model="volume", photo=True, photo_refine=True)
    assert len(calls) == 3
