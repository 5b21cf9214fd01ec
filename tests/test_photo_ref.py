"""CPU: known answers for the numpy restatement of ofx_photo_associate (tests/photo_ref.py) on a 40x32 camera: every tap
code, the maximum rule, windows cut by the image borders, the tie rule, the radius-0 identity against assoc_ref, the
thinning, and the spin-scene check of the idea (search + rigid fit)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import photo_ref as pr  # noqa: E402
import prepare_ref as pp  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
H, W = 32, 40
INTR = (30.0, 30.0, 19.5, 15.5)
EDGE = 0.03
# identity warp that is exact in f32: one node at the origin carries the whole weight
NODES = np.zeros((4, 3), F32)
R_ID = np.tile(np.eye(3, dtype=F32), (4, 1, 1))
T_0 = np.zeros((4, 3), F32)
GREY = np.full((3, H, W), 0.5, F32)


def _at(u, v, z):
    fx, fy, cx, cy = INTR
    return [(u - cx) * z / fx, (v - cy) * z / fy, z]


def _run(points, depth, cim=GREY, colors=None, normals=None, valid=None, **kw):
    pts = np.asarray(points, F32).reshape(-1, 3)
    P = pts.shape[0]
    a, w = np.zeros((P, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (P, 1))
    vm = fo.backproject_depth(np.asarray(depth, F32), *INTR)
    nm = pp.normal_map(vm, INTR, EDGE)
    col = np.full((P, 3), 0.5, F32) if colors is None else np.asarray(colors, F32)
    return pr.associate(pts, normals, col, a, w, valid, R_ID, T_0, NODES, INTR, vm, nm, cim, **kw), vm


def _scene_depth():
    depth = np.ones((H, W), F32)
    depth[10, 10] = 0.0          # a hole
    depth[:, 30:] = 1.05         # a 5 cm step between columns 29 and 30
    return depth


def test_every_code_is_reached_at_radius_0():
    down = [0, 0, -1]
    cases = [
        (_at(5, 5, 1.02), down, [0.5] * 3, 1, 0),
        (_at(5, 5, 1.02), down, [0.5] * 3, 0, 1),          # valid == 0
        (_at(5, 5, -1.0), down, [0.5] * 3, 1, 2),          # behind the camera
        ([5.0, 0.0, 1.0], down, [0.5] * 3, 1, 2),          # off the image
        (_at(10, 10, 1.02), down, [0.5] * 3, 1, 3),        # the hole
        (_at(11, 10, 1.02), down, [0.5] * 3, 1, 4),        # a 4-neighbour is the hole: no normal
        (_at(0, 7, 1.02), down, [0.5] * 3, 1, 4),          # the image border
        (_at(29, 20, 1.02), down, [0.5] * 3, 1, 4),        # the depth step
        (_at(5, 5, 1.2), down, [0.5] * 3, 1, 5),           # 20 cm in front of the surface
        (_at(5, 5, 1.02), [0, 0, 1], [0.5] * 3, 1, 6),     # the normal looks away
        (_at(5, 5, 1.02), down, [0.9, 0.5, 0.5], 1, 7),    # 0.4 from the image's colour against color_max = 0.1
        (_at(5, 5, 1.02), down, [np.nan, 0.5, 0.5], 1, 7),  # a NaN colour
    ]
    pts, nrm, col, val, want = (np.array([c[i] for c in cases], F32) for i in range(5))
    out, vm = _run(pts, _scene_depth(), colors=col, normals=nrm, valid=val.astype(np.uint8), radius=0, color_max=0.1)
    assert out["code"].tolist() == want.astype(int).tolist()
    assert np.array_equal(out["tgt"][0], vm[:, 5, 5]) and out["pixel"][0].tolist() == [5, 5] and out["cost"][0] > 0
    assert np.all(out["tgt"][1:] == 0) and np.all(out["pixel"][1:] == -1) and np.all(out["cost"][1:] == 0)
    assert out["count"].tolist() == [1, 1]
    # the NaN colour is refused with the colour gate off too: !(NaN <= inf)
    out, _ = _run(pts, _scene_depth(), colors=col, normals=nrm, valid=val.astype(np.uint8), radius=0)
    assert out["code"].tolist()[-2:] == [0, 7]


def test_point_code_is_the_largest_tap_code_when_nothing_is_eligible():
    depth = _scene_depth()
    # around the hole (10, 10) with radius 1: the hole is 3, its four neighbours are 4, the diagonal taps are complete
    far, _ = _run([_at(10, 10, 1.2)], depth, radius=1)                                  # ... and too far: 5
    col, _ = _run([_at(10, 10, 1.02)], depth, colors=[[0.9, 0.5, 0.5]], radius=1, color_max=0.1)   # ... refused by colour: 7
    away, _ = _run([_at(10, 10, 1.02)], depth, normals=[[0, 0, 1]], radius=1)           # ... facing away: 6
    assert (far["code"][0], away["code"][0], col["code"][0]) == (5, 6, 7)
    ok, _ = _run([_at(10, 10, 1.02)], depth, radius=1)
    assert ok["code"][0] == 0 and ok["pixel"][0].tolist() == [9, 9]    # a diagonal tap, the first in tap order
    # radius 0 at the hole sees the hole alone
    assert _run([_at(10, 10, 1.2)], depth, radius=0)[0]["code"][0] == 3


@pytest.mark.parametrize("uv,first", [((0, 7), (1, 5)), ((39, 7), (37, 5)), ((20, 0), (18, 1)), ((20, 31), (18, 29)),
                                      ((0, 0), (1, 1)), ((39, 31), (37, 29)), ((39, 0), (37, 1)), ((0, 31), (1, 29))])
def test_window_cut_by_borders_and_corners(uv, first):
    """Constant colour and geo_weight 0: every eligible tap costs 0, so the match is the first eligible tap in tap order
    — the first tap inside the image that is not on its border (border pixels have no normal). dist_max is opened to
    30 cm: a pixel is 3.3 cm wide at this camera's metre."""
    out, vm = _run([_at(*uv, 1.02)], np.ones((H, W), F32), radius=2, geo_weight=0.0, dist_max=0.3)
    assert out["code"][0] == 0 and tuple(out["pixel"][0]) == first and out["cost"][0] == 0
    assert np.array_equal(out["tgt"][0], vm[:, first[1], first[0]])


def test_tie_goes_to_the_first_tap_and_the_geometric_weight_breaks_it():
    pts = [_at(20, 15, 1.02), _at(7, 22, 1.02)]
    tie, _ = _run(pts, np.ones((H, W), F32), radius=3, geo_weight=0.0, dist_max=0.3)
    assert tie["pixel"].tolist() == [[17, 12], [4, 19]] and np.all(tie["cost"] == 0)
    near, vm = _run(pts, np.ones((H, W), F32), radius=3, geo_weight=4.0, dist_max=0.3)
    assert near["pixel"].tolist() == [[20, 15], [7, 22]]               # the nearest vertex is the point's own pixel's
    e = vm[:, 15, 20] - np.asarray(pts[0], F32)
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert near["cost"][0] == F32(0.0) + F32(4.0) * d2


@pytest.fixture(scope="module")
def case():
    c = pr.small_case(300)
    c["normal_image"] = pp.normal_map(c["point_image"], c["intr"], EDGE)
    return c


def _args(c, n=None, normals=True, valid=True):
    sl = slice(0, n)
    return (c["points"][sl], c["normals"][sl] if normals else None, c["colors"][sl], c["anchors"][sl], c["weights"][sl],
            c["valid"][sl] if valid else None, c["node_R"], c["node_T"], c["nodes"], c["intr"], c["point_image"],
            c["normal_image"], c["color_image"])


def test_small_case_reaches_every_code(case):
    seen = set()
    for r in (0, 1, 4, 8):
        out = pr.associate(*_args(case), radius=r, color_max=0.15, dist_max=0.15, cos_min=0.7)
        seen |= set(out["code"].tolist())
        hit = out["code"] == 0
        assert hit.sum() > (20 if r >= 1 else 3)
        d = np.abs(out["pixel"][hit] - np.stack(ar.pixel_f32(out["warped"], case["intr"], H, W)[1:], 1)[hit])
        assert d.max() <= r                                            # the match lies in the window
    assert seen == set(range(8))


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("valid", [True, False])
def test_radius_0_is_associate_in_point_mode(case, normals, valid):
    # NaN colours (a point's, a pixel's) are the one thing associate cannot see: taken out for the identity
    c = dict(case, colors=np.nan_to_num(case["colors"], nan=0.5), color_image=np.nan_to_num(case["color_image"], nan=0.5))
    a = _args(c, None, normals, valid)
    out = pr.associate(*a, radius=0, geo_weight=3.0, dist_max=0.03, cos_min=0.7, max_matches=50)
    ref = ar.associate(a[0], a[1], *a[3:11], dist_max=0.03, cos_min=0.7, edge_max=EDGE, mode=ar.POINT, max_matches=50)
    assert ref["count"][0] > 50
    for k in ("code", "tgt", "warped", "match_idx", "src", "tgt_out", "anchors", "weights", "count"):
        assert np.array_equal(out[k].view(np.uint32) if out[k].dtype == F32 else out[k],
                              ref[k].view(np.uint32) if ref[k].dtype == F32 else ref[k]), k


def test_thinning_when_accepted_exceeds_max_matches(case):
    full = pr.associate(*_args(case), radius=4, max_matches=10000)
    n = int(full["count"][0])
    assert n > 40 and full["count"][1] == n
    thin = pr.associate(*_args(case), radius=4, max_matches=37)
    assert thin["count"].tolist() == [n, 37]
    acc = np.nonzero(full["code"] == 0)[0]
    assert np.array_equal(thin["match_idx"], acc[ar.emitted_ranks(n, 37)])
    assert np.array_equal(thin["pixel_out"], full["pixel"][thin["match_idx"]].astype(F32))
    assert np.array_equal(thin["tgt_out"], full["tgt"][thin["match_idx"]])


def _spin_check(spin_deg, radius, geo_weight=1.0):
    """The sphere of the bench scene at config 1's camera, spun about its own centre (the depth does not change), the
    search in one pass from the identity, then a rigid fit on the matches -> (identity error, fitted error, share of
    single matches more than 1 cm off), mean 3-D errors in metres against the ground truth."""
    from occlusionfusion_amd import synthetic as S
    cam = S.bench_camera(2)
    scene = S.SphereScene(motion="spin", occluder=False, spin_rate=np.radians(spin_deg))
    clean = scene.render(cam, 0, None, 0.0)
    im1 = S.textured_frame(scene, cam, 1, 1)
    intr = tuple(float(x) for x in cam.as_vec())
    vm0 = fo.backproject_depth(clean, *intr)
    c = np.array(scene.center)
    pts = vm0.reshape(3, -1).T[clean.reshape(-1) > 0]
    pts = pts[np.linalg.norm(pts - c, axis=1) < scene.radius + 0.01]             # the sphere's pixels
    nrm = ((pts - c) / np.linalg.norm(pts - c, axis=1, keepdims=True)).astype(F32)
    pts = pts[(nrm * pts).sum(1) / np.linalg.norm(pts, axis=1) < -0.3]            # front-facing with a margin
    col = (np.round(S.surface_texture(pts) * 255.0) / 255.0).astype(F32)          # 8-bit model colours
    P = pts.shape[0]
    a, w = np.zeros((P, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (P, 1))
    vm1 = fo.backproject_depth(np.ascontiguousarray(im1[5]), *intr)
    nm1 = pp.normal_map(vm1, intr, EDGE)
    out = pr.search(pts, None, col, a, w, None, R_ID, T_0, NODES, intr, vm1, nm1, im1[:3], radius=radius,
                    geo_weight=geo_weight)
    gt = scene.deform_points(pts, 1)
    hit = out["code"] == 0
    e_id = float(np.linalg.norm(pts - gt, axis=1).mean())
    R, t = pr.rigid_fit(pts[hit], out["tgt"][hit])
    e_fit = float(np.linalg.norm(pts.astype(np.float64) @ R.T + t - gt, axis=1).mean())
    off = float((np.linalg.norm(out["tgt"][hit] - gt[hit], axis=1) > 0.01).mean())
    return e_id, e_fit, off, P, float(hit.mean())


def test_spin_scene_search_and_rigid_fit():
    """Measured (CPU, one pass, radius 6, a 3 degree spin, 13 063 front-facing points, all matched): mean 3-D error
    16.46 mm under the identity, 1.33 mm after the rigid fit on the matches, 6.0 % of single matches more than 1 cm
    off. Asserted: the fitted error is below half the identity error."""
    e_id, e_fit, off, P, share = _spin_check(3.0, 6)
    print(f"spin 3 deg, radius 6: {P} points, matched {share:.3f}, identity {e_id * 1e3:.2f} mm, "
          f"fitted {e_fit * 1e3:.2f} mm, single matches > 1 cm off {off:.3f}")
    assert e_fit < 0.5 * e_id
