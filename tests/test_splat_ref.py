"""CPU: known answers for the numpy restatement of ofx_splat_points (tests/splat_ref.py) — disc geometry on hand-made
cases, the permutation property of the z-buffer, the two-layer scene in which a tracker without the occlusion gate pulls
a hidden surface onto the one in front of it, and config 1's volume model rendered against the frame it was fused from."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import splat_ref as sp  # noqa: E402
import surface_ref as sr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
INTR = (100.0, 100.0, 16.0, 16.0)       # pixel (16, 16) looks along the axis
H = W = 33
DOWN = np.array([[0, 0, -1]], F32)


def _one(x, n=DOWN, rho=0.025, intr=INTR, h=H, w=W):
    x = np.asarray(x, F32).reshape(-1, 3)
    n = None if n is None else np.broadcast_to(np.asarray(n, F32).reshape(-1, 3), x.shape)
    return sp.splat_warped(x, n, np.ones(x.shape[0], bool), intr, h, w, rho, 0.01)


def _disc_pixels(c, n, rho, intr=INTR, h=H, w=W):
    """f64: the pixels whose ray hits the plane through c with normal n within rho of c, and the smallest distance of a
    hit's |e| from rho (how far the case is from a borderline pixel)."""
    c, n = np.asarray(c, np.float64), np.asarray(n, np.float64)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(u - intr[2]) / intr[0], (v - intr[3]) / intr[1], np.ones_like(u, dtype=np.float64)], -1)
    zp = (n @ c) / (d @ n)
    e = np.linalg.norm(d * zp[..., None] - c, axis=-1)
    return (e <= rho) & (zp > 0), float(np.abs(e - rho).min())


def test_fronto_parallel_disc_covers_the_pixels_whose_ray_hits_it():
    c = np.array([0.002, -0.001, 1.0])
    depth, index, code = _one(c)
    want, slack = _disc_pixels(c, [0, 0, -1], 0.025)
    assert slack > 1e-5                                    # no pixel of the case is borderline in f32
    assert want.sum() == 21 and np.array_equal(depth > 0, want) and code.tolist() == [0]
    assert np.array_equal(index, np.where(want, 0, -1))
    assert np.all(depth[want] == F32(1.0))                 # fronto-parallel: every hit is at the point's depth
    assert depth[16, 16] == F32(1.0)


def test_tilted_disc_is_an_ellipse():
    t = np.deg2rad(60.0)
    n = np.array([np.sin(t), 0.0, -np.cos(t)])            # turned about the image's vertical axis
    c = np.array([0.0, 0.0, 1.0])
    depth, _, code = _one(c, n, rho=0.035)
    want, slack = _disc_pixels(c, n, 0.035)
    assert slack > 1e-5 and code.tolist() == [0]
    assert np.array_equal(depth > 0, want)
    cols, rows = np.unique(np.nonzero(want)[1]).size, np.unique(np.nonzero(want)[0]).size
    assert cols < rows and rows == 7 and cols == 3, (cols, rows)
    # the plane recedes to the right (n_x > 0): depths grow with u along the centre row
    row = depth[16][want[16]]
    assert np.all(np.diff(row) > 0)


def test_radius_is_clamped_and_the_footprint_is_clipped():
    depth, _, code = _one([0.0, 0.0, 0.05])               # 100·0.025/0.05 = 50 pixels -> OFX_SPLAT_RMAX
    assert code.tolist() == [0] and int((depth > 0).sum()) == (2 * sp.RMAX + 1) ** 2
    vv, uu = np.nonzero(depth > 0)
    assert uu.min() == 16 - sp.RMAX and uu.max() == 16 + sp.RMAX and vv.min() == 16 - sp.RMAX
    c = np.array([-0.16, -0.16, 1.0])                      # pixel (0, 0)
    depth, index, code = _one(c)
    want, slack = _disc_pixels(c, [0, 0, -1], 0.025)
    assert slack > 1e-5 and code.tolist() == [0] and np.array_equal(depth > 0, want)
    assert want[0, 0] and 1 < want.sum() < 21 and not want[3:, :].any() and not want[:, 3:].any()


def test_nan_points_and_bad_normals_write_nothing():
    x = np.array([[np.nan, 0, 1], [0, 0, 1], [0.05, 0, 1], [0, 0.05, -1.0], [5.0, 0, 1]], F32)
    n = np.array([[0, 0, -1], [np.nan, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], F32)
    depth, index, code = sp.splat_warped(x, n, np.ones(5, bool), INTR, H, W, 0.025, 0.01)
    assert code.tolist() == [2, 3, 3, 2, 2]
    assert not (depth > 0).any() and np.all(index == -1)
    _, _, code = sp.splat_warped(x, n, np.zeros(5, bool), INTR, H, W, 0.025, 0.01)
    assert code.tolist() == [1] * 5


def test_identical_points_go_to_the_lower_index_and_no_normals_means_facing_the_camera():
    c = [0.002, -0.001, 1.0]
    depth, index, code = _one([c, c])
    assert code.tolist() == [0, 0] and set(np.unique(index)) == {-1, 0} and (index == 0).sum() == 21
    d1, i1, c1 = _one([c, c], n=None)
    assert np.array_equal(d1.view(np.uint32), depth.view(np.uint32)) and np.array_equal(i1, index)
    assert c1.tolist() == [0, 0]
    # without normals nothing can be back-facing, whatever the point
    _, _, c2 = _one([[0.05, 0.05, 0.5], [-0.1, 0.05, 2.0]], n=None)
    assert c2.tolist() == [0, 0]


def test_occlusion_code_and_margin():
    x = np.array([[0, 0, 1.0], [0.001, 0, 1.009], [0.0, 0.001, 1.02]], F32)
    _, index, code = _one(x)
    assert code.tolist() == [0, 0, 4] and index[16, 16] == 0


def test_permutation_leaves_the_depth_and_moves_only_tied_indices():
    x, n, ok = sp.random_cloud()
    P = x.shape[0]
    depth, index, code = sp.splat_warped(x, n, ok, INTR, H, W, 0.012, 0.01)
    assert np.bincount(code, minlength=5).min() > 0        # every code occurs
    # tied pixels: where the lowest and the highest index among the winners differ (the reversed order)
    _, irev, _ = sp.splat_warped(x[::-1], n[::-1], ok[::-1], INTR, H, W, 0.012, 0.01)
    tied = np.where(irev >= 0, P - 1 - irev, -1) != index
    assert 0 < tied.sum() < 0.5 * (index >= 0).sum()
    perm = np.random.default_rng(7).permutation(P)
    d2, i2, c2 = sp.splat_warped(x[perm], n[perm], ok[perm], INTR, H, W, 0.012, 0.01)
    assert np.array_equal(d2.view(np.uint32), depth.view(np.uint32))
    assert np.array_equal(c2, code[perm])
    back = np.where(i2 >= 0, perm[np.maximum(i2, 0)], -1)
    assert np.array_equal(back[~tied], index[~tied])


# ----------------------------------------------------------------------------------------------- the two-layer scene
def track_two_layers(sc, gated, rounds=3):
    """Three rounds of associate -> gn_optimize from the identity on the CPU -> (R, T, per round dict(codes, hidden
    accepted, splat code or None))."""
    N, P = sc["nodes"].shape[0], sc["points"].shape[0]
    vm = fo.backproject_depth(sc["depth"], *sc["intr"])
    R, T = np.tile(np.eye(3, dtype=F32), (N, 1, 1)), np.zeros((N, 3), F32)
    log = []
    for _ in range(rounds):
        valid, scode = None, None
        if gated:
            scode = sp.splat(sc["points"], sc["normals"], sc["anchors"], sc["weights"], None, R, T, sc["nodes"],
                             sc["intr"], sc["H"], sc["W"], 0.004, 0.01)["code"]
            valid = scode == 0
        m = ar.associate(sc["points"], sc["normals"], sc["anchors"], sc["weights"], valid, R, T, sc["nodes"], sc["intr"],
                         vm, max_matches=10000)
        log.append({"hidden_accepted": int(((m["code"] == 0) & sc["hidden"]).sum()), "splat_code": scode})
        out = fo.gn_optimize(sc["nodes"], sc["edges"], sc["edge_weights"], sc["nodes"], np.zeros(N, F32), m["src"],
                             m["anchors"], m["weights"], m["tgt_out"], sc["intr"], prev_rot=R, prev_trans=T)
        assert out["valid_solve"]
        R = np.asarray(out["node_rotations"], F32).reshape(N, 3, 3)
        T = np.asarray(out["node_translations"], F32).reshape(N, 3)
    return R, T, log


@pytest.fixture(scope="module")
def scene():
    return sp.two_layer_scene()


def test_two_layer_scene_counts(scene):
    assert scene["points"].shape[0] == 9801 + 1681 and scene["n_rear"] == 9801 and scene["nodes"].shape[0] == 142
    assert int(scene["hidden"].sum()) == 1681 and int(scene["hidden_nodes"].sum()) == 9
    assert (scene["H"], scene["W"]) == (112, 160)


def test_two_layers_identity_render_marks_the_hidden_points(scene):
    N = scene["nodes"].shape[0]
    r = sp.splat(scene["points"], scene["normals"], scene["anchors"], scene["weights"], None,
                 np.tile(np.eye(3, dtype=F32), (N, 1, 1)), np.zeros((N, 3), F32), scene["nodes"], scene["intr"],
                 scene["H"], scene["W"], 0.004, 0.01)
    code, hidden = r["code"], scene["hidden"]
    print("codes", np.bincount(code, minlength=5).tolist(), "other points coded 4:", int((code[~hidden] == 4).sum()))
    assert np.all(code[hidden] == 4)
    assert (code[~hidden] == 4).sum() <= 0.05 * (~hidden).sum()
    assert set(np.unique(code)) <= {0, 4}


@pytest.mark.slow
def test_two_layers_gated_tracking_leaves_the_hidden_nodes_alone(scene):
    _, T, log = track_two_layers(scene, gated=True)
    hn = scene["hidden_nodes"]
    moved = np.linalg.norm(T[hn], axis=1)
    print("gated: hidden accepted per round", [l["hidden_accepted"] for l in log], "max |T| of hidden nodes",
          float(moved.max()))
    for l in log:
        assert l["hidden_accepted"] == 0
        assert np.all(l["splat_code"][scene["hidden"]] == 4)
        assert (l["splat_code"][~scene["hidden"]] == 4).sum() <= 0.05 * (~scene["hidden"]).sum()
    assert moved.max() <= 1e-3


@pytest.mark.slow
def test_two_layers_ungated_tracking_pulls_the_hidden_nodes_forward(scene):
    """The check that the scene discriminates: without the gate the hidden rear nodes end on the front patch."""
    _, T, log = track_two_layers(scene, gated=False)
    moved = np.linalg.norm(T[scene["hidden_nodes"]], axis=1)
    print("ungated: hidden accepted per round", [l["hidden_accepted"] for l in log], "|T| of hidden nodes",
          moved.min(), moved.max())
    assert log[0]["hidden_accepted"] > 1000
    assert moved.min() >= 0.02


# ----------------------------------------------------------------------------------------------- config 1's model
@pytest.mark.slow
def test_config_1_volume_model_renders_onto_its_own_frame():
    """Frame 0 integrated by the oracle, the model sampled by surface_ref (the chain of test_surface_ref's slow test),
    rendered under the identity with rho = the voxel and margin 0.01, against frame 0's depth."""
    from occlusionfusion_amd import synthetic as S
    c = S.BASELINE_CONFIGS[1]
    scene, seed = S.config_scene(1)
    cam = S.bench_camera(c["cam_scale"])
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = (c["dims"],) * 3
    V = int(np.prod(D))
    origin = np.asarray(c["origin"], F32)
    tsdf, weight, color = np.ones(V, F32), np.zeros(V, F32), np.zeros(V, F32)
    d0 = S.frame_depth(scene, cam, seed, 0)
    fo.integrate(tsdf, weight, color, fo.world_points(origin, D, c["voxel"]), np.ones(V, bool), d0, None, intr,
                 with_color=False)
    a, w = np.zeros((V, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (V, 1))
    bricks = np.arange(np.prod([(d + 7) // 8 for d in D]), dtype=np.int32)
    m = sr.surface_points(tsdf.reshape(D), weight.reshape(D), origin, c["voxel"], bricks, a, w, 1.0, V)
    n = int(m["count"][1])
    assert n > 5000
    p, nn = m["points"][:n], m["normals"][:n]
    depth, index, code = sp.splat_warped(p, nn, np.ones(n, bool), intr, cam.height, cam.width, c["voxel"], 0.01)
    cov = depth > 0
    both = cov & (d0 > 0)
    err = np.abs(depth[both].astype(np.float64) - d0[both])
    nb = sum(np.roll(np.roll(cov, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0))
    holes = int(((~cov) & (nb >= 6)).sum())
    print(f"{n} points, codes {np.bincount(code, minlength=5).tolist()}, covered {int(cov.sum())}, share > 2 cm "
          f"{float((err > 0.02).mean()):.4f}, mean |dz| {err.mean() * 1e3:.2f} mm, interior holes {holes}")
    assert (code == 4).mean() <= 0.10
    assert (err > 0.02).mean() <= 0.02 and err.mean() <= 0.005
    assert holes <= 0.03 * cov.sum()
    for use_n, rho in ((False, c["voxel"]), (False, 0.5 * c["voxel"])):   # for the record (DESIGN), not asserted
        _, _, cd = sp.splat_warped(p, None, np.ones(n, bool), intr, cam.height, cam.width, rho, 0.01)
        print(f"without normals, rho = {rho}: occluded share {float((cd == 4).mean()):.4f}")
