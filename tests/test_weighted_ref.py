"""CPU: the numpy restatement of the weighted integrate and of the observation-weight map (tests/weighted_ref.py) against
the scalar oracle and against known answers — what tests/test_gpu_weighted_integrate.py then holds the kernels to."""
import math
import os
import sys

import numpy as np
import pytest

from oracle import fusion_oracle as fo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cache_ref as sr  # noqa: E402
import weighted_ref as wr  # noqa: E402

F32, F64 = np.float32, np.float64
eq = np.testing.assert_array_equal


@pytest.mark.parametrize("c", [1.0, 0.5, 0.3])
def test_collapses_to_the_scalar_oracle(c):
    """A constant weight image and no cap is fo.integrate with a scalar obs_weight, bit for bit, on scene A's random old
    state. The image holds f32(c), so the scalar it equals is f32(c) as well (0.3 is not an f32: the f64 0.3 differs from
    it in the 25th bit and gives other tsdf bits, as it should); with the constant in obs_weight and an image of ones the
    f64 c itself is reproduced."""
    sc, skin = sr.scene_a(), sr.skin_a()
    H, W = sc.depth.shape
    ref32 = sr.two_frame_fusion(sc, skin, sc.state, float(F32(c)))
    got = wr.two_frame_weighted(sc, skin, sc.state, 1.0, np.full((H, W), c, F32))
    assert got.n == ref32.n > 1000
    eq(got.tsdf, ref32.tsdf), eq(got.weight, ref32.weight), eq(got.color, ref32.color), eq(got.counts, ref32.counts)
    ref64 = sr.two_frame_fusion(sc, skin, sc.state, c)
    got = wr.two_frame_weighted(sc, skin, sc.state, c, np.ones((H, W), F32))
    eq(got.tsdf, ref64.tsdf), eq(got.weight, ref64.weight), eq(got.color, ref64.color)


def test_bad_weights_skip_and_are_not_counted():
    sc, skin = sr.scene_a(), sr.skin_a()
    H, W = sc.depth.shape
    wim = wr.weight_image(np.random.default_rng(3), H, W)
    bad = ~((wim > 0) & np.isfinite(wim))
    assert 0.15 < bad.mean() < 0.25 and (wim == wr.SUBNORMAL).mean() > 0.03
    plain = sr.two_frame_fusion(sc, skin, sc.state, 1.0)
    got = wr.two_frame_weighted(sc, skin, sc.state, 1.0, wim, 2.5)
    skipped = plain.updated & ~got.updated
    assert skipped.sum() > 100 and bad[plain.py[skipped], plain.px[skipped]].all()
    assert not (got.updated & ~plain.updated).any()
    for now, old in ((got.tsdf, sc.state[0]), (got.weight, sc.state[1]), (got.color, sc.state[2])):
        eq(now[~got.updated], old.reshape(-1)[~got.updated])
    assert got.weight[got.updated].max() == F32(2.5) and (sc.state[1] == 3).any()   # the cap also pulls a weight 3 down


def _one_voxel(dists, w_max, obs=1.0):
    """One voxel at the origin pixel of a 1x1 image, held at SDF dist d (in units of trunc) frame after frame."""
    t, w, c = np.zeros(1, F32), np.zeros(1, F32), np.zeros(1, F32)
    intr = (1.0, 1.0, 0.0, 0.0)
    z = 1.0
    out = []
    for d in dists:
        depth = np.full((1, 1), z + d * wr.TRUNC, F32)
        n = wr.integrate_weighted(t, w, c, np.array([[0, 0, z]], F32), np.ones(1, bool), depth, np.zeros((1, 1), F32),
                                  intr, np.full((1, 1), obs, F32), 1.0, w_max)
        assert n == 1
        out.append((float(t[0]), float(w[0])))
    return out


def test_cap_known_answer():
    """20 frames at d1, then m at d2: with w_max = 4 the voxel follows d2 + (d1 - d2)(4/5)^m, without the cap the
    1 / (20 + m) law, both to f32 rounding."""
    d1, d2, M = 0.5, -0.25, 12
    dists = [d1] * 20 + [d2] * M
    # the depths are f32: the SDF values that really go in
    e1 = (F64(F32(1.0 + d1 * wr.TRUNC)) - 1.0) / wr.TRUNC
    e2 = (F64(F32(1.0 + d2 * wr.TRUNC)) - 1.0) / wr.TRUNC
    capped = _one_voxel(dists, 4.0)
    free = _one_voxel(dists, wr.INF)
    assert [w for _, w in capped[:6]] == [1, 2, 3, 4, 4, 4] and capped[-1][1] == 4
    assert [w for _, w in free] == list(range(1, 21 + M))
    tol = 4 * (20 + M) * 2.0 ** -24     # one f32 rounding per frame, |tsdf| <= 1/2
    for m in range(1, M + 1):
        assert abs(capped[19 + m][0] - (e2 + (e1 - e2) * 0.8 ** m)) < tol, m
        assert abs(free[19 + m][0] - (20 * e1 + m * e2) / (20 + m)) < tol, m
    assert abs(capped[-1][0] - e2) < 0.07 * abs(e1 - e2) < abs(free[-1][0] - e2)   # the capped model has adapted


def test_weight_map_known_answers():
    H, W, intr = 31, 43, (60.0, 60.0, 21.0, 15.0)
    # fronto-parallel at z_ref: exactly 1 away from the border with cos_power 0, and on the optical axis for any power
    # (off the axis the viewing ray tilts against the plane's normal, so the angle term falls below 1 there)
    p, n = wr.plane_maps(H, W, intr, 1.0, 0.0)
    w0 = wr.observation_weights(p, n, 0, 1.0, 0.05, 0.0)
    assert (w0[1:-1, 1:-1] == 1).all() and (w0[0] == 0).all() and (w0[:, -1] == 0).all()
    w2 = wr.observation_weights(p, n, 2, 1.0, 0.05, 0.0)
    assert w2[15, 21] == 1 and (w2[1:-1, 1:-1] <= 1).all() and w2[1, 1] < w2[15, 21]
    # farther than z_ref: (z_ref / z)^2
    p, n = wr.plane_maps(H, W, intr, 2.0, 0.0)
    assert wr.observation_weights(p, n, 0, 1.0, 0.05, 0.0)[15, 21] == F32(0.25)
    assert wr.observation_weights(p, n, 0, 0.0, 0.05, 0.0)[15, 21] == 1      # z_ref = 0: no range term
    # 60 degrees: on the optical axis the angle term is cos 60, its square with power 2
    p, n = wr.plane_maps(H, W, intr, 1.0, 60.0)
    w1 = wr.observation_weights(p, n, 1, 0.0, 0.0, 0.0)
    w2 = wr.observation_weights(p, n, 2, 0.0, 0.0, 0.0)
    assert abs(w1[15, 21] - 0.5) < 1e-5 and abs(w2[15, 21] - 0.25) < 1e-5
    assert abs(float(w2[7, 30]) - float(w1[7, 30]) ** 2) < 1e-6
    # floor, edge weight, holes
    p[:, 10, 10] = 0                              # a hole ...
    n[:, 9:12, 10] = 0                            # ... and its neighbours without a normal
    n[:, 10, 9:12] = 0
    w = wr.observation_weights(p, n, 2, 0.0, 0.4, 0.125)
    assert w[10, 10] == 0 and w[9, 10] == w[10, 11] == F32(0.125) and w[0, 5] == F32(0.125)
    assert w[15, 21] == F32(0.4) and w[1:-1, 1:-1].max() > 0.4
    p[2, 20, 20] = np.nan
    assert wr.observation_weights(p, n, 2, 1.0, 0.05, 0.3)[20, 20] == 0     # NaN z is a hole


def test_benefit_of_the_default_weights():
    """The claim the feature makes, measured by the restatement on wr.benefit_scene(): a spinning sphere whose depth noise
    grows as 1 / cos(theta), fused over nine frames under ground-truth transforms, once as the plain running average and
    once with the default fusion weights. e_u = 1.130 mm, e_w = 0.980 mm (RMS against the noise-free frame 0 over the
    10640 sphere pixels with cos(theta) >= 0.5): 13 % less, the order the weighting algebra predicts for this noise
    model. The scene was written down once and not tuned; wr.E_U / wr.E_W record the two figures for the device test."""
    b = wr.benefit_scene()
    assert int(b.mask.sum()) > 5000 and b.nodes.shape[0] > 200
    d_u, d_w = wr.benefit_fuse(b, None)
    e_u, e_w = wr.benefit_error(b, d_u), wr.benefit_error(b, d_w)
    print(f"benefit scenario: e_u = {1e3 * e_u:.4f} mm, e_w = {1e3 * e_w:.4f} mm, gain {100 * (1 - e_w / e_u):.1f} %")
    assert e_w < e_u
    assert abs(e_u - wr.E_U) < 1e-9 and abs(e_w - wr.E_W) < 1e-9      # the records the device test's bar is made of
