"""CPU: the numpy restatement of the sub-pixel refinement (tests/refine_ref.py) against known answers.

* a template that shows a smooth analytic texture shifted by (0.3, -0.45) px is recovered to within the texture's
  interpolation error, with the bound derived from the texture's second derivatives;
* small_case reaches every status code for half 1, 3 and 4, has a count that is no multiple of 8, and no row of it sits
  within 1e-6 (relative) of a deciding threshold — so the GPU parity test may compare every row's status;
* rows that are not refined equal their inputs; rows past the count are untouched; a count of 0 writes nothing.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as rr  # noqa: E402

HALVES = (1, 3, 4)
_CASES = {}


def _case(half):
    """small_case(half) and its restated outputs, computed once and shared (never modified)."""
    if half not in _CASES:
        c = rr.small_case(half)
        pre = dict(px_out=np.full((300, 2), -7.0, np.float32), tgt_out=np.full((300, 3), -7.0, np.float32),
                   status=np.full(300, 99, np.uint8), ssd=np.full(300, -7.0, np.float32))
        _CASES[half] = (c, rr.refine(c["template_image"], c["template_mask"], c["color_image"], c["point_image"],
                                     c["template_px"], c["init_px"], c["tgt_in"], c["count"], c["edge_max"],
                                     outputs=pre, **c["params"]))
    return _CASES[half]


@pytest.mark.parametrize("half", HALVES)
def test_known_shift_is_recovered_within_the_interpolation_error(half):
    """Texture, per channel c: f_c(x, y) = a_c + p_c·x + q_c·y + k_c·x² + m_c·y² — smooth, with the constant second
    derivatives f_xx = 2·k_c, f_yy = 2·m_c and no mixed term. The live image samples f on the pixel grid; the template
    samples f(x + 0.3, y - 0.45), so the template patch at t matches the live frame at u* = t + (0.3, -0.45) exactly, as
    functions. What the refinement sees are bilinear interpolants. On a unit cell the interpolant of f_c is off by at
    most E_c = (|f_xx| + |f_yy|)/8 = (k_c + m_c)/4 (the classical bound: fx(1 - fx)/2·|f_xx| <= |f_xx|/8 per axis), and
    that error is the same at x - 1, x and x + 1 (the same fraction), so the central differences g are the texture's
    exact gradient at the tap. At the fixed point sum g·r = 0 with r(d) = grad f(xi_d)·delta + (e_live - e_template),
    |e_live - e_template| <= 2·E_c, so delta = -G^-1 sum g·e with G = sum g·grad f(xi)^T, which is H up to the change
    of the gradient over |delta| (relative 2·k·|delta|/|g|, far below the 1 % allowed for it here). By Cauchy-Schwarz
    |delta| <= sqrt(tr H)·sqrt(sum e²)/lambda_min(H) <= sqrt(tr H)·sqrt(n_taps·sum_c (2·E_c + 2^-22)²)/lambda_min(H);
    the 2^-22 covers the f32 rounding of the two samples (values below 2, five operations of half an ulp each)."""
    H, W = 32, 40
    coef = np.array([[0.30, 0.020, 0.004, 1.0e-4, 0.5e-4],      # a, p, q, k, m per channel
                     [0.60, -0.005, 0.020, 0.5e-4, 1.0e-4],
                     [0.20, 0.015, 0.015, 0.8e-4, 0.8e-4]])
    shift = np.array([0.3, -0.45])

    def f(x, y):
        return np.stack([a + p * x + q * y + k * x * x + m * y * y for a, p, q, k, m in coef])
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    live = f(uu, vv).astype(np.float32)
    timg = f(uu + shift[0], vv + shift[1]).astype(np.float32)
    assert live.max() < 2 and live.min() > 0
    rng = np.random.default_rng(3)
    R = 64
    tpx = np.stack([rng.uniform(8, W - 9, R), rng.uniform(8, H - 9, R)], 1).astype(np.float32)
    tpx[:8] = np.rint(tpx[:8])                                   # some template pixels on the grid
    ipx = np.rint(tpx + shift + rng.uniform(-0.7, 0.7, (R, 2))).astype(np.float32)
    vm = np.stack([(uu - 19.5) / 30, (vv - 15.5) / 30, np.ones_like(uu)]).astype(np.float32)
    out = rr.refine(timg, None, live, vm, tpx, ipx, np.zeros((R, 3), np.float32), [R, R], 0.03, half=half, iters=8,
                    eps=0.0, max_shift=4.0, min_eig=0.0, ssd_max=np.inf)
    assert np.all(out["status"] == 0)
    # the bound, from the analytic gradient at the taps of each row
    w = 2 * half + 1
    dy, dx = np.divmod(np.arange(w * w), w)
    x = tpx[:, 0, None].astype(np.float64) + shift[0] + (dx - half)[None]
    y = tpx[:, 1, None].astype(np.float64) + shift[1] + (dy - half)[None]
    gx = np.stack([p + 2 * k * x for a, p, q, k, m in coef])     # (3, R, taps)
    gy = np.stack([q + 2 * m * y for a, p, q, k, m in coef])
    hxx, hxy, hyy = (gx * gx).sum((0, 2)), (gx * gy).sum((0, 2)), (gy * gy).sum((0, 2))
    lmin = 0.5 * ((hxx + hyy) - np.sqrt((hxx - hyy) ** 2 + 4 * hxy * hxy))
    E = (coef[:, 3] + coef[:, 4]) / 4
    bound = 1.01 * np.sqrt(hxx + hyy) * np.sqrt(w * w * ((2 * E + 2.0 ** -22) ** 2).sum()) / lmin
    err = np.linalg.norm(out["px_out"].astype(np.float64) - (tpx.astype(np.float64) + shift), axis=1)
    print(f"half {half}: |u - u*| max {err.max():.2e} px, bound min {bound.min():.2e} max {bound.max():.2e} px")
    assert bound.max() < 0.1                                     # the bound says something: well below a pixel
    assert np.all(err <= bound), (err.max(), bound.min())
    # the target is the vertex map at the refined pixel: here an affine map, which bilinear interpolation reproduces
    want = np.stack([(out["px_out"][:, 0] - 19.5) / 30, (out["px_out"][:, 1] - 15.5) / 30, np.ones(R)], 1)
    assert np.abs(out["tgt_out"] - want).max() < 1e-6


@pytest.mark.parametrize("half", HALVES)
def test_small_case_reaches_every_status_and_no_row_sits_on_a_threshold(half):
    c, out = _case(half)
    n = int(c["count"][1])
    assert n % 8 != 0 and 0 < n < c["init_px"].shape[0] and c["count"][0] > n
    hist = np.bincount(out["status"][:n], minlength=8)
    print(f"half {half}: status histogram {hist.tolist()}, smallest margin {out['margin'].min():.3e}")
    assert hist.shape == (8,) and np.all(hist > 0), hist
    assert hist[0] >= n // 3                                     # and a good share of the rows is refined
    assert out["margin"][:n].min() >= 1e-6                       # (what lets the GPU test compare every status)
    assert np.isinf(out["margin"][n:]).all()


@pytest.mark.parametrize("half", HALVES)
def test_fallback_rows_equal_their_inputs_and_rows_past_the_count_are_untouched(half):
    c, out = _case(half)
    n = int(c["count"][1])
    st = out["status"][:n]
    fb = st != 0
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731  (NaN inputs compare by their bits)
    assert np.array_equal(bits(out["px_out"][:n][fb]), bits(c["init_px"][:n][fb]))
    assert np.array_equal(bits(out["tgt_out"][:n][fb]), bits(c["tgt_in"][:n][fb]))
    good = ~fb
    moved = np.abs(out["px_out"][:n][good] - c["init_px"][:n][good]).max(1)
    assert np.all(moved <= c["params"]["max_shift"]) and np.median(moved) > 0.05
    # refined rows land on the answer: the template pixel moved by the case's field (0.35, -0.25) ± 0.1, plus noise
    err = out["px_out"][:n][good] - (c["template_px"][:n][good] + np.array(c["shift"], np.float32))
    assert np.median(np.abs(err)) < 0.15
    assert np.all(out["ssd"][:n][np.isin(st, (1, 2, 3, 4, 5))] == 0) and np.all(out["ssd"][:n][st == 6] > 0.05 ** 2)
    assert np.all(out["ssd"][:n][good] <= 0.05 ** 2)
    # past the count: the prefilled values
    assert np.all(out["px_out"][n:] == -7) and np.all(out["tgt_out"][n:] == -7) and np.all(out["status"][n:] == 99)
    assert np.all(out["ssd"][n:] == -7)


def test_count_zero_and_clamped_counts():
    c, full = _case(3)
    args = (c["template_image"], c["template_mask"], c["color_image"], c["point_image"], c["template_px"], c["init_px"],
            c["tgt_in"])
    pre = dict(px_out=np.full((300, 2), -7.0, np.float32), tgt_out=np.full((300, 3), -7.0, np.float32),
               status=np.full(300, 99, np.uint8), ssd=np.full(300, -7.0, np.float32))
    for cnt in ([0, 0], [5, -3]):
        out = rr.refine(*args, cnt, c["edge_max"], outputs=pre, **c["params"])
        assert all(np.array_equal(out[k], pre[k]) for k in pre)
    out = rr.refine(*args, [400, 400], c["edge_max"], outputs=pre, **c["params"])   # clamped to the rows there are
    n = int(c["count"][1])
    assert np.all(out["status"] != 99) and np.array_equal(out["status"][:n], full["status"][:n])


def test_no_mask_is_a_mask_of_ones_and_the_gates_switch_off():
    c, full = _case(3)
    args = (c["template_image"], c["color_image"], c["point_image"], c["template_px"], c["init_px"], c["tgt_in"],
            c["count"], c["edge_max"])
    a = rr.refine(args[0], None, *args[1:], **c["params"])
    b = rr.refine(args[0], np.ones_like(c["template_mask"]), *args[1:], **c["params"])
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("px_out", "tgt_out", "status", "ssd"))
    n = int(c["count"][1])
    assert (a["status"][:n] == 2).sum() < (full["status"][:n] == 2).sum()        # the mask's hole is gone
    off = rr.refine(args[0], c["template_mask"], *args[1:], **dict(c["params"], ssd_max=np.inf))
    assert not (off["status"] == 6).any()
    was6 = full["status"][:n] == 6
    assert np.all(np.isin(off["status"][:n][was6], (0, 7)))
