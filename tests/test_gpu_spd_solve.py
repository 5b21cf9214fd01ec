"""GPU: the dense f64 SPD solve (ofx_spd_solve through torch.ops.ofx.spd_solve: right-looking blocked Cholesky, 64-column
panels, the right-hand side carried as an extra row, the backward solve in both its forms) against
scipy.linalg.cho_solve in f64 on the host.

Sizes sit below, at and just past one and two panels (and 258, 390: multiples of 6 as the Gauss-Newton systems are);
A = Q diag(d) Qᵀ with d log-spaced, so cond₂ is known by construction. Bounds: the textbook forward bound of a
backward-stable solve, max|x − x_ref| / max|x_ref| <= 16·n·2⁻⁵³·cond₂, and the factor's backward error
max|LLᵀ − A| <= 8·n·2⁻⁵³·max|A| on the lower triangle. The worst measured ratio of each to its bound is printed.
"""
import numpy as np
import pytest
import scipy.linalg as sl
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SIZES = [1, 5, 63, 64, 65, 129, 258, 390]
CONDS = [1e2, 1e6]
_WORST = {"x": 0.0, "L": 0.0}


def _spd(n, cond, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, -np.log10(cond), n) if n > 1 else np.ones(1)
    A = (Q * d) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(n)
    return A, b, Q, d


def _ref(A, b):
    return sl.cho_solve(sl.cho_factor(A, lower=True), b)


def _solve(A, b, dev, pad=0, nan_upper=False):
    from occlusionfusion_amd import ops  # noqa: F401  (registers torch.ops.ofx.*)
    n = A.shape[0]
    Ah = A.copy()
    if nan_upper:
        Ah[np.triu_indices(n, 1)] = np.nan
    buf = torch.zeros((n, n + pad), dtype=torch.float64, device=dev)
    At = buf[:, :n]
    At.copy_(torch.from_numpy(Ah))
    assert At.stride(0) == n + pad or (pad == 0 and n == 1)
    L, x, st = torch.ops.ofx.spd_solve(At, torch.from_numpy(b).to(dev))
    torch.cuda.synchronize()
    return L.cpu().numpy(), x.cpu().numpy(), st.cpu().numpy()


def _check(A, b, cond, L, x, st):
    n = A.shape[0]
    assert st[0] == 0, st
    if n == 1:
        cond = 1.0   # (a 1 x 1 matrix has no spread to construct)
    xr = _ref(A, b)
    ex = np.abs(x - xr).max() / np.abs(xr).max()
    bx = 16 * n * EPS * cond
    Ll = np.tril(L)
    tl = np.tril_indices(n)
    eL = np.abs((Ll @ Ll.T - A)[tl]).max()
    bL = 8 * n * EPS * np.abs(A).max()
    _WORST["x"] = max(_WORST["x"], ex / bx)
    _WORST["L"] = max(_WORST["L"], eL / bL)
    print(f"spd_solve n={n} cond={cond:g}: x err/bound = {ex / bx:.3e}, LLt err/bound = {eL / bL:.3e} "
          f"(worst so far {_WORST['x']:.3e}, {_WORST['L']:.3e})")
    assert ex <= bx, (n, cond, ex, bx)
    assert eL <= bL, (n, cond, eL, bL)


@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("n", SIZES)
def test_spd_solve_matches_scipy(cuda, n, cond):
    A, b, _, _ = _spd(n, cond)
    _check(A, b, cond, *_solve(A, b, cuda))


@pytest.mark.parametrize("n", SIZES)
def test_spd_solve_padded_stride(cuda, n):
    """lda = n + 3: the same solve, bit for bit (the row stride only moves the rows)."""
    A, b, _, _ = _spd(n, 1e6)
    L0, x0, _ = _solve(A, b, cuda)
    L, x, st = _solve(A, b, cuda, pad=3)
    _check(A, b, 1e6, L, x, st)
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(np.tril(L), np.tril(L0))


@pytest.mark.parametrize("n", [5, 65, 258])
def test_spd_solve_reads_only_the_lower_triangle(cuda, n):
    A, b, _, _ = _spd(n, 1e2)
    L0, x0, st0 = _solve(A, b, cuda)
    L, x, st = _solve(A, b, cuda, nan_upper=True)
    assert st[0] == 0 and st0[0] == 0
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(np.tril(L), np.tril(L0))
    assert np.isnan(L[np.triu_indices(n, 1)]).all()   # the strict upper triangle is left as given


def test_spd_solve_flags_an_indefinite_matrix(cuda):
    n = 65
    _, b, Q, d = _spd(n, 1e2)
    d = d.copy()
    d[40] = -d[40]
    A = (Q * d) @ Q.T
    A = 0.5 * (A + A.T)
    _, x, st = _solve(A, b, cuda)
    assert st[0] == 1 and 0 <= st[1] < n, st
    assert not x.any()


def test_spd_solve_flags_a_non_finite_pivot(cuda):
    A, b, _, _ = _spd(129, 1e2)
    A[70, 70] = np.inf
    _, x, st = _solve(A, b, cuda)
    assert st[0] == 1 and st[1] == 70, st
    assert not x.any()


@pytest.mark.parametrize("n", [65, 390])
def test_spd_solve_is_bitwise_repeatable(cuda, n):
    A, b, _, _ = _spd(n, 1e6)
    L0, x0, _ = _solve(A, b, cuda)
    L1, x1, _ = _solve(A, b, cuda)
    np.testing.assert_array_equal(L0, L1)
    np.testing.assert_array_equal(x0, x1)


@pytest.mark.parametrize("form", ["sweep", "panel"])
@pytest.mark.parametrize("n", [1, 64, 65, 129, 390])
def test_spd_solve_both_backward_forms(cuda, n, form, monkeypatch):
    """OFX_DENSE_BACK: the one-workgroup sweep and the one-launch-per-panel form of the backward solve meet the same
    bounds, each bitwise repeatable; the factor does not depend on the form."""
    A, b, _, _ = _spd(n, 1e6)
    L0, _, _ = _solve(A, b, cuda)
    monkeypatch.setenv("OFX_DENSE_BACK", form)
    L, x, st = _solve(A, b, cuda)
    _check(A, b, 1e6, L, x, st)
    L1, x1, _ = _solve(A, b, cuda)
    np.testing.assert_array_equal(x, x1)
    np.testing.assert_array_equal(L, L0)
    np.testing.assert_array_equal(L, L1)


@pytest.mark.parametrize("form", ["sweep", "panel"])
def test_spd_solve_indefinite_under_both_backward_forms(cuda, form, monkeypatch):
    monkeypatch.setenv("OFX_DENSE_BACK", form)
    _, b, Q, d = _spd(129, 1e2)
    d = d.copy()
    d[100] = -d[100]
    A = (Q * d) @ Q.T
    _, x, st = _solve(0.5 * (A + A.T), b, cuda)
    assert st[0] == 1 and 0 <= st[1] < 129 and not x.any()


@pytest.mark.parametrize("n", [0, 3073])
def test_spd_solve_range(cuda, n):
    from occlusionfusion_amd import ops  # noqa: F401
    from occlusionfusion_amd._lib import OfxError
    A = torch.eye(n, dtype=torch.float64, device=cuda)
    with pytest.raises(OfxError, match="3072"):
        torch.ops.ofx.spd_solve(A, torch.zeros(n, dtype=torch.float64, device=cuda))


def test_spd_solve_wrapper(cuda):
    """occlusionfusion_amd.spd_solve takes host arrays."""
    from occlusionfusion_amd import spd_solve
    A, b, _, _ = _spd(65, 1e2)
    L, x, st = spd_solve(A, b)
    _check(A, b, 1e2, L.cpu().numpy(), x.cpu().numpy(), st.cpu().numpy())
