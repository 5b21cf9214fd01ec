"""CPU: torch.ops.ofx.spd_solve is registered without mutations and its fake kernel propagates shapes and dtypes on meta
tensors; the C ABI exports ofx_spd_solve and ofx_gn_solver_info; precond="direct" maps to OFX_PRECOND_DIRECT."""
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, ops


def test_spd_solve_registered():
    assert "spd_solve" in ops.OPS
    sch = str(torch.ops.ofx.spd_solve.default._schema)
    assert sch.startswith("ofx::spd_solve(Tensor A, Tensor b)") and "!" not in sch, sch


@pytest.mark.parametrize("n", [1, 65, 390])
def test_spd_solve_fake_kernel(n):
    with FakeTensorMode():
        L, x, st = torch.ops.ofx.spd_solve(torch.empty(n, n, dtype=torch.float64), torch.empty(n, dtype=torch.float64))
        assert (L.shape, L.dtype, x.shape, x.dtype, st.shape, st.dtype) == \
            ((n, n), torch.float64, (n,), torch.float64, (2,), torch.int32)
    L, x, st = torch.ops.ofx.spd_solve(torch.empty(n, n, dtype=torch.float64, device="meta"),
                                       torch.empty(n, dtype=torch.float64, device="meta"))
    assert L.shape == (n, n) and x.shape == (n,) and st.dtype == torch.int32 and L.device.type == "meta"


def test_spd_solve_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.spd_solve(torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))


def test_new_entry_points_exported():
    for name in ("ofx_spd_solve", "ofx_gn_solver_info"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib, name)
    assert _lib.lib.ofx_abi_version() == 5   # entry points and an enum value only: no struct changed


def test_spd_solve_range_is_a_status_code():
    """n outside [1, 3072] comes back as OFX_ERR_RANGE before any pointer is touched (no GPU work)."""
    for n in (0, 3073, -1):
        assert _lib.lib.ofx_spd_solve(None, n, max(n, 1), None, None, None) == -3
        assert b"3072" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_spd_solve(None, 8, 8, None, None, None) == -1   # null buffers: OFX_ERR_ARG


def test_direct_is_a_precond_choice():
    from occlusionfusion_amd.registration import GN_DEFAULTS, _PRECOND
    assert _PRECOND["direct"] == 3 and GN_DEFAULTS["precond"] == "auto"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ofx.h")).read()
    assert re.search(r"OFX_PRECOND_DIRECT\s*=\s*3", hdr)
