"""CPU: the surface-point sampler exists at every layer — header, library exports, ctypes signatures, the
torch.ops.ofx.surface_points schema and fake kernel, and the Python classes — without a device. ABI version stays 5."""
import ctypes
import inspect
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ofx_surface_create", "ofx_surface_destroy", "ofx_surface_points")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert len(_lib._SIGS["ofx_surface_points"]) == 20
    assert _lib.lib.ofx_abi_version() == 5   # entry points only: no struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


def test_argument_errors_are_status_codes():
    """Checked before any device work: a null handle out-pointer, a negative or oversized capacity, a null handle."""
    assert _lib.lib.ofx_surface_create(10, None) == -1
    h = ctypes.c_void_p()
    assert _lib.lib.ofx_surface_create(-1, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_surface_create(1 << 22, ctypes.byref(h)) == -3 and not h.value
    assert b"int32" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_surface_points(*([None] * 5), 0, None, None, 4, 1.0, 0, *([None] * 9)) == -1
    assert _lib.lib.ofx_surface_destroy(None) == 0


def test_surface_points_registered():
    assert "surface_points" in ops.OPS
    sch = str(torch.ops.ofx.surface_points.default._schema).replace("SymInt", "int")
    assert sch.startswith("ofx::surface_points(Tensor(a0!) state, int handle, Tensor tsdf, Tensor weight, "
                          "Tensor brick_list, int n_list, Tensor skin_anchors, Tensor skin_weights, int k, int[] dims, "
                          "float[] origin, float voxel_size, float trunc_margin, float w_min, "), sch
    for name in ("points", "normals", "anchors_out", "weights_out", "voxel", "valid", "count"):
        assert re.search(rf"Tensor\(a\d+!\) {name}\b", sch), (name, sch)
    assert re.search(r"Tensor\(a\d+!\)\? code\b", sch), sch
    assert sch.count("!") == 9 and sch.endswith("-> ()")


def _args(M, n_list, device=None, code=True):
    kw = {} if device is None else {"device": device}
    outs = ops.surface_outputs(M, device if device is not None else "cpu", n_list if code else None)
    n = max(1, n_list) * 512
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(27 * 512, **kw), torch.empty(27 * 512, **kw),
            torch.empty(max(1, n_list), dtype=torch.int32, **kw), n_list, torch.empty(n * 4, dtype=torch.int16, **kw),
            torch.empty(n * 4, **kw), 4, [20, 18, 22], [0.0, 0.0, 0.0], 0.01, 0.04, 1.0, *outs], outs


@pytest.mark.parametrize("M,n_list", [(1000, 27), (1, 1), (0, 0)])
def test_output_shapes_and_fake_kernel(M, n_list):
    want = [((M, 3), torch.float32), ((M, 3), torch.float32), ((M, 4), torch.int32), ((M, 4), torch.float32),
            ((M,), torch.int32), ((M,), torch.uint8), ((max(1, n_list) * 512,), torch.uint8), ((2,), torch.int32)]
    with FakeTensorMode():
        args, outs = _args(M, n_list)
        assert [(tuple(t.shape), t.dtype) for t in outs] == want
        assert torch.ops.ofx.surface_points(*args) is None
        args, outs = _args(M, n_list, code=False)
        assert outs[6] is None and torch.ops.ofx.surface_points(*args) is None
    args, outs = _args(M, n_list, device="meta")
    assert torch.ops.ofx.surface_points(*args) is None and all(t.device.type == "meta" for t in outs)


def test_surface_points_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.surface_points(*_args(10, 27)[0])


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd import surface
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    from occlusionfusion_amd.warpfield import WarpField
    assert pkg.SurfaceSampler is surface.SurfaceSampler and len(surface.CODE_NAMES) == 8
    sig = inspect.signature(WarpField.surface_points)
    assert list(sig.parameters)[1:] == ["max_points", "w_min", "with_codes", "sync"]
    assert {k: v.default for k, v in list(sig.parameters.items())[2:]} == dict(w_min=1.0, with_codes=False, sync=True)
    sig = inspect.signature(Registration.update_from_volume)
    assert {k: v.default for k, v in list(sig.parameters.items())[1:]} == dict(max_points=None, w_min=1.0)
    sig = inspect.signature(FusionPipeline.track_step)
    assert sig.parameters["model"].default == "canonical" and "max_model_points" in sig.parameters
    assert "overlap does not apply" in FusionPipeline.track_step.__doc__
