"""CPU: the model z-buffer's entry points exist at every layer — header, library exports, ctypes struct, the
torch.ops.ofx.splat_points schema and fake kernel, and the Python classes and keywords — without a device. ABI version
stays 5."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ofx_splat_create", "ofx_splat_destroy", "ofx_splat_points")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert re.search(r"#define\s+OFX_SPLAT_RMAX\s+4\b", hdr) and _lib.SPLAT_RMAX == 4
    assert _lib.lib.ofx_abi_version() == 5   # entry points and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_splat_params_layout_matches_ctypes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(ofx_splat_params),offsetof(ofx_splat_params,splat_radius),'
                   'offsetof(ofx_splat_params,occl_margin),offsetof(ofx_splat_params,_pad));}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = _lib.SplatParams
    assert c == [ctypes.sizeof(S), S.splat_radius.offset, S.occl_margin.offset, S._pad.offset] == [16, 0, 4, 8]


def test_argument_errors_are_status_codes():
    """Checked before any device work: a null handle out-pointer, a negative or oversized capacity, a null handle."""
    assert _lib.lib.ofx_splat_create(10, 10, None) == -1
    h = ctypes.c_void_p()
    assert _lib.lib.ofx_splat_create(-1, 10, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_splat_create(10, -1, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_splat_create(1 << 31, 10, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_splat_create(10, 1 << 31, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_splat_points(*([None] * 6), 0, None, 0, *([None] * 8)) == -1
    assert b"null handle" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_splat_destroy(None) == 0


def test_splat_points_registered():
    assert "splat_points" in ops.OPS
    sch = str(torch.ops.ofx.splat_points.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::splat_points(Tensor(a0!) state, int handle, Tensor points, Tensor? normals, Tensor anchors, "
                   "Tensor weights, Tensor? valid, Tensor packed_nodes, float[] intr, int height, int width, "
                   "float splat_radius, float occl_margin) -> (Tensor, Tensor, Tensor, Tensor, Tensor)"), sch
    mutated = [a.name for a in torch.ops.ofx.splat_points.default._schema.arguments
               if a.alias_info is not None and a.alias_info.is_write]
    assert mutated == ["state"]


def _args(P, N, device=None, normals=True, valid=True):
    kw = {} if device is None else {"device": device}
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(P, 3, **kw),
            torch.empty(P, 3, **kw) if normals else None, torch.empty(P, 4, dtype=torch.int32, **kw),
            torch.empty(P, 4, **kw), torch.empty(P, dtype=torch.bool, **kw) if valid else None,
            torch.empty(N, 16, **kw), [30.0, 30.0, 19.5, 15.5]]


@pytest.mark.parametrize("P", [8229, 1, 0])
def test_splat_points_fake_kernel(P):
    def want(n):
        return [((32, 40), torch.float32), ((32, 40), torch.int32), ((P,), torch.uint8), ((P, 3), torch.float32),
                ((n, 3), torch.float32)]
    with FakeTensorMode():
        out = torch.ops.ofx.splat_points(*_args(P, 24), 32, 40, 0.004, 0.01)
        assert [(tuple(t.shape), t.dtype) for t in out] == want(P)
        out = torch.ops.ofx.splat_points(*_args(P, 24, normals=False, valid=False), 32, 40, 0.004, 0.01)
        assert [(tuple(t.shape), t.dtype) for t in out] == want(0)   # no normals: an empty warped_normals
    out = torch.ops.ofx.splat_points(*_args(P, 24, device="meta"), 32, 40, 0.004, 0.01)
    assert [(tuple(t.shape), t.dtype) for t in out] == want(P) and all(t.device.type == "meta" for t in out)


def test_splat_points_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.splat_points(*_args(5, 4), 32, 40, 0.004, 0.01)


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd import association
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    from occlusionfusion_amd.warpfield import WarpField
    assert pkg.ModelRenderer is association.ModelRenderer
    assert list(inspect.signature(association.ModelRenderer.__init__).parameters)[1:] == ["max_points", "max_pixels",
                                                                                            "device"]
    sig = inspect.signature(association.ModelRenderer.render)
    assert list(sig.parameters)[1:] == ["points", "normals", "anchors", "weights", "valid", "warpfield_or_packed_nodes",
                                        "intr", "height", "width", "splat_radius", "occl_margin", "normal_map"]
    assert sig.parameters["occl_margin"].default == 0.01 and sig.parameters["normal_map"].default is False
    assert "nothing is\n        read back" in association.ModelRenderer.render.__doc__
    assert association.SPLAT_CODE_NAMES == ("visible", "invalid_skin", "off_image", "back_facing", "occluded")
    for fn in (association.icp_track, Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["occlusion"].default is False and p["splat_radius"].default is None
        assert p["occl_margin"].default == 0.01 and p["assoc"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(association.icp_track).parameters
    assert p["renderer"].default is None
    d = {k: v.default for k, v in inspect.signature(WarpField.render_live).parameters.items() if k != "self"}
    assert d == dict(max_points=65536, w_min=1.0, splat_radius=None, intr=None, height=None, width=None)


def test_occlusion_without_a_renderer_or_a_radius_is_a_value_error():
    from occlusionfusion_amd.association import icp_track
    args = [None] * 12   # refused before anything is touched
    with pytest.raises(ValueError, match="ModelRenderer"):
        icp_track(*args, occlusion=True, splat_radius=0.004)
    with pytest.raises(ValueError, match="splat_radius"):
        icp_track(*args, occlusion=True, renderer=object())


def test_default_splat_radius_rule():
    """The voxel size for a model with normals, half of it without (DESIGN: fronto-parallel discs of a full voxel read
    17.5 % of config 1's own model as occluded, 4.7 % at half)."""
    from occlusionfusion_amd.association import default_splat_radius
    assert default_splat_radius(0.008, True) == 0.008
    assert default_splat_radius(0.008, False) == 0.004
