"""CPU: the projective-association entry points exist at every layer — header, library exports, ctypes struct, the
torch.ops.ofx.associate schema and fake kernel, and the Python classes — without a device. ABI version stays 5."""
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
NAMES = ("ofx_assoc_create", "ofx_assoc_destroy", "ofx_associate")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert re.search(r"OFX_ASSOC_POINT\s*=\s*0\s*,\s*OFX_ASSOC_PLANE\s*=\s*1", hdr)
    assert _lib.lib.ofx_abi_version() == 5   # entry points and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_assoc_params_layout_matches_ctypes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(ofx_assoc_params),offsetof(ofx_assoc_params,edge_max),offsetof(ofx_assoc_params,mode),'
                   'offsetof(ofx_assoc_params,max_matches));}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    A = _lib.AssocParams
    assert c == [ctypes.sizeof(A), A.edge_max.offset, A.mode.offset, A.max_matches.offset] == [24, 8, 12, 16]


def test_argument_errors_are_status_codes():
    """Checked before any device work: a null handle out-pointer, a negative or oversized capacity."""
    assert _lib.lib.ofx_assoc_create(10, None) == -1
    h = ctypes.c_void_p()
    assert _lib.lib.ofx_assoc_create(-1, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_assoc_create(1 << 31, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_associate(*([None] * 6), 0, None, 0, None, None, 0, 0, *([None] * 11)) == -1
    assert _lib.lib.ofx_assoc_destroy(None) == 0


def test_associate_registered():
    assert "associate" in ops.OPS
    sch = str(torch.ops.ofx.associate.default._schema).replace("SymInt", "int")   # (how the schema prints an int)
    assert sch.startswith("ofx::associate(Tensor(a0!) state, int handle, Tensor points, Tensor? normals, Tensor anchors, "
                          "Tensor weights, Tensor? valid, Tensor packed_nodes, Tensor point_image, float[] intr, "
                          "float dist_max, float cos_min, float edge_max, int target_mode, int max_matches)"), sch
    assert sch.count("!") == 1 and sch.endswith("-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")


def _args(P, N, H, W, device=None, normals=True, valid=True):
    kw = {} if device is None else {"device": device}
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(P, 3, **kw),
            torch.empty(P, 3, **kw) if normals else None, torch.empty(P, 4, dtype=torch.int32, **kw),
            torch.empty(P, 4, **kw), torch.empty(P, dtype=torch.bool, **kw) if valid else None,
            torch.empty(N, 16, **kw), torch.empty(3, H, W, **kw), [30.0, 30.0, 19.5, 15.5], 0.05, 0.5, 0.03, 1]


@pytest.mark.parametrize("P,M", [(8229, 1000), (1, 10), (0, 5)])
def test_associate_fake_kernel(P, M):
    want = [((P,), torch.uint8), ((P, 3), torch.float32), ((P, 3), torch.float32), ((M,), torch.int32),
            ((M, 3), torch.float32), ((M, 3), torch.float32), ((M, 4), torch.int32), ((M, 4), torch.float32),
            ((2,), torch.int32)]
    with FakeTensorMode():
        out = torch.ops.ofx.associate(*_args(P, 24, 32, 40), M)
        assert [(tuple(t.shape), t.dtype) for t in out] == want
        out = torch.ops.ofx.associate(*_args(P, 24, 32, 40, normals=False, valid=False), M)
        assert [(tuple(t.shape), t.dtype) for t in out] == want
    out = torch.ops.ofx.associate(*_args(P, 24, 32, 40, device="meta"), M)
    assert [(tuple(t.shape), t.dtype) for t in out] == want and all(t.device.type == "meta" for t in out)


def test_associate_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.associate(*_args(5, 4, 32, 40), 10)


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd import association
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    assert pkg.ProjectiveAssociator is association.ProjectiveAssociator
    sig = inspect.signature(association.ProjectiveAssociator.associate)
    assert list(sig.parameters)[1:9] == ["points", "normals", "anchors", "weights", "valid", "warpfield_or_packed_nodes",
                                         "point_image", "intr"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(dist_max=0.05, cos_min=0.5, edge_max=0.03, mode="plane", max_matches=10000)
    assert "host sync" in association.ProjectiveAssociator.associate.__doc__
    sig = inspect.signature(Registration.track)
    assert list(sig.parameters)[1:5] == ["target_frame_data", "complete_node_motion_data", "source_normals", "icp_iters"]
    assert sig.parameters["icp_iters"].default == 3 and sig.parameters["complete_node_motion_data"].default is None
    assert callable(FusionPipeline.track_step)
    assert issubclass(association.TooFewMatches, RuntimeError)
