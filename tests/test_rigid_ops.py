"""CPU: the rigid pre-alignment entry points exist at every layer — header, library exports, ctypes struct, the
torch.ops.ofx.rigid_icp schema (pose declared mutated) and fake kernel, and the Python layers — without a device. ABI
version stays 5."""
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
NAMES = ("ofx_rigid_create", "ofx_rigid_destroy", "ofx_rigid_icp")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert len(_lib._SIGS["ofx_rigid_icp"]) == 18
    assert _lib.lib.ofx_abi_version() == 5   # entry points and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_rigid_params_layout_matches_ctypes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(ofx_rigid_params),offsetof(ofx_rigid_params,iters),offsetof(ofx_rigid_params,min_matches),'
                   'offsetof(ofx_rigid_params,damping),offsetof(ofx_rigid_params,stop_twist));}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    R = _lib.RigidParams
    assert c == [ctypes.sizeof(R), R.iters.offset, R.min_matches.offset, R.damping.offset, R.stop_twist.offset]
    assert c == [40, 12, 16, 24, 32]


def test_argument_errors_are_status_codes():
    """Checked before any device work: a null handle out-pointer, a negative or oversized capacity, a null handle."""
    assert _lib.lib.ofx_rigid_create(10, None) == -1
    h = ctypes.c_void_p()
    assert _lib.lib.ofx_rigid_create(-1, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_rigid_create(1 << 31, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_rigid_icp(*([None] * 6), 0, None, 0, None, None, 0, 0, *([None] * 5)) == -1
    assert b"null handle" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_rigid_destroy(None) == 0


def test_rigid_icp_registered_with_pose_mutated():
    assert "rigid_icp" in ops.OPS
    sch = str(torch.ops.ofx.rigid_icp.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::rigid_icp(Tensor(a0!) state, int handle, Tensor points, Tensor? normals, Tensor anchors, "
                   "Tensor weights, Tensor? valid, Tensor packed_nodes, Tensor point_image, float[] intr, "
                   "float dist_max, float cos_min, float edge_max, int iters, int min_matches, float damping, "
                   "float stop_twist, Tensor(a17!) pose) -> (Tensor, Tensor)"), sch
    mutated = [a.name for a in torch.ops.ofx.rigid_icp.default._schema.arguments
               if a.alias_info is not None and a.alias_info.is_write]
    assert mutated == ["state", "pose"]


def _args(P, N, H, W, iters, device=None, normals=True, valid=True):
    kw = {} if device is None else {"device": device}
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(P, 3, **kw),
            torch.empty(P, 3, **kw) if normals else None, torch.empty(P, 4, dtype=torch.int32, **kw),
            torch.empty(P, 4, **kw), torch.empty(P, dtype=torch.bool, **kw) if valid else None,
            torch.empty(N, 16, **kw), torch.empty(3, H, W, **kw), [30.0, 30.0, 19.5, 15.5], 0.05, 0.5, 0.03, iters, 6,
            1e-6, 0.0, torch.zeros(3, 4, dtype=torch.float64, **kw)]


@pytest.mark.parametrize("P,iters", [(8229, 4), (1, 1), (0, 3)])
def test_rigid_icp_fake_kernel(P, iters):
    want = [((P,), torch.uint8), ((iters, 32), torch.float64)]
    with FakeTensorMode():
        out = torch.ops.ofx.rigid_icp(*_args(P, 24, 32, 40, iters))
        assert [(tuple(t.shape), t.dtype) for t in out] == want
        out = torch.ops.ofx.rigid_icp(*_args(P, 24, 32, 40, iters, normals=False, valid=False))
        assert [(tuple(t.shape), t.dtype) for t in out] == want
    out = torch.ops.ofx.rigid_icp(*_args(P, 24, 32, 40, iters, device="meta"))
    assert [(tuple(t.shape), t.dtype) for t in out] == want and all(t.device.type == "meta" for t in out)


def test_rigid_icp_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.rigid_icp(*_args(5, 4, 32, 40, 2))


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd import association
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    assert pkg.RigidAligner is association.RigidAligner and pkg.fold_rigid is association.fold_rigid
    sig = inspect.signature(association.RigidAligner.align)
    assert list(sig.parameters)[1:10] == ["points", "normals", "anchors", "weights", "valid",
                                          "warpfield_or_packed_nodes", "point_image", "intr", "pose"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(pose=None, iters=4, dist_max=0.05, cos_min=0.5, edge_max=0.03, damping=1e-6, min_matches=6,
                     stop_twist=0.0, sync=False)
    for fn in (association.icp_track, Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["rigid_iters"].default == 0 and p["rigid_iters"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert p["assoc"].kind is inspect.Parameter.VAR_KEYWORD


def test_fold_rigid_on_cpu_tensors_equals_the_restatement():
    """fold_rigid is plain tensor arithmetic on the pose's device: checked here against tests/rigid_ref.py's."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import rigid_ref as rr
    from occlusionfusion_amd.association import fold_rigid
    rng = np.random.default_rng(2)
    nodes = rng.normal(0, 0.4, (30, 3)).astype(np.float32)
    R = rr.fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.1, (30, 3))).astype(np.float32)
    T = rng.normal(0, 0.01, (30, 3)).astype(np.float32)
    pose = rr.rigid_about((0.3, 1.0, 0.2), 3.0, (0, 0, 1.3), (0.012, -0.008, 0.0139))
    for rot, trans in ((R, T), (None, None), (R, None)):
        want_R, want_T = rr.fold_rigid(nodes, rot, trans, pose)
        got_R, got_T = fold_rigid(nodes, rot, trans, torch.from_numpy(pose))
        assert got_R.dtype == torch.float32 and got_T.dtype == torch.float32
        # f64 products summed in a different order, then one rounding to f32: at most one f32 ulp apart
        assert np.abs(got_R.numpy() - want_R).max() <= np.spacing(np.float32(1.0))
        assert np.abs(got_T.numpy() - want_T).max() <= np.spacing(np.float32(np.abs(want_T).max()))
