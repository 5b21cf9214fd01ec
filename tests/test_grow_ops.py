"""CPU: graph growth exists at every layer — header, library exports, ctypes signatures, the torch.ops.ofx.grow_nodes
schema and fake kernel, and the Python classes — without a device. ABI version stays 5."""
import ctypes
import inspect
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ofx_grow_create", "ofx_grow_destroy", "ofx_grow_nodes", "ofx_skin_grow_plan", "ofx_skin_grow_apply")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    assert len(_lib._SIGS["ofx_grow_nodes"]) == 19
    assert (len(_lib._SIGS["ofx_skin_grow_plan"]), len(_lib._SIGS["ofx_skin_grow_apply"])) == (12, 14)
    assert _lib.lib.ofx_abi_version() == 5   # entry points only: no struct changed


def test_argument_errors_are_status_codes():
    """Checked before any device work: a null handle out-pointer, negative or oversized capacities, a null handle."""
    assert _lib.lib.ofx_grow_create(10, 10, None) == -1
    h = ctypes.c_void_p()
    assert _lib.lib.ofx_grow_create(-1, 10, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_grow_create(10, -1, ctypes.byref(h)) == -1 and not h.value
    assert _lib.lib.ofx_grow_create(65537, 10, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_grow_create(10, 4097, ctypes.byref(h)) == -3 and not h.value
    assert b"4096" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_grow_nodes(*([None] * 5), 0, None, 1, *([None] * 4), 8, 0.02, 0.04, 0.02, 0, None, None) == -1
    assert _lib.lib.ofx_grow_destroy(None) == 0
    d = _lib.VolumeDesc()
    d.dim[:] = [20, 18, 22]
    d.brick_x0, d.brick_x1, d.voxel_size = 0, 3, 0.01
    assert _lib.lib.ofx_skin_grow_plan(ctypes.byref(d), None, 14, None, 0.02, 4, None, 0, None, None, None, None) == -1
    assert _lib.lib.ofx_skin_grow_apply(ctypes.byref(d), None, 14, 0.02, 4, None, None, 1, *([None] * 6)) == -1
    assert _lib.lib.ofx_skin_grow_apply(None, None, 14, 0.02, 4, None, None, 0, *([None] * 6)) == -1


def test_grow_nodes_registered():
    assert "grow_nodes" in ops.OPS
    sch = str(torch.ops.ofx.grow_nodes.default._schema).replace("SymInt", "int")
    assert sch.startswith("ofx::grow_nodes(Tensor(a0!) state, int handle, Tensor points, Tensor anchors, Tensor weights, "
                          "Tensor valid, Tensor(a6!) nodes, int n_nodes, "), sch
    for name in ("nodes", "rotations", "translations", "edges", "edge_weights", "count"):
        assert re.search(rf"Tensor\(a\d+!\) {name}\b", sch), (name, sch)
    assert "float node_coverage, float min_dist, float spacing, int max_new" in sch
    assert sch.count("!") == 7 and sch.endswith("-> ()")


def _args(M, n_nodes, max_new, k_e=8, device="cpu"):
    f, i = torch.float32, torch.int32
    rows = n_nodes + max_new
    kw = dict(device=device)
    return [torch.zeros(1, dtype=i, **kw), 0, torch.empty((M, 3), dtype=f, **kw), torch.empty((M, 4), dtype=i, **kw),
            torch.empty((M, 4), dtype=f, **kw), torch.empty(M, dtype=torch.uint8, **kw),
            torch.empty((rows, 3), dtype=f, **kw), n_nodes, torch.empty((rows, 3, 3), dtype=f, **kw),
            torch.empty((rows, 3), dtype=f, **kw), torch.empty((rows, k_e), dtype=i, **kw),
            torch.empty((rows, k_e), dtype=f, **kw), 0.02, 0.04, 0.02, max_new, torch.empty(3, dtype=i, **kw)]


@pytest.mark.parametrize("M,n_nodes,max_new", [(1000, 14, 64), (1, 4, 1), (0, 4, 0)])
def test_fake_kernel(M, n_nodes, max_new):
    with FakeTensorMode():
        assert torch.ops.ofx.grow_nodes(*_args(M, n_nodes, max_new)) is None
    assert torch.ops.ofx.grow_nodes(*_args(M, n_nodes, max_new, device="meta")) is None


def test_grow_nodes_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.grow_nodes(*_args(10, 14, 8))


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd import grow
    from occlusionfusion_amd.warpfield import WarpField
    assert pkg.NodeGrower is grow.NodeGrower and (grow.MAX_POINTS, grow.MAX_NEW) == (65536, 4096)
    sig = inspect.signature(grow.NodeGrower.grow)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        min_dist=None, spacing=None, max_new=None, count=None)
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    sig = inspect.signature(FusionPipeline.track_step)
    assert sig.parameters["grow_every"].default == 0 and sig.parameters["grow"].default is None
    assert callable(Registration.grow_from_volume) and callable(FusionPipeline.grow_graph)
    sig = inspect.signature(WarpField.grow_from_volume)
    assert {k: v.default for k, v in list(sig.parameters.items())[1:]} == dict(
        max_new=256, min_dist=None, spacing=None, max_points=65536, w_min=1.0, incremental=False)
