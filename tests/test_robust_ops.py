"""CPU: the per-match weights and robust data rows exist at every layer — header, library export, ctypes struct, the
setting's argument checks, the torch.ops.ofx.gn_set_robust schema and fake kernel, the match_weights / robust keywords of
GaussNewtonSolver.optimize and the robust keyword of the tracking layers — without a device. ABI version stays 5."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "ofx_gn_set_robust" in declared and "ofx_gn_set_robust" in _lib.EXPORTED
    assert hasattr(lib, "ofx_gn_set_robust")
    assert re.search(r"OFX_ROBUST_NONE = 0, OFX_ROBUST_HUBER = 1, OFX_ROBUST_TUKEY = 2", hdr)
    assert _lib.ROBUST_KERNELS == {"none": 0, "huber": 1, "tukey": 2}
    assert _lib.lib.ofx_abi_version() == 5   # an entry point and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_gn_robust_layout_matches_ctypes(tmp_path):
    fields = ("match_weights", "kernel", "_pad", "scale")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu' + " %zu" * 4 +
                   '\\n",sizeof(ofx_gn_robust),' + ",".join(f"offsetof(ofx_gn_robust,{f})" for f in fields) + ");}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = _lib.GnRobust
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] == [24, 0, 8, 12, 16]


@pytest.mark.parametrize("kernel,scale,word", [(3, 0.03, b"unknown robust kernel 3"), (-1, 0.03, b"unknown robust kernel"),
                                               (1, 0.0, b"scale"), (2, -0.03, b"scale"), (2, float("nan"), b"scale"),
                                               (1, float("inf"), b"scale")])
def test_bad_settings_are_status_codes(kernel, scale, word):
    """The setting is checked before the handle is touched: refused with a text even on a null handle."""
    rb = _lib.GnRobust(None, kernel, 0, scale)
    st = _lib.lib.ofx_gn_set_robust(None, ctypes.byref(rb))
    msg = _lib.lib.ofx_last_error()
    assert st == -1 and word in msg, (st, msg)
    with pytest.raises(_lib.OfxError, match=word.decode()):
        _lib.call("ofx_gn_set_robust", None, ctypes.byref(rb))


def test_good_settings_reach_the_handle_check():
    for rb in (None, _lib.GnRobust(None, 0, 0, 0.0), _lib.GnRobust(None, 0, 0, float("nan")),   # (no kernel: scale unread)
               _lib.GnRobust(ctypes.c_void_p(64), 2, 0, 0.03), _lib.GnRobust(None, 1, 0, 0.005)):
        st = _lib.lib.ofx_gn_set_robust(None, ctypes.byref(rb) if rb is not None else None)
        assert st == -1 and b"null handle" in _lib.lib.ofx_last_error()


def test_gn_set_robust_registered_with_state_mutation():
    assert "gn_set_robust" in ops.OPS
    sch = str(torch.ops.ofx.gn_set_robust.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::gn_set_robust(Tensor(a0!) state, int handle, Tensor? match_weights, int kernel, float scale) "
                   "-> ()"), sch
    muts = [a.name for a in torch.ops.ofx.gn_set_robust.default._schema.arguments if a.alias_info is not None]
    assert muts == ["state"]


def test_gn_set_robust_fake_kernel_and_cpu_refusal():
    with FakeTensorMode():
        st = torch.zeros(1, dtype=torch.int32)
        assert torch.ops.ofx.gn_set_robust(st, 0, torch.empty(600), 2, 0.03) is None
        assert torch.ops.ofx.gn_set_robust(st, 0, None, 0, 0.0) is None
    assert torch.ops.ofx.gn_set_robust(torch.zeros(1, dtype=torch.int32, device="meta"), 0, None, 1, 0.005) is None
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.gn_set_robust(torch.zeros(1, dtype=torch.int32), 0, torch.ones(8), 2, 0.03)


def test_robust_defaults_and_keyword_validation():
    import robust_ref as RR
    from occlusionfusion_amd.registration import ROBUST_DEFAULTS, robust_params
    assert ROBUST_DEFAULTS == {"huber": 0.005, "tukey": 0.03} == RR.DEFAULTS
    assert robust_params(None) is None and robust_params(False) is None and robust_params({"kernel": "none"}) is None
    assert robust_params("huber") == (1, 0.005) and robust_params("tukey") == (2, 0.03)
    assert robust_params({"kernel": "tukey"}) == (2, 0.03)
    assert robust_params({"kernel": "huber", "scale": 0.01}) == (1, 0.01)
    with pytest.raises(TypeError, match="delta"):
        robust_params({"kernel": "huber", "delta": 0.01})
    with pytest.raises(ValueError, match="cauchy"):
        robust_params("cauchy")
    with pytest.raises(ValueError, match="cauchy"):
        robust_params({"kernel": "cauchy", "scale": 0.01})
    with pytest.raises(ValueError, match="kernel"):
        robust_params({"scale": 0.01})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            robust_params({"kernel": "tukey", "scale": bad})


def test_python_layers_have_the_keywords():
    from occlusionfusion_amd import association
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import GaussNewtonSolver, Registration
    p = inspect.signature(GaussNewtonSolver.optimize).parameters
    assert p["match_weights"].default is None and p["robust"].default is None
    assert list(p)[:11] == ["self", "graph_nodes", "graph_edges", "graph_edges_weights", "target_node_position",
                            "node_confidence", "source_points", "anchors", "weights", "target_points", "intrinsics"]
    assert list(p).index("prefetch") < list(p).index("match_weights")        # appended: positional callers are unmoved
    for fn in (association.icp_track, Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["robust"].default is None and p["robust"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert p["assoc"].kind is inspect.Parameter.VAR_KEYWORD
        assert list(p).index("photo") < list(p).index("robust") < list(p).index("assoc")


def test_bad_robust_keyword_is_refused_before_any_device_work():
    from occlusionfusion_amd.association import icp_track
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import GaussNewtonSolver, Registration
    args = [None] * 12   # refused before anything is touched
    with pytest.raises(TypeError, match="delta"):
        icp_track(*args, robust={"kernel": "huber", "delta": 1.0})
    with pytest.raises(ValueError, match="cauchy"):
        icp_track(*args, robust="cauchy")
    reg = object.__new__(Registration)                      # no device object behind it: refused before any is needed
    with pytest.raises(ValueError, match="cauchy"):
        reg.track({"im": None}, robust="cauchy")
    pipe = object.__new__(FusionPipeline)
    with pytest.raises(TypeError, match="delta"):
        pipe.track_step(None, 1, robust={"delta": 1.0})
    s = object.__new__(GaussNewtonSolver)
    with pytest.raises(ValueError, match="cauchy"):
        s.optimize(*([None] * 10), robust="cauchy")
    with pytest.raises(TypeError, match="delta"):
        s.optimize(*([None] * 10), robust={"kernel": "tukey", "delta": 0.03})


def test_registration_optimize_forwards_correspondence_weights():
    """Registration.optimize hands the target frame's correspondence_weights entry, restricted to the valid and selected
    vertices, to the solver as match_weights; without the entry the call is as it was (match_weights None)."""
    from occlusionfusion_amd.registration import Registration

    class Graph:
        nodes, edges, edges_weights = np.zeros((4, 3), np.float32), np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)

    class Stop(Exception):
        pass

    seen = {}

    class Solver:
        def optimize(self, *a, **kw):
            seen.update(kw, n=a[5].shape[0])
            raise Stop

    reg = object.__new__(Registration)
    reg.graph, reg.solver, reg.device, reg.max_matches = Graph, Solver(), torch.device("cpu"), 100
    reg.intrinsics = np.array([100.0, 100.0, 8.0, 8.0])
    reg.prev_rot = reg.prev_trans = None
    reg.valid_source_verts = np.array([True, False, True, True, True, True])
    reg.source_pcd = torch.zeros(5, 3)
    reg.point_anchors = torch.zeros(5, 4, dtype=torch.int32)
    reg.anchor_weight = torch.zeros(5, 4)
    sf = {"target_matches": np.zeros((6, 3), np.float32), "valid_verts": np.array([True, True, False, True, True])}
    cw = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], np.float32)
    with pytest.raises(Stop):
        reg.optimize({"source_id": 0, "target_id": 1}, sf, None, {"correspondence_weights": cw})
    assert seen["n"] == 4 and np.array_equal(seen["match_weights"], np.array([0.1, 0.3, 0.5, 0.6], np.float32))
    seen.clear()
    with pytest.raises(Stop):
        reg.optimize({"source_id": 0, "target_id": 1}, sf, None, {})
    assert seen["match_weights"] is None
