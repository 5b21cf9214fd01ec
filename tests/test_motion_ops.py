"""CPU: the motion completion entry points exist at every layer — header, library exports, ctypes struct, the
torch.ops.ofx.motion_forward / motion_complete schemas and fake kernels, the Python layers — without a device; the
weight blob round-trips and refuses a wrong shape. ABI version stays 5."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from occlusionfusion_amd import _lib, motion, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_ref import load_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ofx_motion_create", "ofx_motion_destroy", "ofx_motion_set_graph", "ofx_motion_forward", "ofx_motion_complete",
         "ofx_motion_reset", "ofx_motion_info")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    # the header's parameter lists and _lib.py's agree in length
    for n in NAMES:
        params = re.search(r"^\s*int\s+" + n + r"\s*\(([^;]*)\);", hdr, re.M | re.S).group(1)
        assert len(params.split(",")) == len(_lib._SIGS[n]), n
    assert _lib.lib.ofx_abi_version() == 5   # entry points and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_motion_graph_layout_matches_ctypes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(ofx_motion_graph),offsetof(ofx_motion_graph,n),offsetof(ofx_motion_graph,k),'
                   'offsetof(ofx_motion_graph,down),offsetof(ofx_motion_graph,up));}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    G = _lib.MotionGraph
    assert c == [ctypes.sizeof(G), G.n.offset, G.k.offset, G.down.offset, G.up.offset]
    assert c == [112, 32, 48, 64, 88]


def test_argument_errors_are_status_codes():
    """Checked before any device work: null pointers, a blob of the wrong length or with the wrong tag, bad capacities."""
    h = ctypes.c_void_p()
    blob = np.zeros(motion.blob_floats(), np.float32)
    p = blob.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.ofx_motion_create(p, blob.size, 10, 16, None) == -1
    assert _lib.lib.ofx_motion_create(None, blob.size, 10, 16, ctypes.byref(h)) == -1
    assert _lib.lib.ofx_motion_create(p, blob.size - 1, 10, 16, ctypes.byref(h)) == -1 and not h.value
    assert b"floats" in _lib.lib.ofx_last_error()
    assert _lib.lib.ofx_motion_create(p, blob.size, 10, 16, ctypes.byref(h)) == -1 and not h.value   # no tag
    assert b"tag" in _lib.lib.ofx_last_error()
    blob[:2] = np.array([motion.TAG, blob.size], np.uint32).view(np.float32)
    assert _lib.lib.ofx_motion_create(p, blob.size, 0, 16, ctypes.byref(h)) == -1
    assert _lib.lib.ofx_motion_create(p, blob.size, 10, 17, ctypes.byref(h)) == -1
    assert _lib.lib.ofx_motion_create(p, blob.size, 16385, 16, ctypes.byref(h)) == -3 and not h.value
    assert _lib.lib.ofx_motion_forward(*([None] * 4), 1, 1, None, None) == -1
    assert _lib.lib.ofx_motion_complete(*([None] * 4), 1, 2.0, *([None] * 8)) == -1
    assert _lib.lib.ofx_motion_set_graph(None, None, None) == -1 and _lib.lib.ofx_motion_reset(None) == -1
    assert _lib.lib.ofx_motion_info(None, None) == -1 and _lib.lib.ofx_motion_destroy(None) == 0


def test_pack_weights_round_trips_and_refuses_a_wrong_shape():
    sd = load_weights()
    blob = motion.pack_weights(sd)
    assert blob.dtype == np.float32 and blob.size == motion.blob_floats() == 294152 + 64 + 2
    head = blob[:2].view(np.uint32)
    assert int(head[0]) == motion.TAG and int(head[1]) == blob.size
    back = motion.unpack_weights(blob)
    assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    # tensors are accepted as well as arrays, and give the same blob
    assert np.array_equal(motion.pack_weights({k: torch.from_numpy(v) for k, v in sd.items()}), blob)
    bad = dict(sd)
    bad["layer51.conv.lin_key.weight"] = np.zeros((64, 32), np.float32)
    with pytest.raises(ValueError, match="layer51.conv.lin_key.weight"):
        motion.pack_weights(bad)
    missing = {k: v for k, v in sd.items() if k != "lin.bias"}
    with pytest.raises(KeyError):
        motion.pack_weights(missing)
    with pytest.raises(ValueError):
        motion.pack_weights(dict(sd, extra=np.zeros(3, np.float32)))
    with pytest.raises(ValueError):
        motion.unpack_weights(blob[:-1])


def test_load_state_dict_reads_npz_and_checkpoints(tmp_path):
    sd = load_weights()
    np.savez(tmp_path / "w.npz", **sd)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "w.tar")
    a, b = motion.load_state_dict(str(tmp_path / "w.npz")), motion.load_state_dict(str(tmp_path / "w.tar"))
    assert set(a) == set(b) == set(sd)
    assert np.array_equal(motion.pack_weights(a), motion.pack_weights(b))


def test_ops_registered_with_state_mutated():
    assert "motion_forward" in ops.OPS and "motion_complete" in ops.OPS
    sch = str(torch.ops.ofx.motion_forward.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::motion_forward(Tensor(a0!) state, int handle, Tensor pos, Tensor curr_motion, Tensor hist) "
                   "-> Tensor"), sch
    sch = str(torch.ops.ofx.motion_complete.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::motion_complete(Tensor(a0!) state, int handle, Tensor src, Tensor dst, Tensor visible, "
                   "float conf_scale, int max_hist) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)"), sch
    for op in (torch.ops.ofx.motion_forward, torch.ops.ofx.motion_complete):
        mutated = [a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write]
        assert mutated == ["state"]


def _fwd(N, T, device=None):
    kw = {} if device is None else {"device": device}
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(N, 3, **kw), torch.empty(N, 4, **kw),
            torch.empty(T, N, 4, **kw)]


def _cmp(N, device=None):
    kw = {} if device is None else {"device": device}
    return [torch.zeros(1, dtype=torch.int32, **kw), 0, torch.empty(N, 3, dtype=torch.float64, **kw),
            torch.empty(N, 3, dtype=torch.float64, **kw), torch.empty(N, dtype=torch.bool, **kw), 2.0, 16]


@pytest.mark.parametrize("N,T", [(254, 16), (1, 1)])
def test_fake_kernels(N, T):
    want = [((N, 3), torch.float64), ((N,), torch.float64), ((1,), torch.int32), ((N, 3), torch.float32),
            ((N, 4), torch.float32), ((16, N, 4), torch.float32), ((N, 4), torch.float32)]
    with FakeTensorMode():
        out = torch.ops.ofx.motion_forward(*_fwd(N, T))
        assert (tuple(out.shape), out.dtype) == ((N, 4), torch.float32)
        out = torch.ops.ofx.motion_complete(*_cmp(N))
        assert [(tuple(t.shape), t.dtype) for t in out] == want
    out = torch.ops.ofx.motion_complete(*_cmp(N, device="meta"))
    assert [(tuple(t.shape), t.dtype) for t in out] == want and all(t.device.type == "meta" for t in out)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.motion_forward(*_fwd(5, 2))
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.motion_complete(*_cmp(5))


def test_python_layers_exist():
    import occlusionfusion_amd as pkg
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    assert pkg.MotionCompleter is motion.MotionCompleter
    for name in ("from_checkpoint", "set_graph", "__call__", "reset", "forward"):
        assert callable(getattr(motion.MotionCompleter, name))
    assert list(inspect.signature(motion.MotionCompleter.__call__).parameters)[1:] == [
        "source_node_positions", "deformed_node_positions", "visible_mask"]
    for fn in (Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["motion_net"].default is None and p["motion_net"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
