"""CPU: the sub-pixel refinement exists at every layer — header, library export, ctypes struct, argument checks, the
torch.ops.ofx.photo_refine schema and fake kernel, and the photo_refine keyword of the tracking layers — without a
device. ABI version stays 5."""
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
INF = float("inf")
NAN = float("nan")
GOOD = (3, 8, 1e-3, 4.0, 1e-6, INF, 0.03, 0)     # half, iters, eps, max_shift, min_eig, ssd_max, edge_max, pad


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "ofx_photo_refine" in declared and "ofx_photo_refine" in _lib.EXPORTED
    assert hasattr(lib, "ofx_photo_refine")
    assert re.search(r"#define\s+OFX_REFINE_HMAX\s+4\b", hdr) and _lib.REFINE_HMAX == 4
    assert _lib.lib.ofx_abi_version() == 5   # an entry point and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)
    assert os.path.exists(os.path.join(ROOT, "occlusionfusion_amd", "csrc", "refine.hip"))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_refine_params_layout_matches_ctypes(tmp_path):
    fields = ("half", "iters", "eps", "max_shift", "min_eig", "ssd_max", "edge_max")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu' + " %zu" * 7 +
                   '\\n",sizeof(ofx_refine_params),' + ",".join(f"offsetof(ofx_refine_params,{f})" for f in fields) +
                   ");}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = _lib.RefineParams
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] == [32, 0, 4, 8, 12, 16, 20, 24]


def _call(prm=GOOD, R=10, H=32, W=40, bufs=None, null_prm=False):
    """ofx_photo_refine with made-up, never dereferenced buffer addresses: every case here is refused before any device
    work."""
    vp = ctypes.c_void_p
    b = dict(timg=64, mask=None, cimg=64, pimg=64, tpx=64, ipx=64, tgt=64, count=64, px_o=64, tgt_o=64, status=64,
             ssd=64)
    b.update(bufs or {})
    a = {k: (vp(v) if v is not None else None) for k, v in b.items()}
    p = _lib.RefineParams(*prm)
    st = _lib.lib.ofx_photo_refine(a["timg"], a["mask"], a["cimg"], a["pimg"], a["tpx"], a["ipx"], a["tgt"], a["count"],
                                   R, H, W, None if null_prm else ctypes.byref(p), a["px_o"], a["tgt_o"], a["status"],
                                   a["ssd"], None)
    return st, _lib.lib.ofx_last_error()


def _with(**kw):
    names = ("half", "iters", "eps", "max_shift", "min_eig", "ssd_max", "edge_max", "pad")
    d = dict(zip(names, GOOD))
    d.update(kw)
    return tuple(d[k] for k in names)


@pytest.mark.parametrize("prm,word", [
    (_with(half=0), b"half"), (_with(half=5), b"half"), (_with(half=-1), b"half"),
    (_with(iters=0), b"iters"), (_with(iters=-2), b"iters"),
    (_with(eps=-1e-3), b"eps"), (_with(eps=INF), b"eps"), (_with(eps=NAN), b"eps"),
    (_with(max_shift=-1.0), b"max_shift"), (_with(max_shift=INF), b"max_shift"), (_with(max_shift=NAN), b"max_shift"),
    (_with(min_eig=-1e-6), b"min_eig"), (_with(min_eig=INF), b"min_eig"), (_with(min_eig=NAN), b"min_eig"),
    (_with(edge_max=-0.01), b"edge_max"), (_with(edge_max=INF), b"edge_max"), (_with(edge_max=NAN), b"edge_max"),
    (_with(ssd_max=NAN), b"ssd_max")])
def test_bad_parameters_are_status_codes(prm, word):
    st, msg = _call(prm)
    assert st == -1 and word in msg, (st, msg)


def test_null_size_and_alignment_refusals_are_status_codes():
    st, msg = _call(null_prm=True)
    assert st == -1 and b"null params" in msg
    st, msg = _call(bufs={"count": None})
    assert st == -1 and b"null params" in msg
    for H, W in ((0, 40), (32, 0), (-1, 40)):
        st, msg = _call(H=H, W=W)
        assert st == -1 and b"image size" in msg
    st, msg = _call(R=-1)
    assert st == -1 and b"max_rows" in msg
    for k in ("timg", "cimg", "pimg", "tpx", "ipx", "tgt", "px_o", "tgt_o", "status", "ssd"):
        st, msg = _call(bufs={k: None})
        assert st == -1 and b"null buffer" in msg, (k, st, msg)
    for k in ("timg", "cimg", "pimg", "tpx", "ipx", "tgt", "px_o", "tgt_o", "ssd", "count"):
        st, msg = _call(bufs={k: 66})
        assert st == -1 and b"4-byte aligned" in msg, (k, st, msg)
    # the parameters are checked before the buffers
    st, msg = _call(_with(half=9), bufs={"timg": None})
    assert st == -1 and b"half" in msg
    with pytest.raises(_lib.OfxError, match="iters"):
        p = _lib.RefineParams(*_with(iters=0))
        _lib.call("ofx_photo_refine", *([None] * 7), ctypes.c_void_p(64), 10, 32, 40, ctypes.byref(p), *([None] * 5))


def test_photo_refine_registered_with_its_mutations():
    assert "photo_refine" in ops.OPS
    sch = str(torch.ops.ofx.photo_refine.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::photo_refine(Tensor template_image, Tensor? template_mask, Tensor color_image, "
                   "Tensor point_image, Tensor template_px, Tensor init_px, Tensor tgt_in, Tensor count, int half, "
                   "int iters, float eps, float max_shift, float min_eig, float ssd_max, float edge_max, "
                   "Tensor(a15!) px_out, Tensor(a16!) tgt_out, Tensor(a17!) status, Tensor(a18!) ssd) -> ()"), sch
    muts = [a.name for a in torch.ops.ofx.photo_refine.default._schema.arguments if a.alias_info is not None]
    assert muts == ["px_out", "tgt_out", "status", "ssd"]


def _op_args(R, H=32, W=40, device="cpu", mask=True):
    f = torch.float32
    e = lambda *s, dtype=f: torch.empty(s, dtype=dtype, device=device)  # noqa: E731
    return (e(3, H, W), e(H, W, dtype=torch.uint8) if mask else None, e(3, H, W), e(3, H, W), e(R, 2), e(R, 2), e(R, 3),
            e(2, dtype=torch.int32), 3, 8, 1e-3, 4.0, 1e-6, INF, 0.03, e(R, 2), e(R, 3), e(R, dtype=torch.uint8), e(R))


@pytest.mark.parametrize("R", [0, 1, 300])
def test_photo_refine_fake_kernel(R):
    with FakeTensorMode():
        assert torch.ops.ofx.photo_refine(*_op_args(R)) is None
        assert torch.ops.ofx.photo_refine(*_op_args(R, mask=False)) is None
    assert torch.ops.ofx.photo_refine(*_op_args(R, device="meta")) is None


def test_photo_refine_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.photo_refine(*_op_args(8))


def test_python_layers_exist():
    from occlusionfusion_amd import association
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    assert association.REFINE_DEFAULTS == dict(half=3, iters=8, eps=1e-3, max_shift=4.0, min_eig=1e-6, ssd_max=INF)
    assert association.PHOTO_DEFAULTS == dict(radius=4, color_max=INF, geo_weight=1.0)      # untouched
    assert len(association.REFINE_CODE_NAMES) == 8
    rp = association.refine_params
    assert rp(None) is None and rp(False) is None and rp(True) == association.REFINE_DEFAULTS
    assert rp(True) is not association.REFINE_DEFAULTS
    assert rp({"half": 2, "ssd_max": 0.1}) == dict(association.REFINE_DEFAULTS, half=2, ssd_max=0.1)
    with pytest.raises(TypeError, match="radius"):
        rp({"radius": 2})
    sig = inspect.signature(association.ProjectiveAssociator.refine_photo)
    assert list(sig.parameters) == ["self", "match", "template_image", "template_px", "color_image", "point_image",
                                    "edge_max", "template_mask", "refine"]
    assert sig.parameters["template_mask"].default is None
    assert sig.parameters["refine"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(association.icp_track).parameters
    assert p["photo_refine"].default is None and p["template"].default is None
    for fn in (Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["photo_refine"].default is None and p["photo_refine"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert list(p).index("photo_refine") < list(p).index("assoc")
    assert inspect.signature(Registration.update).parameters["template"].default is None
    assert callable(FusionPipeline._canonical_template)


def test_refusals_before_any_device_work():
    from occlusionfusion_amd.association import icp_track
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    args = [None] * 12   # refused before anything is touched
    col = dict(colors=np.zeros((1, 3), np.float32), color_image=np.zeros((3, 4, 4), np.float32))
    with pytest.raises(TypeError, match="radius"):
        icp_track(*args, photo=True, photo_refine={"half": 2, "radius": 1}, **col)
    with pytest.raises(ValueError, match="needs photo"):
        icp_track(*args, photo_refine=True, template=(None, None, None))          # no photo
    with pytest.raises(ValueError, match="template"):
        icp_track(*args, photo=True, photo_refine=True, **col)                    # no template
    reg = object.__new__(Registration)                      # no device object behind it: refused before any is needed
    reg.source_colors = np.zeros((1, 3), np.float32)
    reg.source_template = None
    with pytest.raises(TypeError, match="radius"):
        reg.track({"im": None}, photo=True, photo_refine={"radius": 1})
    with pytest.raises(ValueError, match="needs photo"):
        reg.track({"im": None}, photo_refine=True)
    with pytest.raises(ValueError, match="template"):
        reg.track({"im": None}, photo=True, photo_refine={"half": 2})
    pipe = object.__new__(FusionPipeline)
    with pytest.raises(TypeError, match="radius"):
        pipe.track_step(None, 1, photo=True, photo_refine={"radius": 1})
    with pytest.raises(ValueError, match="needs photo"):
        pipe.track_step(None, 1, photo_refine=True)
    with pytest.raises(ValueError, match="template of the rendered model is not built"):
        pipe.track_step(None, 1, model="volume", photo=True, photo_refine=True)
    with pytest.raises(ValueError, match="template of the rendered model is not built"):
        pipe.track_step(None, 1, model="volume", photo_refine={"half": 2})
