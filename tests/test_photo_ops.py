"""CPU: the photometric search exists at every layer — header, library export, ctypes struct, argument checks, the
torch.ops.ofx.photo_associate schema and fake kernel, and the photo keyword of the tracking layers — without a device.
ABI version stays 5."""
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
INTR = [30.0, 30.0, 19.5, 15.5]
INF = float("inf")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "ofx_photo_associate" in declared and "ofx_photo_associate" in _lib.EXPORTED
    assert hasattr(lib, "ofx_photo_associate")
    assert re.search(r"#define\s+OFX_PHOTO_RMAX\s+8\b", hdr) and _lib.PHOTO_RMAX == 8
    assert _lib.lib.ofx_abi_version() == 5   # an entry point and a new struct only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_photo_params_layout_matches_ctypes(tmp_path):
    fields = ("dist_max", "cos_min", "color_max", "geo_weight", "radius", "max_matches")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("%zu' + " %zu" * 6 +
                   '\\n",sizeof(ofx_photo_params),' + ",".join(f"offsetof(ofx_photo_params,{f})" for f in fields) +
                   ");}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = _lib.PhotoParams
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] == [24, 0, 4, 8, 12, 16, 20]


def _call(handle, prm=None, cam=None, n=0, H=32, W=40, bufs=None, count=64):
    """ofx_photo_associate with made-up, never dereferenced buffer addresses: every case here is refused before any
    device work."""
    prm = prm if prm is not None else _lib.PhotoParams(0.05, 0.5, INF, 1.0, 4, 100)
    cam = cam if cam is not None else _lib.Camera(*INTR, 40, 32)
    vp = ctypes.c_void_p
    b = dict(points=64, normals=None, colors=64, anchors=64, weights=64, valid=None, packed=64, pimg=64, nimg=64,
             cimg=64, code=64, tgt=64, warped=None, pixel=None, cost=None, midx=64, src=64, tgt_o=64, a_o=64, w_o=64,
             px_o=None)
    b.update(bufs or {})
    a = {k: (vp(v) if v is not None else None) for k, v in b.items()}
    st = _lib.lib.ofx_photo_associate(handle, a["points"], a["normals"], a["colors"], a["anchors"], a["weights"],
                                      a["valid"], n, a["packed"], 6, ctypes.byref(cam), a["pimg"], a["nimg"], a["cimg"],
                                      H, W, ctypes.byref(prm), a["code"], a["tgt"], a["warped"], a["pixel"], a["cost"],
                                      a["midx"], a["src"], a["tgt_o"], a["a_o"], a["w_o"], a["px_o"],
                                      vp(count) if count else None, None)
    return st, _lib.lib.ofx_last_error()


def _stand_in(capacity):
    """A stand-in for an ofx_assoc handle, in host memory: the call reads only the handle's first field, its capacity
    (int64), before it refuses; nothing is launched on it. (A real handle needs a device.)"""
    buf = (ctypes.c_int64 * 4)(capacity, 0, 0, 0)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("prm,word", [((0.05, 0.5, INF, 1.0, 9, 100), b"radius"), ((0.05, 0.5, INF, 1.0, -1, 100), b"radius"),
                                      ((0.05, 0.5, INF, -1.0, 4, 100), b"geo_weight"),
                                      ((0.05, 0.5, INF, INF, 4, 100), b"geo_weight"),
                                      ((0.05, 0.5, INF, float("nan"), 4, 100), b"geo_weight"),
                                      ((0.05, 0.5, float("nan"), 1.0, 4, 100), b"color_max"),
                                      ((0.05, 0.5, INF, 1.0, 4, -1), b"max_matches")])
def test_bad_parameters_are_status_codes(prm, word):
    keep, h = _stand_in(0)
    st, msg = _call(h, _lib.PhotoParams(*prm))
    assert st == -1 and word in msg, (st, msg)


def test_null_size_and_capacity_refusals_are_status_codes():
    keep, h = _stand_in(5)
    st, msg = _call(None)
    assert st == -1 and b"null handle" in msg
    st, msg = _call(h, count=None)
    assert st == -1 and b"null handle" in msg
    st, msg = _call(h, n=6)
    assert st == -1 and b"n_points" in msg
    st, msg = _call(h, n=-1)
    assert st == -1 and b"n_points" in msg
    st, msg = _call(h, cam=_lib.Camera(*INTR, 41, 32))
    assert st == -1 and b"differ" in msg
    for k in ("points", "colors", "anchors", "weights", "packed", "pimg", "nimg", "cimg", "code", "tgt"):
        st, msg = _call(h, n=5, bufs={k: None})
        assert st == -1 and b"null buffer" in msg, (k, st, msg)
    for k in ("anchors", "weights", "packed", "a_o", "w_o"):
        st, msg = _call(h, n=5, bufs={k: 72})
        assert st == -1 and b"16-byte aligned" in msg, (k, st, msg)
    st, msg = _call(h, n=5, bufs={"midx": None})
    assert st == -1 and b"null compacted output" in msg
    st, msg = _call(h, n=5, bufs={"px_o": 64})
    assert st == -1 and b"pixel_out" in msg            # the compacted pixels are copied from the per-point ones
    with pytest.raises(_lib.OfxError, match="radius"):
        prm, cam = _lib.PhotoParams(0.05, 0.5, INF, 1.0, 12, 100), _lib.Camera(*INTR, 40, 32)
        _lib.call("ofx_photo_associate", h, *([None] * 6), 0, None, 6, ctypes.byref(cam), None, None, None, 32, 40,
                  ctypes.byref(prm), *([None] * 11), ctypes.c_void_p(64), None)


def test_photo_associate_registered_with_state_mutation():
    assert "photo_associate" in ops.OPS
    sch = str(torch.ops.ofx.photo_associate.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::photo_associate(Tensor(a0!) state, int handle, Tensor points, Tensor? normals, Tensor colors, "
                   "Tensor anchors, Tensor weights, Tensor? valid, Tensor packed_nodes, Tensor point_image, "
                   "Tensor normal_image, Tensor color_image, float[] intr, float dist_max, float cos_min, "
                   "float color_max, float geo_weight, int radius, int max_matches) -> (Tensor, Tensor, Tensor, Tensor, "
                   "Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)"), sch
    muts = [a.name for a in torch.ops.ofx.photo_associate.default._schema.arguments if a.alias_info is not None]
    assert muts == ["state"]


def _op_args(P, H=32, W=40, device="cpu", normals=True, valid=True):
    f = torch.float32
    e = lambda *s, dtype=f: torch.empty(s, dtype=dtype, device=device)  # noqa: E731
    return (e(1, dtype=torch.int32), 0, e(P, 3), e(P, 3) if normals else None, e(P, 3), e(P, 4, dtype=torch.int32),
            e(P, 4), e(P, dtype=torch.bool) if valid else None, e(6, 16), e(3, H, W), e(3, H, W), e(3, H, W), INTR, 0.05,
            0.5, INF, 1.0, 4, 77)


@pytest.mark.parametrize("P", [0, 1, 300])
def test_photo_associate_fake_kernel(P):
    f, i = torch.float32, torch.int32
    want = [((P,), torch.uint8), ((P, 3), f), ((P, 3), f), ((P, 2), i), ((P,), f), ((77,), i), ((77, 3), f), ((77, 3), f),
            ((77, 4), i), ((77, 4), f), ((77, 2), f), ((2,), i)]
    with FakeTensorMode():
        out = torch.ops.ofx.photo_associate(*_op_args(P))
        assert [(tuple(t.shape), t.dtype) for t in out] == want
        out = torch.ops.ofx.photo_associate(*_op_args(P, normals=False, valid=False))
        assert [(tuple(t.shape), t.dtype) for t in out] == want
    out = torch.ops.ofx.photo_associate(*_op_args(P, device="meta"))
    assert [(tuple(t.shape), t.dtype) for t in out] == want and all(t.device.type == "meta" for t in out)


def test_photo_associate_refuses_cpu_tensors():
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.photo_associate(*_op_args(8))


def test_python_layers_exist():
    from occlusionfusion_amd import association, synthetic
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    from occlusionfusion_amd.tsdf import TSDFVolume
    from occlusionfusion_amd.warpfield import WarpField
    sig = inspect.signature(association.ProjectiveAssociator.associate_photo)
    assert list(sig.parameters)[:12] == ["self", "points", "normals", "colors", "anchors", "weights", "valid",
                                         "warpfield_or_packed_nodes", "point_image", "normal_image", "color_image", "intr"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(dist_max=0.05, cos_min=0.5, color_max=INF, geo_weight=1.0, radius=4, max_matches=10000)
    assert association.PHOTO_DEFAULTS == dict(radius=4, color_max=INF, geo_weight=1.0)
    assert association.PHOTO_CODE_NAMES == association.CODE_NAMES + ("colour",) and len(association.CODE_NAMES) == 7
    for fn in (association.icp_track, Registration.track, FusionPipeline.track_step):
        p = inspect.signature(fn).parameters
        assert p["photo"].default is None and p["photo"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert p["assoc"].kind is inspect.Parameter.VAR_KEYWORD
        names = list(p)
        assert names.index("photo") < names.index("assoc")
    assert list(inspect.signature(association.icp_track).parameters)[:12] == [
        "associator", "solver", "graph_nodes", "graph_edges", "graph_edges_weights", "points", "normals", "anchors",
        "weights", "valid", "depth", "intr"]
    assert list(inspect.signature(WarpField.surface_colors).parameters) == ["self", "model"]
    assert inspect.signature(Registration.update).parameters["colors"].default is None
    assert callable(TSDFVolume.voxel_rgb)
    for name in ("surface_texture", "textured_frame"):
        assert callable(getattr(synthetic, name))
    assert callable(synthetic.SphereScene.undeform_points)


def test_unknown_photo_key_is_a_type_error_and_missing_colours_a_value_error_before_any_device_work():
    from occlusionfusion_amd.association import icp_track
    from occlusionfusion_amd.pipeline import FusionPipeline
    from occlusionfusion_amd.registration import Registration
    args = [None] * 12   # refused before anything is touched
    with pytest.raises(TypeError, match="sigma_c"):
        icp_track(*args, photo={"radius": 2, "sigma_c": 1.0})
    with pytest.raises(TypeError, match="edge_max"):
        icp_track(*args, photo={"edge_max": 0.03})          # the association's own gates stay **assoc's
    with pytest.raises(ValueError, match="colours"):
        icp_track(*args, photo=True)
    with pytest.raises(ValueError, match="colours"):
        icp_track(*args, photo={"radius": 2}, colors=np.zeros((1, 3), np.float32))   # no colour image
    reg = object.__new__(Registration)                      # no device object behind it: refused before any is needed
    reg.source_colors = None
    with pytest.raises(TypeError, match="sigma_c"):
        reg.track({"im": None}, photo={"sigma_c": 1.0})
    with pytest.raises(ValueError, match="colours"):
        reg.track({"im": None}, photo=True)
    pipe = object.__new__(FusionPipeline)
    with pytest.raises(TypeError, match="sigma_c"):
        pipe.track_step(None, 1, photo={"sigma_c": 1.0})
    with pytest.raises(ValueError, match="colours"):
        pipe.track_step(None, 1, photo=True)


def test_spin_scene_and_texture():
    from occlusionfusion_amd import synthetic as S
    cam = S.bench_camera(4)
    spin = S.SphereScene(motion="spin", occluder=False)
    assert np.array_equal(spin.render(cam, 0, None, 0.0), spin.render(cam, 7, None, 0.0))   # the depth never changes
    rng = np.random.default_rng(0)
    d = rng.normal(size=(200, 3))
    on = np.array(spin.center) + spin.radius * d / np.linalg.norm(d, axis=1, keepdims=True)
    plane = np.stack([rng.uniform(-0.5, 0.5, 50), rng.uniform(-0.4, 0.4, 50), np.full(50, spin.plane_z)], 1)
    pts = np.concatenate([on[on[:, 2] < spin.plane_z - 0.05], plane])
    moved = spin.deform_points(pts, 4)
    n_s = len(pts) - 50
    assert np.allclose(np.linalg.norm(moved[:n_s] - spin.center, axis=1), spin.radius)     # stays on the sphere
    ang = np.degrees(np.arccos(np.clip(((moved[:n_s] - spin.center) * (pts[:n_s] - spin.center)).sum(1)
                                       / spin.radius ** 2, -1, 1)))
    assert ang.max() <= 6.0 + 1e-9 and ang.max() > 5.0 and np.array_equal(moved[n_s:], pts[n_s:])
    for scene in (spin, S.SphereScene(motion="rigid", occluder=False), S.SphereScene(occluder=False)):
        assert np.allclose(scene.undeform_points(scene.deform_points(pts, 9), 9), pts, atol=1e-12)
    c = S.surface_texture(rng.uniform(-1, 2, (5000, 3)))
    assert c.shape == (5000, 3) and c.min() > 0.0 and c.max() < 1.0 and c.std(0).min() > 0.1
    im = S.textured_frame(spin, cam, 1, 2)
    assert im.shape == (6, cam.height, cam.width) and im.dtype == np.float32
    assert np.array_equal(im[5], S.frame_depth(spin, cam, 1, 2))
    assert np.allclose(im[:3] * 255, np.round(im[:3] * 255), atol=1e-4)                     # an 8-bit image
    hole = im[5] == 0
    assert hole.any() and np.all(im[:3][:, hole] == np.float32(128 / 255))                  # mid-grey without a surface
    # the texture is attached to the surface: a pixel's colour is the texture at its canonical point
    v, u = np.nonzero(~hole)
    z = spin.render(cam, 2, None, 0.0)[v, u].astype(np.float64)
    p = np.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], 1)
    want = S.surface_texture(spin.undeform_points(p, 2))
    assert np.abs(im[:3][:, v, u].T - want).mean() < 0.012                                  # 1 % noise + quantisation
