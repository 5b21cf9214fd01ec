"""CPU: the weighted integrate and the observation-weight map exist at every layer — header, library exports, ctypes
structs, argument checks that answer with a status code before any launch, the torch.ops.ofx schemas and fake kernels,
and the Python keywords with their checks before any device work — without a device. ABI version stays 5."""
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
NEW = ("ofx_integrate_w", "ofx_integrate_palette_w", "ofx_integrate_palette_cull_w", "ofx_integrate_points_w",
       "ofx_observation_weights")
INF = float("inf")
vp = ctypes.c_void_p


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    declared = set(re.findall(r"^\s*int\s+(ofx_\w+)\s*\(", hdr, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in declared and n in _lib.EXPORTED and hasattr(lib, n), n
    # each twin takes its sibling's arguments plus the ofx_obs_weights pointer
    for n in NEW[:4]:
        assert len(_lib._SIGS[n]) == len(_lib._SIGS[n[:-2]]) + 1, n
    assert _lib.lib.ofx_abi_version() == 5   # entry points and new structs only: no existing struct changed
    assert re.search(r"#define\s+OFX_ABI_VERSION\s+5\b", hdr)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_struct_layouts_match_ctypes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(){printf("' + "%zu " * 8 + '\\n",'
                   "sizeof(ofx_obs_weights),offsetof(ofx_obs_weights,obs_im),offsetof(ofx_obs_weights,w_max),"
                   "sizeof(ofx_obs_params),offsetof(ofx_obs_params,cos_power),offsetof(ofx_obs_params,z_ref),"
                   "offsetof(ofx_obs_params,w_floor),offsetof(ofx_obs_params,edge_weight));}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    W, P = _lib.ObsWeights, _lib.ObsParams
    assert c == [ctypes.sizeof(W), W.obs_im.offset, W.w_max.offset, ctypes.sizeof(P), P.cos_power.offset, P.z_ref.offset,
                 P.w_floor.offset, P.edge_weight.offset] == [16, 0, 8, 16, 0, 4, 8, 12]


# ------------------------------------------------------------------------------------------------ status codes
def _obs(prm=(2, 1.0, 0.05, 0.0), p=64, n=64, out=64, H=32, W=40):
    """ofx_observation_weights with made-up, never dereferenced addresses: every case here is refused before a launch."""
    st = _lib.lib.ofx_observation_weights(vp(p), vp(n), H, W, ctypes.byref(_lib.ObsParams(*prm)), vp(out), None)
    return st, _lib.lib.ofx_last_error()


@pytest.mark.parametrize("prm,word", [((3, 1.0, 0.05, 0.0), b"cos_power"), ((-1, 1.0, 0.05, 0.0), b"cos_power"),
                                      ((2, -1.0, 0.05, 0.0), b"z_ref"), ((2, INF, 0.05, 0.0), b"z_ref"),
                                      ((2, float("nan"), 0.05, 0.0), b"z_ref"), ((2, 1.0, -0.05, 0.0), b"w_floor"),
                                      ((2, 1.0, INF, 0.0), b"w_floor"), ((2, 1.0, float("nan"), 0.0), b"w_floor"),
                                      ((2, 1.0, 0.05, -1.0), b"edge_weight"), ((2, 1.0, 0.05, INF), b"edge_weight"),
                                      ((2, 1.0, 0.05, float("nan")), b"edge_weight")])
def test_observation_weights_bad_parameters_are_status_codes(prm, word):
    st, msg = _obs(prm)
    assert st == -1 and word in msg, (st, msg)


def test_observation_weights_bad_buffers_and_sizes_are_status_codes():
    for kw in (dict(p=None), dict(n=None), dict(out=None)):
        st, msg = _obs(**kw)
        assert st == -1 and b"null buffer" in msg, (kw, st, msg)
    for kw in (dict(p=66), dict(n=65), dict(out=67)):
        st, msg = _obs(**kw)
        assert st == -1 and b"aligned" in msg, (kw, st, msg)
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 16, W=1 << 15)):
        st, msg = _obs(**kw)
        assert st == -1 and b"image size" in msg, (kw, st, msg)
    assert _lib.lib.ofx_observation_weights(vp(64), vp(64), 32, 40, None, vp(64), None) == -1
    assert b"null params" in _lib.lib.ofx_last_error()
    with pytest.raises(_lib.OfxError, match="cos_power"):
        _lib.call("ofx_observation_weights", vp(64), vp(64), 32, 40, ctypes.byref(_lib.ObsParams(7, 1.0, 0.05, 0.0)),
                  vp(64), None)


def _desc(sem=0):
    d = _lib.VolumeDesc()
    d.dim[:] = [16, 16, 16]
    d.brick_x0, d.brick_x1, d.semantics = 0, 2, sem
    d.origin[:] = [0.0, 0.0, 1.0]
    d.voxel_size, d.trunc_margin = 0.004, 0.04
    return d


def _twins(desc, ow):
    """The four _w entry points with made-up, never dereferenced addresses -> their status codes and messages."""
    L, cam, b = _lib.lib, _lib.Camera(525.0, 525.0, 20.0, 16.0, 40, 32), ctypes.byref
    a = vp(64)
    owp = None if ow is None else b(ow)
    out = []
    for name, args in (
            ("src", lambda: L.ofx_integrate_w(b(desc), b(cam), a, None, 0, None, 0, 1, None, 0, None, None, 1.0, a, a, None,
                                              None, owp, None)),
            ("warp", lambda: L.ofx_integrate_w(b(desc), b(cam), a, None, 1, a, 8, 4, a, 2, a, a, 1.0, a, a, None, None, owp,
                                               None)),
            ("pal", lambda: L.ofx_integrate_palette_w(b(desc), b(cam), a, None, a, 8, 4, a, 2, a, a, a, a, a, 1.0, a, a,
                                                      None, None, owp, None)),
            ("cull", lambda: L.ofx_integrate_palette_cull_w(b(desc), b(cam), a, None, a, 8, 4, a, 2, a, a, a, a, a, 1.0, a,
                                                            a, None, None, a, a, owp, None)),
            ("points", lambda: L.ofx_integrate_points_w(b(desc), b(cam), a, None, a, a, None, 10, 1.0, a, a, None, None,
                                                        owp, None))):
        out.append((name, args(), L.ofx_last_error()))
    return out


@pytest.mark.parametrize("ow,sem,word", [(None, 0, b"null observation weights"),
                                         ((None, INF), 0, b"null observation weights"),
                                         ((66, INF), 0, b"aligned"),
                                         ((64, 0.0), 0, b"w_max"), ((64, -2.0), 0, b"w_max"),
                                         ((64, float("nan")), 0, b"w_max"),
                                         ((64, INF), 1, b"CPU semantics"), ((64, 2.5), 1, b"CPU semantics")])
def test_weighted_integrate_bad_arguments_are_status_codes(ow, sem, word):
    w = None if ow is None else _lib.ObsWeights(ow[0], ow[1], 0.0)
    for name, st, msg in _twins(_desc(sem), w):
        assert st == -1 and word in msg, (name, st, msg)


# ------------------------------------------------------------------------------------------------ torch ops
def test_ops_registered_with_mutations():
    for n in ("integrate_weighted", "integrate_points_weighted", "observation_weights"):
        assert n in ops.OPS
    for n in ("integrate_weighted", "integrate_points_weighted"):
        sch = str(getattr(torch.ops.ofx, n).default._schema)
        assert "Tensor(a0!) tsdf, Tensor(a1!) weight, Tensor(a2!)? color, Tensor(a3!)? n_updated" in sch
        assert sch.endswith("Tensor obs_im, float w_max) -> ()"), sch
    sch = str(torch.ops.ofx.observation_weights.default._schema).replace("SymInt", "int")
    assert sch == ("ofx::observation_weights(Tensor point_image, Tensor normal_image, int cos_power, float z_ref, "
                   "float w_floor, float edge_weight) -> Tensor"), sch
    assert not any(a.alias_info is not None for a in torch.ops.ofx.observation_weights.default._schema.arguments)
    # the unweighted operators are as they were
    assert str(torch.ops.ofx.integrate.default._schema).endswith("Tensor? pal_n, Tensor? local) -> ()")


def test_fake_kernels_and_cpu_refusal():
    with FakeTensorMode():
        w = torch.ops.ofx.observation_weights(torch.empty(3, 17, 33), torch.empty(3, 17, 33), 2, 1.0, 0.05, 0.0)
        assert tuple(w.shape) == (17, 33) and w.dtype == torch.float32
        vol = torch.empty(512 * 8)
        geo = ([16, 16, 16], [0, 2], [0.0, 0.0, 1.0], 0.004, 0.04, 0, [525.0, 525.0, 319.5, 223.5], 1.0)
        assert torch.ops.ofx.integrate_weighted(vol, vol.clone(), None, None, torch.empty(448, 640), None, *geo, None, 0,
                                                1, None, 0, None, None, None, None, None, torch.empty(448, 640),
                                                INF) is None
        assert torch.ops.ofx.integrate_points_weighted(vol, vol.clone(), None, None, torch.empty(448, 640), None, *geo,
                                                       torch.empty(9, 3), torch.empty(9, dtype=torch.int64), None,
                                                       torch.empty(448, 640), 2.5) is None
    with pytest.raises(NotImplementedError):
        torch.ops.ofx.observation_weights(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5), 2, 1.0, 0.05, 0.0)


# ------------------------------------------------------------------------------------------------ Python layers
def test_python_keywords_exist_with_their_defaults():
    from occlusionfusion_amd import tsdf
    from occlusionfusion_amd.pipeline import FusionPipeline
    T = tsdf.TSDFVolume
    for fn in (T.integrate, T.integrate_device, T.integrate_points):
        p = inspect.signature(fn).parameters
        assert p["weight_image"].default is None and p["max_weight"].default is None and p["obs_weight"].default == 1.0
    p = inspect.signature(T.observation_weights).parameters
    assert {k: v.default for k, v in list(p.items())[3:]} == dict(cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0)
    assert tsdf.FUSION_WEIGHT_DEFAULTS == dict(cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0, max_weight=None,
                                               filter=True)
    assert inspect.signature(FusionPipeline.__init__).parameters["fusion_weights"].default is None
    p = inspect.signature(FusionPipeline.track_step).parameters
    assert p["fusion_weights"].default is None and p["w_min"].default is None
    assert inspect.signature(FusionPipeline.sample_model).parameters["w_min"].default is None
    assert inspect.signature(FusionPipeline.grow_graph).parameters["w_min"].default is None


def test_fusion_weight_params_and_w_min():
    from occlusionfusion_amd.image_proc import PREPARE_DEFAULTS
    from occlusionfusion_amd.tsdf import fusion_weight_params, resolve_w_min
    assert fusion_weight_params(None) is None and fusion_weight_params(False) is None
    d = fusion_weight_params(True)
    assert d == dict(cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0, max_weight=INF, filter=PREPARE_DEFAULTS)
    d = fusion_weight_params(dict(cos_power=1, max_weight=8, filter=dict(radius=2)))
    assert d["cos_power"] == 1 and d["max_weight"] == 8.0 and d["filter"] == dict(PREPARE_DEFAULTS, radius=2)
    assert fusion_weight_params(dict(filter=None))["filter"]["radius"] == 0
    with pytest.raises(TypeError, match="sigma_z"):
        fusion_weight_params(dict(sigma_z=1.0))
    with pytest.raises(TypeError, match="edge_max"):
        fusion_weight_params(dict(filter=dict(edge_max=0.03)))
    with pytest.raises(TypeError):
        fusion_weight_params(3)
    for bad in (dict(cos_power=3), dict(cos_power=1.5), dict(z_ref=-1.0), dict(z_ref=INF), dict(w_floor=float("nan")),
                dict(edge_weight=-0.1), dict(max_weight=0.0), dict(max_weight=-1), dict(max_weight=float("nan")),
                dict(filter=dict(radius=9)), dict(filter=dict(sigma_r=0.0))):
        with pytest.raises(ValueError):
            fusion_weight_params(bad)
    # w_min: today's 1.0 without fusion weights, w_floor with them, an explicit value respected, the cap not below it
    assert resolve_w_min(None, None) == 1.0 and resolve_w_min(2.0, None) == 2.0
    assert resolve_w_min(None, fusion_weight_params(True)) == 0.05
    assert resolve_w_min(0.5, fusion_weight_params(True)) == 0.5
    assert resolve_w_min(None, fusion_weight_params(dict(w_floor=0.2, max_weight=0.2))) == 0.2
    with pytest.raises(ValueError, match="max_weight"):
        resolve_w_min(1.0, fusion_weight_params(dict(max_weight=0.5)))
    with pytest.raises(ValueError, match="max_weight"):
        resolve_w_min(None, fusion_weight_params(dict(w_floor=0.3, max_weight=0.25)))


def test_pipeline_checks_run_before_any_device_work():
    """No device exists here: the constructor and track_step refuse bad fusion_weights before touching one."""
    from occlusionfusion_amd.pipeline import FusionPipeline
    with pytest.raises(TypeError, match="sigma_z"):
        FusionPipeline(None, None, None, None, fusion_weights=dict(sigma_z=1.0))
    with pytest.raises(ValueError, match="cos_power"):
        FusionPipeline(None, None, None, None, fusion_weights=dict(cos_power=5))
    pipe = FusionPipeline.__new__(FusionPipeline)      # (no constructor: nothing but the keyword checks can run)
    pipe.fusion_weights = None
    with pytest.raises(TypeError, match="cos_pow"):
        pipe.track_step(None, 1, fusion_weights=dict(cos_pow=2))
    with pytest.raises(ValueError, match="z_ref"):
        pipe.track_step(None, 1, fusion_weights=dict(z_ref=-1.0))
    with pytest.raises(ValueError, match="max_weight"):
        pipe.track_step(None, 1, fusion_weights=dict(max_weight=0.01))   # below w_floor, the resolved w_min
    with pytest.raises(ValueError, match="max_weight"):
        pipe.track_step(None, 1, w_min=1.0, fusion_weights=dict(max_weight=0.5))


def test_volume_checks_run_before_any_device_work():
    from occlusionfusion_amd.tsdf import TSDFVolume, max_weight_param, observation_weight_params
    assert max_weight_param(None) == INF and max_weight_param(4) == 4.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_weight"):
            max_weight_param(bad)
    with pytest.raises(ValueError, match="cos_power"):
        observation_weight_params(cos_power=True)
    vol = TSDFVolume.__new__(TSDFVolume)               # (no constructor, no device)
    vol.semantics = "pycuda"
    for kw in (dict(weight_image=torch.ones(2, 2)), dict(max_weight=4.0)):
        with pytest.raises(ValueError, match="semantics"):
            vol.integrate({"im": None, "id": 0}, **kw)
        with pytest.raises(ValueError, match="semantics"):
            vol.integrate_device(**kw)
        with pytest.raises(ValueError, match="semantics"):
            vol.integrate_points(None, None, **kw)
    vol.semantics = "cpu"
    with pytest.raises(ValueError, match="max_weight"):
        vol.integrate({"im": None, "id": 0}, max_weight=0.0)
    with pytest.raises(ValueError, match="cos_power"):
        vol.observation_weights(None, None, cos_power=4)
