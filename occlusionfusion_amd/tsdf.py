"""TSDFVolume — drop-in for fusion_with_occlusion/tsdf.py:TSDFVolume, backed by libofx (HIP, gfx950).

Same constructor (bbox, max_depth, cam_intr, fopt, visualizer), same `integrate(image_data,
obs_weight=1.)`, `update(im, frame_id)`, `get_volume() -> (tsdf, color, weight)`,
`check_visibility(points) -> (valid, depth_diff)`, `get_visible_nodes()`, `save_volume/load_volume`,
`clear()`. Volume state stays device-resident (8³ bricks); get_volume() copies D2H only on request.
Both of the reference's integrate arithmetics are available (`semantics`, include/ofx.h OFX_SEM_*):
"cpu" (default; the numba/numpy branch, tsdf.py:442-494: f64 projection, round-half-even pixels, no
ray factor) and "pycuda" (the GPU-mode kernel, tsdf.py:192-288: f32, roundf(.+0.5) pixels, ray-factor
scaled depth difference). The reference picks pycuda iff `fopt.gpu` and pycuda imports (tsdf.py:143);
here the choice is explicit: constructor argument, else `fopt.integrate_semantics`, else "cpu".
"""
import logging
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.ofx.*)
from ._lib import call, ptr, stream_ptr, byref
from .sharding import shard_bricks  # noqa: F401  (re-exported: reference-style import path)

log = logging.getLogger(__name__)
TRUNC_MARGIN = 0.04  # tsdf.py:127
SEMANTICS = {"cpu": 0, "pycuda": 1}   # OFX_SEM_CPU / OFX_SEM_PYCUDA


# fusion_weights=True: the per-pixel observation weights of the weighted integrate. Conventions of volumetric fusion
# (an angle term cos^2, a range term against 1 m, a small floor, depth-edge pixels left out), not measurements.
FUSION_WEIGHT_DEFAULTS = dict(cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0, max_weight=None, filter=True)
FUSION_EDGE_MAX = 0.03   # the normal map's depth-edge bound (prepare_depth_device's default, the association's)


def _finite_nonneg(name, v):
    v = float(v)
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
    return v


def observation_weight_params(cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0):
    """The checked parameters of TSDFVolume.observation_weights (a ValueError for a bad value, no device work)."""
    if isinstance(cos_power, bool) or cos_power not in (0, 1, 2):
        raise ValueError(f"cos_power must be 0, 1 or 2, got {cos_power!r}")
    return dict(cos_power=int(cos_power), z_ref=_finite_nonneg("z_ref", z_ref), w_floor=_finite_nonneg("w_floor", w_floor),
                edge_weight=_finite_nonneg("edge_weight", edge_weight))


def max_weight_param(max_weight):
    """max_weight=None -> +inf (no cap); else a float > 0 (a ValueError otherwise)."""
    if max_weight is None:
        return float("inf")
    m = float(max_weight)
    if not m > 0.0:
        raise ValueError(f"max_weight must be > 0 (None: no cap), got {max_weight!r}")
    return m


def fusion_weight_params(fusion_weights):
    """fusion_weights=None | False -> None; True -> FUSION_WEIGHT_DEFAULTS; a dict -> the defaults with its entries. An
    unknown key is a TypeError and a bad value a ValueError, both before any device work. `filter` takes what
    depth_filter takes (None / False: the raw frame's normals; True; a dict of radius, sigma_s, sigma_r, range_cut) and
    comes back as prepare_depth_device's keywords."""
    from .image_proc import PREPARE_DEFAULTS
    if fusion_weights is None or fusion_weights is False:
        return None
    prm = dict(FUSION_WEIGHT_DEFAULTS)
    if fusion_weights is not True:
        if not isinstance(fusion_weights, dict):
            raise TypeError(f"fusion_weights must be None, True or a dict, got {type(fusion_weights).__name__}")
        unknown = set(fusion_weights) - set(prm)
        if unknown:
            raise TypeError(f"unknown fusion_weights parameters {sorted(unknown)}")
        prm.update(fusion_weights)
    out = observation_weight_params(prm["cos_power"], prm["z_ref"], prm["w_floor"], prm["edge_weight"])
    out["max_weight"] = max_weight_param(prm["max_weight"])
    f = prm["filter"]
    if f is None or f is False:
        filt = dict(PREPARE_DEFAULTS, radius=0)
    else:
        filt = dict(PREPARE_DEFAULTS)
        if f is not True:
            if not isinstance(f, dict):
                raise TypeError(f"fusion_weights filter must be None, True or a dict, got {type(f).__name__}")
            unknown = set(f) - set(filt)
            if unknown:
                raise TypeError(f"unknown fusion_weights filter parameters {sorted(unknown)}")
            filt.update(f)
        if not (isinstance(filt["radius"], (int, np.integer)) and 0 <= filt["radius"] <= _lib.PREPARE_RMAX):
            raise ValueError(f"fusion_weights filter radius must be an integer in [0, {_lib.PREPARE_RMAX}]")
        if not (float(filt["sigma_s"]) > 0 and float(filt["sigma_r"]) > 0):
            raise ValueError("fusion_weights filter sigma_s and sigma_r must be positive")
        if filt["range_cut"] is not None and not float(filt["range_cut"]) > 0:
            raise ValueError("fusion_weights filter range_cut must be positive")
    out["filter"] = filt
    return out


def resolve_w_min(w_min, fusion):
    """The model sampling's w_min (accumulated weight): None -> 1.0 without fusion weights (one whole observation), the
    weights' w_floor with them (seen at least once by a pixel that has a normal; 1.0 would empty the model after the
    source frame). An explicit value stands. The weight cap must not lie below it (ValueError)."""
    if w_min is None:
        w_min = 1.0 if fusion is None else fusion["w_floor"]
    w_min = float(w_min)
    if fusion is not None and fusion["max_weight"] < w_min:
        raise ValueError(f"fusion_weights max_weight ({fusion['max_weight']}) is below the model's w_min ({w_min}): no "
                         "voxel could ever be sampled")
    return w_min


def _opt(fopt, name, default=None):
    if fopt is None:
        return default
    if isinstance(fopt, dict):
        return fopt.get(name, default)
    return getattr(fopt, name, default)


def volume_geometry(bbox, max_depth, cam_intr, voxel_dim=None, voxel_size=None):
    """tsdf.py:55-129: frustum bounds of the bbox at max_depth -> (vol_bnds, vol_dim, voxel_size, origin f32)."""
    fx, fy, cx, cy = (float(v) for v in cam_intr[:4])
    w_min, h_min, w_max, h_max = bbox
    md = np.array([0, max_depth, max_depth, max_depth, max_depth])
    pts = np.array([(np.array([0, w_min, w_min, w_max, w_max]) - cx) * md / fx,
                    (np.array([0, h_min, h_max, h_min, h_max]) - cy) * md / fy, md])
    vol_bnds = np.asarray([np.min(pts, axis=1), np.max(pts, axis=1)]).T
    if voxel_dim is not None:
        vol_dim = np.array([voxel_dim] * 3) if isinstance(voxel_dim, (int, np.integer)) else np.asarray(voxel_dim)
        assert vol_dim.shape[0] == 3, f"Voxel dimension should have length = 3 found {voxel_dim}"
        vs = float(((vol_bnds[:, 1] - vol_bnds[:, 0]) / vol_dim).max())
    elif voxel_size is not None:
        vs = float(voxel_size)
        vol_dim = np.ceil((vol_bnds[:, 1] - vol_bnds[:, 0]) / vs).astype(int)
    else:
        raise ValueError("fopt needs voxel_dim or voxel_size")
    vol_bnds[:, 1] = vol_bnds[:, 0] + vol_dim * vs
    return vol_bnds, vol_dim.astype(np.int64), vs, vol_bnds[:, 0].astype(np.float32)


class TSDFVolume:
    """Volumetric TSDF fusion of RGB-D images (tsdf.py:37-876), MI355X-resident."""

    def __init__(self, bbox, max_depth, cam_intr, fopt, visualizer=None, device=None, shard=None, semantics=None):
        vd = _opt(fopt, "voxel_dim")
        vs = _opt(fopt, "voxel_size")
        vol_bnds, vol_dim, voxel_size, origin = volume_geometry(bbox, max_depth, cam_intr, vd, vs)
        self._init(vol_bnds, vol_dim, voxel_size, origin, cam_intr, fopt, visualizer, device, shard, semantics)

    @classmethod
    def from_grid(cls, origin, voxel_size, vol_dim, cam_intr, fopt=None, visualizer=None, device=None, shard=None,
                  semantics=None):
        """Direct grid construction (benchmark configs): origin (3,), voxel size (m), dims (3,)."""
        self = cls.__new__(cls)
        origin = np.asarray(origin, np.float32)
        vol_dim = np.asarray(vol_dim, np.int64).reshape(3)
        vol_bnds = np.stack([origin.astype(np.float64), origin.astype(np.float64) + vol_dim * float(voxel_size)], 1)
        self._init(vol_bnds, vol_dim, float(voxel_size), origin, cam_intr, fopt, visualizer, device, shard, semantics)
        return self

    def _init(self, vol_bnds, vol_dim, voxel_size, origin, cam_intr, fopt, visualizer, device, shard, semantics=None):
        self.fopt = fopt if fopt is not None else SimpleNamespace(source_frame=0, skip_rate=1)
        self.vis = visualizer
        self.cam_intr = np.eye(3)
        self.cam_intr[0, 0], self.cam_intr[1, 1], self.cam_intr[0, 2], self.cam_intr[1, 2] = (float(v) for v in cam_intr[:4])
        self._vol_bnds = vol_bnds
        self._vol_dim = np.asarray(vol_dim, np.int64)
        self._voxel_size = voxel_size
        self._vol_origin = np.asarray(origin, np.float32)
        self._trunc_margin = TRUNC_MARGIN
        self._color_const = 256 * 256
        self.gpu_mode = True
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        nbx = int((self._vol_dim[0] + 7) // 8)
        rank, world, kind = (tuple(shard) + ("slab",))[:3] if shard is not None else (0, 1, "slab")
        if kind not in ("slab", "hash"):
            raise ValueError(f"shard kind must be 'slab' or 'hash', got {kind!r}")
        self.shard = (rank, world)
        self.shard_kind = kind
        self.owned_bricks = None    # hash shards: int32 device list of this rank's bricks
        self.owned_mask = None      # hash shards: bool device mask over all bricks
        if kind == "hash":          # whole brick address space, own bricks by spatial hash (sharding.hash_owner)
            from .sharding import hash_owner
            self.brick_x0, self.brick_x1 = 0, nbx
            self.brick_owner = hash_owner(nbx, int((self._vol_dim[1] + 7) // 8), int((self._vol_dim[2] + 7) // 8),
                                          world)
        else:
            self.brick_x0, self.brick_x1 = shard_bricks(nbx, rank, world)
        self.desc = _lib.VolumeDesc()
        self.desc.dim[:] = [int(d) for d in self._vol_dim]
        self.desc.brick_x0, self.desc.brick_x1 = self.brick_x0, self.brick_x1
        self.desc.origin[:] = [float(o) for o in self._vol_origin]
        self.desc.voxel_size = float(self._voxel_size)
        self.desc.trunc_margin = float(self._trunc_margin)
        sem = semantics if semantics is not None else _opt(self.fopt, "integrate_semantics", "cpu")
        if sem not in SEMANTICS:
            raise ValueError(f"integrate semantics must be one of {sorted(SEMANTICS)}, got {sem!r}")
        self.semantics = sem
        self.desc.semantics = SEMANTICS[sem]
        n = _lib.c_int64()
        call("ofx_volume_num_slots", byref(self.desc), byref(n))
        self.n_slots = int(n.value)
        self.n_bricks = self.n_slots // 512
        self.x_lo = self.brick_x0 * 8
        self.x_hi = min(self.brick_x1 * 8, int(self._vol_dim[0]))
        kw = dict(dtype=torch.float32, device=self.device)
        self.tsdf_b = torch.empty(self.n_slots, **kw)
        self.weight_b = torch.empty(self.n_slots, **kw)
        self.color_b = torch.empty(self.n_slots, **kw)
        self.n_updated = torch.zeros(max(1, self.n_bricks), dtype=torch.int32, device=self.device)  # per brick
        if kind == "hash":
            mask = self.brick_owner == rank
            self.owned_mask = torch.from_numpy(mask).to(self.device)
            self.owned_bricks = torch.from_numpy(np.nonzero(mask)[0].astype(np.int32)).to(self.device)
        self.with_color = True
        self.use_palette = True    # warped integrate through the skin cache's LDS node palette
        # per-frame brick cull in front of the palette integrate (ofx_integrate_palette_cull): bricks whose warped
        # voxels provably update nothing are skipped; bit-identical results
        self.brick_cull = True
        self._cull = None          # (tile maxima, per-slot flags) scratch of the cull
        # fusion_weight_params(...) or None: with it every staged / updated frame gets an observation-weight map
        # (obs_t) and integrate_device() fuses with it; None (the default) is the reference's plain running average
        self.fusion_weights = None
        self.obs_t = None          # the current frame's observation-weight map (H,W) f32, and its weight cap
        self.obs_wmax = float("inf")
        self._ones = None          # a constant-1 weight image: a cap without a weight image
        call("ofx_volume_reset", byref(self.desc), ptr(self.tsdf_b), ptr(self.weight_b), ptr(self.color_b), stream_ptr())
        self.warpfield = None
        self._world_pts = None
        self.log = log

    # ------------------------------------------------------------------ frame input
    def camera(self):
        c = _lib.Camera()
        c.fx, c.fy = float(self.cam_intr[0, 0]), float(self.cam_intr[1, 1])
        c.cx, c.cy = float(self.cam_intr[0, 2]), float(self.cam_intr[1, 2])
        c.height, c.width = int(self.depth_t.shape[0]), int(self.depth_t.shape[1])
        return c

    def _unpack(self, im):
        """(depth, packed colour) device tensors of a (6,H,W) frame; the colour packing is enqueued here."""
        im_t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im, dtype=np.float32))
        im_t = im_t.to(self.device, torch.float32, non_blocking=True)
        assert im_t.dim() == 3 and im_t.shape[0] >= 4, f"Input not correct: expected (6,H,W), got {tuple(im_t.shape)}"
        depth = im_t[-1].contiguous()
        H, W = depth.shape
        color = torch.empty((H, W), dtype=torch.float32, device=self.device)
        rgb = im_t[:3].contiguous()
        call("ofx_pack_color", ptr(rgb), H, W, ptr(color), stream_ptr())
        fw = self.fusion_weights
        if fw is None:
            return depth, color
        # the frame's observation weights, from the vertex and normal maps of the (filtered) frame; the integrated
        # depth stays the raw one. Holes stay holes under the filter: no pixel with raw depth gets a hole's weight 0.
        from .image_proc import prepare_depth_device
        K = self.cam_intr
        prep = prepare_depth_device(depth, K[0, 0], K[1, 1], K[0, 2], K[1, 2], edge_max=FUSION_EDGE_MAX, **fw["filter"])
        obs = torch.ops.ofx.observation_weights(prep["point_image"], prep["normals"], fw["cos_power"], fw["z_ref"],
                                                fw["w_floor"], fw["edge_weight"])
        return depth, color, obs, fw["max_weight"]

    def observation_weights(self, point_image, normal_image, cos_power=2, z_ref=1.0, w_floor=0.05, edge_weight=0.0):
        """The per-pixel observation weights (H,W) f32 of a frame for integrate(weight_image=), from
        prepare_depth_device's vertex map and normal map (3,H,W) (torch.ops.ofx.observation_weights ->
        ofx_observation_weights; new capability, no reference twin): max(w_floor, cos^cos_power · min(1, (z_ref/z)²))
        with cos the angle between the normal and the viewing ray (cos_power 0, 1 or 2; z_ref = 0: no range term),
        edge_weight where a pixel has depth but no normal (border, beside a hole, on a depth edge), 0 at holes. The
        defaults are conventions of volumetric fusion, not measurements. No host sync."""
        prm = observation_weight_params(cos_power, z_ref, w_floor, edge_weight)
        p = torch.as_tensor(point_image, dtype=torch.float32, device=self.device)
        n = torch.as_tensor(normal_image, dtype=torch.float32, device=self.device)
        return torch.ops.ofx.observation_weights(p, n, prm["cos_power"], prm["z_ref"], prm["w_floor"], prm["edge_weight"])

    def stage(self, im):
        """Unpack the frame that the next update(im, ...) will take, now: its device work (the colour packing) is
        enqueued at this point of the stream and update() only adopts the result. A frame loop stages frame t
        before frame t's solve, so the host work between the solve's return and the integrate launch shrinks (the
        GPU waits for it there). With fusion_weights set the frame's observation-weight map is built here too and
        rides along (a fourth and fifth entry: the map and its weight cap)."""
        self._staged = (im,) + self._unpack(im)

    def update(self, im, frame_id):
        """tsdf.py:545-572: unpack the (6,H,W) frame; depth = im[-1]; colour folded on device."""
        st = getattr(self, "_staged", None)
        self._staged = None
        un = st[1:] if st is not None and st[0] is im else self._unpack(im)
        self.depth_t, self.color_t = un[0], un[1]
        self.obs_t, self.obs_wmax = (un[2], un[3]) if len(un) > 2 else (None, float("inf"))
        self.im = im
        if hasattr(self, "frame_id"):
            skip = _opt(self.fopt, "skip_rate", 1)
            assert self.frame_id + skip == frame_id, \
                f"Updating image data failed. Previous frame:{self.frame_id}, current frame:{frame_id} not integrated."
        self.frame_id = frame_id

    @property
    def depth_im(self):
        return self.depth_t.cpu().numpy()

    @property
    def color_im(self):
        return self.color_t.cpu().numpy()

    # ------------------------------------------------------------------ integrate
    def integrate(self, image_data, obs_weight=1., weight_image=None, max_weight=None):
        """tsdf.py:378-494: warp (non-source frames) + integrate, fused on device. weight_image / max_weight: the
        weighted integrate (integrate_device)."""
        self._check_weighted(weight_image, max_weight)
        self.update(image_data["im"], image_data["id"])
        self.integrate_device(obs_weight, weight_image=weight_image, max_weight=max_weight)

    def _check_weighted(self, weight_image, max_weight):
        """The weighted integrate's arguments, checked before any device work -> (weighted?, w_max)."""
        w_max = max_weight_param(max_weight)
        on = weight_image is not None or max_weight is not None
        if on and self.semantics != "cpu":
            raise ValueError("the weighted integrate (weight_image / max_weight / fusion_weights) has 'cpu' semantics only")
        return on, w_max

    def _weight_image(self, weight_image):
        """(H,W) f32 contiguous device tensor of the current frame's size: weight_image, or ones for a cap alone."""
        H, W = (int(v) for v in self.depth_t.shape)
        if weight_image is None:
            if self._ones is None or tuple(self._ones.shape) != (H, W):
                self._ones = torch.ones((H, W), dtype=torch.float32, device=self.device)
            return self._ones
        w = torch.as_tensor(weight_image, dtype=torch.float32, device=self.device).contiguous()
        if tuple(w.shape) != (H, W):
            raise ValueError(f"weight_image must have the depth image's shape {(H, W)}, got {tuple(w.shape)}")
        return w

    def _op_geometry(self, obs_weight):
        """The integrate operators' arguments dims ... obs_weight: the shard, the camera and the frame's weight."""
        d, K = self.desc, self.cam_intr
        return ([int(v) for v in d.dim], [self.brick_x0, self.brick_x1], [float(v) for v in d.origin],
                float(d.voxel_size), float(d.trunc_margin), int(d.semantics),
                [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])], float(obs_weight))

    def _cull_scratch(self, n_list):
        """The brick cull's (tile maxima, per-slot flags), regrown when the frame or the brick list outgrows them."""
        H, W = (int(v) for v in self.depth_t.shape)
        nt = ((W + 7) // 8) * ((H + 7) // 8)
        if self._cull is None or self._cull[0].numel() < nt or self._cull[1].numel() < n_list:
            self._cull = (torch.empty(nt, dtype=torch.float32, device=self.device),
                          torch.empty(max(1, n_list), dtype=torch.uint8, device=self.device))
        return self._cull

    def integrate_device(self, obs_weight=1., count_updates=False, weight_image=None, max_weight=None):
        """Integrate the current (already updated) frame through torch.ops.ofx.integrate (the warped palette path:
        its library call directly); no host sync.

        weight_image ((H,W) f32, e.g. observation_weights(...)) and / or max_weight: the weighted integrate (new; the
        reference has none). A voxel's observation counts obs_weight · weight_image[its pixel] — a pixel whose weight
        is not a finite number > 0 updates nothing — and the stored weight is capped at max_weight, so the model keeps
        adapting. With both None, and no fusion_weights set on the volume, the calls are the unweighted ones, argument
        for argument; with fusion_weights set, the map built when the frame was staged / updated is used. Every path
        takes the weighted form of its operator or library entry (the same kernels' weighted forms) when a weight
        image is in force."""
        on, w_max = self._check_weighted(weight_image, max_weight)
        if not on and self.obs_t is not None:
            if self.semantics != "cpu":
                raise ValueError("fusion_weights needs 'cpu' integrate semantics")
            on, weight_image, w_max = True, self.obs_t, self.obs_wmax
        wi = self._weight_image(weight_image) if on else None
        color = self.color_b if self.with_color else None
        color_im = self.color_t if self.with_color else None
        nu = self.n_updated if count_updates else None

        def op(*warp):   # the paths off the frame loop: torch.ops.ofx.integrate(_weighted) with packed_nodes ... local
            f, tail = (torch.ops.ofx.integrate_weighted, (wi, w_max)) if on else (torch.ops.ofx.integrate, ())
            f(self.tsdf_b, self.weight_b, color, nu, self.depth_t, color_im, *self._op_geometry(obs_weight), *warp, *tail)

        if self.frame_id == _opt(self.fopt, "source_frame", 0):
            ob = self.owned_bricks
            return op(None, 0, 1, ob, 0 if ob is None else int(ob.shape[0]), None, None, None, None, None)
        if self.warpfield is None:
            raise RuntimeError("non-source frame integrate needs tsdf.warpfield (WarpField) to be set")
        cache = self.warpfield.skin_tsdf_cache()
        nodes = self.warpfield.packed_nodes()
        if not (self.use_palette and cache.pal_n is not None):   # global anchors
            return op(nodes, self.warpfield.num_nodes, cache.k, cache.brick_list, cache.n_list, cache.anchors,
                      cache.weights, None, None, None)
        # the frame loop's path: the library call of the operator's palette branch, made directly
        ow = _lib.ObsWeights(wi.data_ptr(), w_max, 0.0) if on else None
        scratch = self._cull_scratch(cache.n_list) if self.brick_cull else ()
        call("ofx_integrate_palette" + ("_cull" if self.brick_cull else "") + ("_w" if on else ""), byref(self.desc),
             byref(self.camera()), ptr(self.depth_t), ptr(color_im), ptr(nodes), self.warpfield.num_nodes, cache.k,
             ptr(cache.brick_list), cache.n_list, ptr(cache.anchors), ptr(cache.weights), ptr(cache.pal_ids),
             ptr(cache.pal_n), ptr(cache.local), float(obs_weight), ptr(self.tsdf_b), ptr(self.weight_b), ptr(color),
             ptr(nu), *(ptr(t) for t in scratch), *((byref(ow),) if on else ()), stream_ptr())

    def integrate_points(self, points, voxel_ids, valid=None, obs_weight=1., count_updates=False, weight_image=None,
                         max_weight=None):
        """tsdf.py:442-494 on explicit points: point p (already warped, e.g. WarpField.deform_tsdf) updates the
        voxel with C-order id voxel_ids[p] against the current frame (update() first). Voxel ids must be
        distinct; ids outside this shard are ignored. Returns the update count (device u32 tensor) if asked.
        weight_image / max_weight: the weighted integrate, as integrate_device takes them (a fusion_weights map of
        the volume is not applied here: explicit points come with explicit weights)."""
        on, w_max = self._check_weighted(weight_image, max_weight)
        pts = torch.as_tensor(points, dtype=torch.float32, device=self.device).reshape(-1, 3).contiguous()
        vox = torch.as_tensor(voxel_ids, dtype=torch.int64, device=self.device).reshape(-1).contiguous()
        if vox.shape[0] != pts.shape[0]:
            raise ValueError(f"{pts.shape[0]} points but {vox.shape[0]} voxel ids")
        v = None if valid is None else torch.as_tensor(valid, device=self.device).reshape(-1).to(torch.uint8)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device) if count_updates else None
        f, tail = ((torch.ops.ofx.integrate_points_weighted, (self._weight_image(weight_image), w_max)) if on else
                   (torch.ops.ofx.integrate_points, ()))
        f(self.tsdf_b, self.weight_b, self.color_b if self.with_color else None, cnt, self.depth_t,
          self.color_t if self.with_color else None, *self._op_geometry(obs_weight), pts, vox, v, *tail)
        return cnt

    def raycast(self, cam_intr=None, height=None, width=None, z_near=0.1, z_far=10.0):
        """Depth (H,W) f32 (0 = miss), normals (H,W,3) f32 and packed colours (H,W) f32 of the fused surface seen
        from the camera (identity pose) — device tensors (ofx_raycast). New capability: the reference renders
        no TSDF (its surfaces come from marching cubes); parity with oracle.raycast, unpinned against the
        reference. Needs the whole volume (an unsharded volume or shard world 1)."""
        if self.shard[1] != 1:
            raise ValueError("raycast needs the whole volume: gather a sharded volume first")
        K = self.cam_intr
        intr = [float(v) for v in (cam_intr if cam_intr is not None else (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))[:4]]
        if height is None or width is None:
            height, width = (int(x) for x in self.depth_t.shape)
        d = self.desc
        return torch.ops.ofx.raycast(self.tsdf_b, self.weight_b, self.color_b if self.with_color else None,
                                     [int(x) for x in d.dim], [float(x) for x in d.origin], float(d.voxel_size),
                                     float(d.trunc_margin), intr, int(height), int(width), float(z_near), float(z_far))

    @staticmethod
    def integrate_timing(enable=True):
        """(kernel ms, launches) of the warped integrate kernels since the last call, from hipEvents the library
        records around each launch on its stream (ofx_integrate_timing); then (re)arm or disarm recording."""
        ms, n = _lib.c_double(), _lib.c_int64()
        call("ofx_integrate_timing", 1 if enable else 0, byref(ms), byref(n))
        return ms.value, n.value

    # ------------------------------------------------------------------ readback
    def _dense(self, t):
        Dy, Dz = int(self._vol_dim[1]), int(self._vol_dim[2])
        out = torch.empty((self.x_hi - self.x_lo, Dy, Dz), dtype=torch.float32, device=self.device)
        call("ofx_volume_to_dense", byref(self.desc), ptr(t), ptr(out), stream_ptr())
        return out

    def voxel_rgb(self, voxel_ids):
        """The fused colour of voxels given by their C-order ids (as WarpField.surface_points' "voxel" column; whole
        volumes only) -> (P,3) f32 rgb in [0,1] on the device: id -> brick slot -> packed colour c -> b = floor(c /
        65536), g = floor((c - 65536 b) / 256), r = the rest, each divided by 255 (ofx_pack_color's inverse for 8-bit
        colours). An id outside the volume (the padding rows' -1) gives zeros. Torch integer math on torch's current
        stream, no host read; off the hot path."""
        if self.brick_x0 != 0 or self.n_slots != int(np.prod((self._vol_dim + 7) // 8)) * 512:
            raise ValueError("voxel_rgb needs a whole volume, not a shard")
        ids = voxel_ids if isinstance(voxel_ids, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(voxel_ids))
        ids = ids.to(device=self.device, dtype=torch.int64).reshape(-1)
        Dx, Dy, Dz = (int(x) for x in self._vol_dim)
        nby, nbz = (Dy + 7) // 8, (Dz + 7) // 8
        ok = (ids >= 0) & (ids < Dx * Dy * Dz)
        t = torch.where(ok, ids, torch.zeros_like(ids))
        k, r = t % Dz, t // Dz
        j, i = r % Dy, r // Dy
        slot = (((i // 8) * nby + j // 8) * nbz + k // 8) * 512 + ((i % 8) * 8 + j % 8) * 8 + k % 8
        c = self.color_b[slot].to(torch.int64)   # packed colours are integers below 2^24: exact in f32
        rgb = torch.stack([c % 256, (c // 256) % 256, c // 65536], 1).to(torch.float32) / 255.0
        return torch.where(ok[:, None], rgb, torch.zeros_like(rgb))

    def get_volume_device(self):
        """(tsdf, color, weight) C-order device tensors of this shard (x-slab [x_lo, x_hi))."""
        return self._dense(self.tsdf_b), self._dense(self.color_b), self._dense(self.weight_b)

    def get_volume(self):
        """tsdf.py:673-680: (tsdf, color, weight) numpy f32 (Dx_shard, Dy, Dz)."""
        return tuple(t.cpu().numpy() for t in self.get_volume_device())

    def save_volume(self, datapath):
        """Stacked (3,Dx,Dy,Dz) [tsdf, color, weight] as tsdf.py:682-687 — written with np.save (no pickle)."""
        data = np.stack(self.get_volume(), 0)
        with open(datapath, "wb") as f:
            np.save(f, data)

    def load_volume(self, datapath):
        data = np.load(datapath, allow_pickle=False)
        for arr, dst in zip(data, (self.tsdf_b, self.color_b, self.weight_b)):
            src = torch.from_numpy(np.ascontiguousarray(arr, np.float32)).to(self.device)
            call("ofx_volume_from_dense", byref(self.desc), ptr(src), ptr(dst), stream_ptr())
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ geometry helpers
    @property
    def world_pts(self):
        """vox2world over the C-order grid (tsdf.py:294-307,338-349), numpy (V_shard,3) f32."""
        if self._world_pts is None:
            o = self._vol_origin.astype(np.float64)
            vs = np.float64(self._voxel_size)
            axes = []
            rng = [(self.x_lo, self.x_hi), (0, int(self._vol_dim[1])), (0, int(self._vol_dim[2]))]
            for j, (a, b) in enumerate(rng):
                axes.append((o[j] + vs * np.arange(a, b, dtype=np.float32).astype(np.float64)).astype(np.float32))
            g = np.stack(np.meshgrid(*axes, indexing="ij"), -1)
            self._world_pts = g.reshape(-1, 3)
        return self._world_pts

    def check_visibility(self, points):
        """tsdf.py:599-612 -> (valid bool (P,), depth_diff f64 (P,)). numba types cam2pix by the array it gets
        (tsdf.py:351-364): float32 points (get_visible_nodes' deformed nodes) project in f32 (ofx_visibility_f32),
        float64 points (the integrate path's rigid_transform output) in f64 (ofx_visibility; their values must be
        f32-representable, as vox2world / ED-warp positions are)."""
        f32 = isinstance(points, np.ndarray) and points.dtype == np.float32 or (
            isinstance(points, torch.Tensor) and points.dtype == torch.float32)
        pts = torch.as_tensor(np.ascontiguousarray(points, np.float32) if isinstance(points, np.ndarray) else points,
                              device=self.device).to(torch.float32).contiguous()
        P = pts.shape[0]
        valid = torch.empty(P, dtype=torch.uint8, device=self.device)
        dd = torch.empty(P, dtype=torch.float64, device=self.device)
        cam = self.camera()
        call("ofx_visibility_f32" if f32 else "ofx_visibility", ptr(pts), P, byref(cam), ptr(self.depth_t),
             float(self._trunc_margin), ptr(valid), ptr(dd), stream_ptr())
        return valid.cpu().numpy().astype(bool), dd.cpu().numpy()

    def get_visible_nodes(self):
        """tsdf.py:614-638 (without the .npy side file): the warp field's f32 deformed nodes (g + T) checked
        against this frame's depth with the f32 projection numba gives them."""
        assert self.warpfield.frame_id == self.frame_id
        visible, _ = self.check_visibility(np.asarray(self.warpfield.get_deformed_nodes(), np.float32))
        return visible

    # ------------------------------------------------------------------ surface extraction
    @staticmethod
    def compute_truncated_region(tsdf_vol, max_diff):
        """tsdf.py:704-745 on a dense numpy (W,H,D) volume -> bool (W,H,D); computed by the HIP kernel."""
        t = np.ascontiguousarray(tsdf_vol, np.float32)
        desc = _lib.VolumeDesc()
        desc.dim[:] = [int(x) for x in t.shape]
        desc.brick_x0, desc.brick_x1 = 0, (t.shape[0] + 7) // 8
        desc.voxel_size, desc.trunc_margin = 1.0, TRUNC_MARGIN
        n = _lib.c_int64()
        call("ofx_volume_num_slots", byref(desc), byref(n))
        dev = torch.device("cuda", torch.cuda.current_device())
        src = torch.from_numpy(t).to(dev)
        br = torch.empty(int(n.value), dtype=torch.float32, device=dev)
        call("ofx_volume_from_dense", byref(desc), ptr(src), ptr(br), stream_ptr())
        m = torch.empty(int(n.value), dtype=torch.uint8, device=dev)
        call("ofx_truncated_region", byref(desc), ptr(br), float(max_diff), ptr(m), stream_ptr())
        mf = m.float()
        dense = torch.empty(t.shape, dtype=torch.float32, device=dev)
        call("ofx_volume_to_dense", byref(desc), ptr(mf), ptr(dense), stream_ptr())
        return dense.cpu().numpy() != 0

    def truncated_region_device(self, max_diff=1.2):
        """Bricked u8 mask of this (whole) volume's truncated region."""
        m = torch.empty(self.n_slots, dtype=torch.uint8, device=self.device)
        call("ofx_truncated_region", byref(self.desc), ptr(self.tsdf_b), float(max_diff), ptr(m), stream_ptr())
        return m

    def extract_mesh_device(self, use_mask=True, mask=None, level=0.0, max_diff=1.2, with_normals=True,
                            with_values=False, with_keys=False):
        """Marching cubes on the resident volume -> dict of device tensors: verts (V,3) f32 voxel
        coordinates, faces (F,3) int32 and optional normals / values / keys (include/ofx.h ofx_mesh_*)."""
        if getattr(self, "_mesh_h", None) is None:
            h = _lib.c_void_p()
            call("ofx_mesh_create", byref(h))
            self._mesh_h = h
        nv, nf = _lib.c_int64(), _lib.c_int64()
        call("ofx_mesh_count", self._mesh_h, byref(self.desc), ptr(self.tsdf_b), ptr(mask), float(max_diff),
             1 if use_mask else 0, float(level), byref(nv), byref(nf), stream_ptr())
        V, F = int(nv.value), int(nf.value)
        kw = dict(device=self.device)
        out = {"verts": torch.empty((V, 3), dtype=torch.float32, **kw),
               "faces": torch.empty((F, 3), dtype=torch.int32, **kw),
               "normals": torch.empty((V, 3), dtype=torch.float32, **kw) if with_normals else None,
               "values": torch.empty(V, dtype=torch.float32, **kw) if with_values else None,
               "keys": torch.empty(V, dtype=torch.int64, **kw) if with_keys else None}
        call("ofx_mesh_emit", self._mesh_h, ptr(out["verts"]), ptr(out["faces"]), ptr(out["normals"]),
             ptr(out["values"]), ptr(out["keys"]), stream_ptr())
        return out

    def brick_column_slots(self):
        """Voxel slots of one brick column (one x-brick of the bricked layout: ny·nz bricks of 512)."""
        return int((self._vol_dim[1] + 7) // 8) * int((self._vol_dim[2] + 7) // 8) * 512

    def _need_slab(self, what):
        if self.shard_kind != "slab":
            raise ValueError(f"{what} needs x-slab shards (a hash-bucket shard holds scattered bricks): gather the "
                             "volume (sharding.merge_hash_shards) or shard it as (rank, world, 'slab')")

    def boundary_columns(self):
        """(first, last) brick columns of this shard as (2, slots) device tensors [tsdf; colour] — what the
        neighbouring shards need as marching-cubes halo (sharding.exchange_boundary)."""
        self._need_slab("boundary_columns")
        c = self.brick_column_slots()
        first = torch.stack([self.tsdf_b[:c], self.color_b[:c]])
        last = torch.stack([self.tsdf_b[-c:], self.color_b[-c:]])
        return first, last

    def extract_mesh_shard(self, lo=None, hi=None, use_mask=True, level=0.0, max_diff=1.2, with_normals=True,
                           with_values=False):
        """Marching cubes of this shard's own cells (far corners in its x-slab) -> device dict: verts (V,3)
        voxel coordinates, faces (F,3) int32 into this part's vertices, keys (V,) int64, normals, values, world
        (V,3) f32 and colors (V,3) u8. lo / hi: the neighbours' last / first brick columns as (2, slots)
        [tsdf; colour] tensors (None at the volume's ends). sharding.merge_shard_meshes of the parts in rank
        order is the whole volume's extract_mesh_device + get_mesh colours, bit for bit (include/ofx.h
        ofx_mesh_count_range)."""
        self._need_slab("extract_mesh_shard")
        nbx = int((self._vol_dim[0] + 7) // 8)
        x0, x1 = self.brick_x0, self.brick_x1
        if (x0 > 0) != (lo is not None) or (x1 < nbx) != (hi is not None):
            raise ValueError(f"shard bricks [{x0},{x1}) of {nbx}: halo columns needed below: {x0 > 0}, above: {x1 < nbx}")
        c = self.brick_column_slots()
        for h in (lo, hi):
            if h is not None and tuple(h.shape) != (2, c):
                raise ValueError(f"halo column must be (2, {c}), got {tuple(h.shape)}")
        tsdf = torch.cat(([lo[0]] if lo is not None else []) + [self.tsdf_b] + ([hi[0]] if hi is not None else []))
        color = torch.cat(([lo[1]] if lo is not None else []) + [self.color_b] + ([hi[1]] if hi is not None else []))
        desc = _lib.VolumeDesc.from_buffer_copy(self.desc)
        desc.brick_x0 = x0 - (1 if lo is not None else 0)
        desc.brick_x1 = x1 + (1 if hi is not None else 0)
        if getattr(self, "_mesh_h", None) is None:
            h = _lib.c_void_p()
            call("ofx_mesh_create", byref(h))
            self._mesh_h = h
        nv, nf = _lib.c_int64(), _lib.c_int64()
        call("ofx_mesh_count_range", self._mesh_h, byref(desc), ptr(tsdf), None, float(max_diff), 1 if use_mask else 0,
             float(level), 8 * x0, min(8 * x1, int(self._vol_dim[0])), byref(nv), byref(nf), stream_ptr())
        V, F = int(nv.value), int(nf.value)
        kw = dict(device=self.device)
        out = {"verts": torch.empty((V, 3), dtype=torch.float32, **kw),
               "faces": torch.empty((F, 3), dtype=torch.int32, **kw),
               "normals": torch.empty((V, 3), dtype=torch.float32, **kw) if with_normals else None,
               "values": torch.empty(V, dtype=torch.float32, **kw) if with_values else None,
               "keys": torch.empty(V, dtype=torch.int64, **kw)}
        call("ofx_mesh_emit", self._mesh_h, ptr(out["verts"]), ptr(out["faces"]), ptr(out["normals"]),
             ptr(out["values"]), ptr(out["keys"]), stream_ptr())
        out["world"] = torch.empty((V, 3), dtype=torch.float32, **kw)
        out["colors"] = torch.empty((V, 3), dtype=torch.uint8, **kw)
        call("ofx_mesh_finish", byref(desc), ptr(color), ptr(out["verts"]), V, ptr(out["world"]), ptr(out["colors"]),
             stream_ptr())
        return out

    def _mesh_world_colors(self, verts):
        V = verts.shape[0]
        world = torch.empty((V, 3), dtype=torch.float32, device=self.device)
        colors = torch.empty((V, 3), dtype=torch.uint8, device=self.device)
        call("ofx_mesh_finish", byref(self.desc), ptr(self.color_b), ptr(verts), V, ptr(world), ptr(colors),
             stream_ptr())
        return world, colors

    def get_mesh(self):
        """tsdf.py:770-809: marching cubes of the truncated region (max_diff 1.2) -> (verts world f32 (V,3),
        faces (F,3), norms f32 (V,3), colors uint8 (V,3) [r,g,b]), numpy."""
        m = self.extract_mesh_device(use_mask=True, max_diff=1.2)
        world, colors = self._mesh_world_colors(m["verts"])
        return (world.cpu().numpy(), m["faces"].cpu().numpy().astype(np.int64), m["normals"].cpu().numpy(),
                colors.cpu().numpy())

    def get_point_cloud(self):
        """tsdf.py:748-768: unmasked marching-cubes vertices in world coordinates + colours -> (V,6)."""
        m = self.extract_mesh_device(use_mask=False, with_normals=False)
        world, colors = self._mesh_world_colors(m["verts"])
        return np.hstack([world.cpu().numpy(), colors.cpu().numpy()])

    def get_canonical_model(self):
        """tsdf.py:811-820 (cached until clear())."""
        if not hasattr(self, "canonical_model"):
            self.canonical_model = self.get_mesh()
        return self.canonical_model

    def get_deformed_model(self):
        """tsdf.py:829-845: canonical mesh warped to the current frame (WarpField.deform_mesh)."""
        if hasattr(self, "deformed_model"):
            return self.deformed_model
        src = _opt(self.fopt, "source_frame", 0)
        if self.frame_id != src:
            verts, faces, normals, colors = self.get_canonical_model()
            dv, dn, _, _, _ = self.warpfield.deform_mesh(verts, normals)
            self.deformed_model = (dv, faces, dn, colors)
        else:
            self.deformed_model = self.get_canonical_model()
        return self.deformed_model

    def __del__(self):
        h = getattr(self, "_mesh_h", None)
        if h is not None and h.value:
            try:
                _lib.lib.ofx_mesh_destroy(h)
            except Exception:
                pass
            self._mesh_h = None

    def clear(self):
        """tsdf.py:857-876."""
        for a in ("reduced_graph_dict", "deformed_model", "canonical_model"):
            if hasattr(self, a):
                delattr(self, a)
