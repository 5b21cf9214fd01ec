"""Skinned surface points of the TSDF: the tracking model, read off the volume itself.

The reference refreshes its model every frame with marching cubes and a k-NN skin of the vertices
(tsdf.get_deformed_model / optimizer.update, fusion_tests/lepard_nicp_test.py:471,537). Tracking needs no triangles:
SurfaceSampler takes canonical surface points, their outward normals and their anchors and weights from the bricked
volume and the skin cache in one pass over the cache's listed bricks (torch.ops.ofx.surface_points ->
ofx_surface_points). A point carries the cached skin of its voxel, the skin the integrate warps that voxel with, so the
tracked model and the fused model move identically. No reference twin; the contract is in include/ofx.h and restated
by tests/surface_ref.py.
"""
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.ofx.*)
from ._lib import byref, call

CODE_NAMES = ("accepted", "boundary", "unobserved", "off_band", "unobserved_neighbour", "not_at_zero_level",
              "degenerate_gradient", "invalid_skin")


class SurfaceSampler:
    """Owns an ofx_surface handle (per-brick counts, their scan and the accepted-voxel bit words for up to max_bricks
    listed bricks) and the output tensors of the last call, which are reused while the capacity stays the same."""

    def __init__(self, max_bricks, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_bricks = int(max_bricks)
        self._h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            call("ofx_surface_create", self.max_bricks, byref(self._h))
        self._state = torch.zeros(1, dtype=torch.int32, device=self.device)   # ofx::surface_points ordering token
        self._out = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib.ofx_surface_destroy(h)
            except Exception:
                pass
        self._h = None

    def _outputs(self, max_points, n_list, with_codes):
        o = self._out
        if (o is None or o[0].shape[0] != max_points or (with_codes and (o[6] is None or o[6].shape[0] < n_list * 512))):
            o = self._out = ops.surface_outputs(max_points, self.device, n_list if with_codes else None)
        return o

    def sample(self, vol, cache, max_points, w_min=1.0, with_codes=False):
        """Sample the whole volume `vol` (TSDFVolume) through the skin cache `cache` (WarpField.skin_tsdf_cache) into
        max_points padded rows -> dict(points (M,3), normals (M,3), anchors i32 (M,4), weights (M,4), voxel i32 (M,),
        valid u8 (M,), code u8 (n_list*512,) or None, count i32 (2,) = [accepted, emitted]), all on the device, enqueued
        on torch's current stream without a host read. The tensors are the sampler's own: the next call with the same
        capacity overwrites them."""
        if vol.brick_x0 != 0 or vol.brick_x1 != (int(vol._vol_dim[0]) + 7) // 8 or vol.owned_mask is not None:
            raise ValueError("surface points need the whole volume: a sharded TSDFVolume is not supported")
        if cache.k != 4:
            raise ValueError(f"surface points need a skin cache with K = 4 anchors, not {cache.k}")
        if cache.n_list > self.max_bricks:
            raise ValueError(f"{cache.n_list} listed bricks exceed the sampler's capacity ({self.max_bricks})")
        M = int(max_points)
        pts, nrm, a, w, vox, valid, code, count = self._outputs(M, cache.n_list, with_codes)
        d = vol.desc
        torch.ops.ofx.surface_points(self._state, self._h.value, vol.tsdf_b, vol.weight_b, cache.brick_list,
                                     cache.n_list, cache.anchors, cache.weights, cache.k, [int(v) for v in d.dim],
                                     [float(v) for v in d.origin], float(d.voxel_size), float(d.trunc_margin),
                                     float(w_min), pts, nrm, a, w, vox, valid, code if with_codes else None, count)
        return {"points": pts, "normals": nrm, "anchors": a, "weights": w, "voxel": vox, "valid": valid,
                "code": code[:cache.n_list * 512] if with_codes else None, "count": count}
