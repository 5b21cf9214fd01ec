"""PyTorch-ROCm custom operators over the libofx C ABI: `torch.ops.ofx.*` (torch.library).

The shims (TSDFVolume, WarpField, GaussNewtonSolver) call these operators, so the fusion hot path is
visible to the dispatcher, to FakeTensor / meta tracing and to graph capture with the kernels still the
hand-written HIP ones in libofx.so. Conventions:

* every operator is registered for the CUDA (= HIP) dispatch key only: CPU tensors raise
  NotImplementedError ("no kernel for CPU") — there is no CPU fallback;
* work is enqueued on torch's current stream of the tensors' device, asynchronously (no host sync);
* in-place outputs are declared in the schema (`Tensor(a!)`), so functionalisation sees the mutation;
* the GN operators take the solver handle (an `int`, the C pointer) and a one-element `state` tensor that
  they declare mutated: the handle's scratch (warm-start ring, preconditioner, row order) is hidden state,
  and the declared mutation keeps two solves on one handle ordered under any graph transformation;
* every operator has a fake (meta) kernel giving output shapes and dtypes without a device.

Registration is the low-level `torch.library.Library` form (schema inferred from the Python signature exactly
as `torch.library.custom_op` would, CUDA kernel + fake kernel) rather than the `custom_op` decorator: the
decorator's Python-side autograd / mutation wrapping costs ≈ 50 µs per call on the host, and the fusion loop
issues two of these calls per frame on its critical path (measured: 69 vs 19 µs per 18-argument call).

Reference call sites these operators replace: TSDFVolume.integrate (fusion_with_occlusion/tsdf.py:378-494),
WarpField.skin / deform (warpfield.py:83-129, 270-305, 369-380), DeformNet.optimize (model/model.py:222-859).
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import byref, call, ptr, stream_ptr

_NS = "ofx"
_LIB = torch.library.Library(_NS, "FRAGMENT")


class _Op:
    """One registered operator: `fn` is its CUDA kernel; `register_fake` attaches the meta kernel."""

    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __call__(self, *args):
        return getattr(torch.ops.ofx, self.name)(*args)

    def register_fake(self, fake):
        torch.library.register_fake(f"{_NS}::{self.name}", fake, lib=_LIB)
        return fake


def _op(name, mutates_args):
    def deco(fn):
        _LIB.define(name + torch.library.infer_schema(fn, mutates_args=mutates_args))
        _LIB.impl(name, fn, "CUDA")
        return _Op(name, fn)
    return deco


def _volume_desc(dims, brick_range, origin, voxel_size, trunc_margin, semantics):
    d = _lib.VolumeDesc()
    d.dim[:] = [int(x) for x in dims]
    d.brick_x0, d.brick_x1 = int(brick_range[0]), int(brick_range[1])
    d.origin[:] = [float(x) for x in origin]
    d.voxel_size, d.trunc_margin, d.semantics = float(voxel_size), float(trunc_margin), int(semantics)
    return d


def _camera(intr, height, width):
    c = _lib.Camera()
    c.fx, c.fy, c.cx, c.cy = (float(v) for v in intr[:4])
    c.height, c.width = int(height), int(width)
    return c


def _stream(t):
    return stream_ptr(torch.cuda.current_stream(t.device))


# --------------------------------------------------------------------------------------------- integrate
def _obs_weights(obs_im, depth, w_max):
    if obs_im.dtype != torch.float32 or tuple(obs_im.shape) != tuple(depth.shape):
        raise ValueError(f"weighted integrate: obs_im must be float32 of the depth's shape {tuple(depth.shape)}, got "
                         f"{obs_im.dtype} {tuple(obs_im.shape)}")
    if not obs_im.is_contiguous():
        raise ValueError("weighted integrate: obs_im must be contiguous")
    return _lib.ObsWeights(obs_im.data_ptr(), float(w_max), 0.0)


def _integrate_call(ow, name, frame, *args):
    """The one library call of an integrate operator: entry point `name` with the arguments `frame` that all four
    operators begin with (tsdf ... obs_weight) and its own `args`; with observation weights ow (_obs_weights; None:
    unweighted) its _w form, which takes ow in front of the stream."""
    (tsdf, weight, color, n_updated, depth, color_im, dims, brick_range, origin, voxel_size, trunc_margin, semantics, intr,
     obs_weight) = frame
    desc = _volume_desc(dims, brick_range, origin, voxel_size, trunc_margin, semantics)
    cam = _camera(intr, depth.shape[0], depth.shape[1])
    call(name if ow is None else name + "_w", byref(desc), byref(cam), ptr(depth), ptr(color_im), *args,
         float(obs_weight), ptr(tsdf), ptr(weight), ptr(color), ptr(n_updated), *(() if ow is None else (byref(ow),)),
         _stream(tsdf))


def _integrate(ow, *a):
    """integrate (ow None) / integrate_weighted: a = integrate's arguments."""
    frame, (packed_nodes, n_nodes, k, brick_list, n_list, anchors, weights, pal_ids, pal_n, local) = a[:14], a[14:]
    if packed_nodes is None:   # source frame; brick_list: a hash shard's own bricks (None: all of the shard)
        _integrate_call(ow, "ofx_integrate", frame, 0, None, 0, 1, ptr(brick_list), n_list, None, None)
    elif pal_ids is not None:
        _integrate_call(ow, "ofx_integrate_palette", frame, ptr(packed_nodes), n_nodes, k, ptr(brick_list), n_list,
                        ptr(anchors), ptr(weights), ptr(pal_ids), ptr(pal_n), ptr(local))
    else:
        _integrate_call(ow, "ofx_integrate", frame, 1, ptr(packed_nodes), n_nodes, k, ptr(brick_list), n_list,
                        ptr(anchors), ptr(weights))


def _integrate_points(ow, *a):
    """integrate_points (ow None) / integrate_points_weighted: a = integrate_points' arguments."""
    frame, (points, voxel_ids, valid) = a[:14], a[14:]
    _integrate_call(ow, "ofx_integrate_points", frame, ptr(points), ptr(voxel_ids), ptr(valid), points.shape[0])


def _no_result(*args):
    """The fake kernel of the four integrate operators: they mutate their first arguments and return nothing."""
    return None

@_op("integrate", mutates_args=("tsdf", "weight", "color", "n_updated"))
def integrate(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], n_updated: Optional[Tensor], depth: Tensor,
              color_im: Optional[Tensor], dims: List[int], brick_range: List[int], origin: List[float],
              voxel_size: float, trunc_margin: float, semantics: int, intr: List[float], obs_weight: float,
              packed_nodes: Optional[Tensor], n_nodes: int, k: int, brick_list: Optional[Tensor], n_list: int,
              anchors: Optional[Tensor], weights: Optional[Tensor], pal_ids: Optional[Tensor],
              pal_n: Optional[Tensor], local: Optional[Tensor]) -> None:
    """TSDFVolume.integrate's device work (tsdf.py:378-494): source frame when packed_nodes is None
    (ofx_integrate warp=0), else the fused skin-cache ED warp + integrate of the listed bricks — through the
    LDS node palette when pal_ids is given (ofx_integrate_palette), with global node gathers otherwise."""
    _integrate(None, tsdf, weight, color, n_updated, depth, color_im, dims, brick_range, origin, voxel_size, trunc_margin,
               semantics, intr, obs_weight, packed_nodes, n_nodes, k, brick_list, n_list, anchors, weights, pal_ids, pal_n,
               local)


integrate.register_fake(_no_result)


@_op("integrate_points", mutates_args=("tsdf", "weight", "color", "n_updated"))
def integrate_points(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], n_updated: Optional[Tensor],
                     depth: Tensor, color_im: Optional[Tensor], dims: List[int], brick_range: List[int],
                     origin: List[float], voxel_size: float, trunc_margin: float, semantics: int, intr: List[float],
                     obs_weight: float, points: Tensor, voxel_ids: Tensor, valid: Optional[Tensor]) -> None:
    """TSDFVolume.integrate of given (already deformed) points into the voxels `voxel_ids` (C-order ids,
    distinct): tsdf.py:442-494 with pts from WarpField.deform_tsdf (warpfield.py:369-380)."""
    _integrate_points(None, tsdf, weight, color, n_updated, depth, color_im, dims, brick_range, origin, voxel_size,
                      trunc_margin, semantics, intr, obs_weight, points, voxel_ids, valid)


integrate_points.register_fake(_no_result)


@_op("integrate_weighted", mutates_args=("tsdf", "weight", "color", "n_updated"))
def integrate_weighted(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], n_updated: Optional[Tensor], depth: Tensor,
                       color_im: Optional[Tensor], dims: List[int], brick_range: List[int], origin: List[float],
                       voxel_size: float, trunc_margin: float, semantics: int, intr: List[float], obs_weight: float,
                       packed_nodes: Optional[Tensor], n_nodes: int, k: int, brick_list: Optional[Tensor], n_list: int,
                       anchors: Optional[Tensor], weights: Optional[Tensor], pal_ids: Optional[Tensor],
                       pal_n: Optional[Tensor], local: Optional[Tensor], obs_im: Tensor, w_max: float) -> None:
    """torch.ops.ofx.integrate with a per-pixel observation-weight image obs_im (f32, the depth's shape) and a cap w_max
    on the stored weight (inf: none): ofx_integrate_w / ofx_integrate_palette_w (new capability, CPU semantics only; off
    by default — nothing calls it unless a weight image or a cap is asked for)."""
    _integrate(_obs_weights(obs_im, depth, w_max), tsdf, weight, color, n_updated, depth, color_im, dims, brick_range,
               origin, voxel_size, trunc_margin, semantics, intr, obs_weight, packed_nodes, n_nodes, k, brick_list, n_list,
               anchors, weights, pal_ids, pal_n, local)


integrate_weighted.register_fake(_no_result)


@_op("integrate_points_weighted", mutates_args=("tsdf", "weight", "color", "n_updated"))
def integrate_points_weighted(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], n_updated: Optional[Tensor],
                              depth: Tensor, color_im: Optional[Tensor], dims: List[int], brick_range: List[int],
                              origin: List[float], voxel_size: float, trunc_margin: float, semantics: int,
                              intr: List[float], obs_weight: float, points: Tensor, voxel_ids: Tensor,
                              valid: Optional[Tensor], obs_im: Tensor, w_max: float) -> None:
    """torch.ops.ofx.integrate_points with an observation-weight image and a weight cap (ofx_integrate_points_w)."""
    _integrate_points(_obs_weights(obs_im, depth, w_max), tsdf, weight, color, n_updated, depth, color_im, dims,
                      brick_range, origin, voxel_size, trunc_margin, semantics, intr, obs_weight, points, voxel_ids, valid)


integrate_points_weighted.register_fake(_no_result)


@_op("observation_weights", mutates_args=())
def observation_weights(point_image: Tensor, normal_image: Tensor, cos_power: int, z_ref: float, w_floor: float,
                        edge_weight: float) -> Tensor:
    """ofx_observation_weights (new capability, no reference twin): the per-pixel observation weight (H,W) f32 of a frame
    from ofx_prepare_depth's vertex map and normal map, (3,H,W) f32 each — an angle term cos^cos_power of the normal
    against the viewing ray, a range term min(1, (z_ref / z)^2) (z_ref = 0: none), floored at w_floor; edge_weight where
    a pixel has depth but no normal, 0 at holes."""
    if point_image.dim() != 3 or point_image.shape[0] != 3 or tuple(normal_image.shape) != tuple(point_image.shape):
        raise ValueError(f"observation_weights: point_image and normal_image must both be (3, H, W), got "
                         f"{tuple(point_image.shape)} and {tuple(normal_image.shape)}")
    if point_image.dtype != torch.float32 or normal_image.dtype != torch.float32:
        raise ValueError("observation_weights: point_image and normal_image must be float32")
    p, n = point_image.contiguous(), normal_image.contiguous()
    H, W = int(p.shape[1]), int(p.shape[2])
    prm = _lib.ObsParams(int(cos_power), float(z_ref), float(w_floor), float(edge_weight))
    out = torch.empty((H, W), dtype=torch.float32, device=p.device)
    call("ofx_observation_weights", ptr(p), ptr(n), H, W, byref(prm), ptr(out), _stream(p))
    return out


@observation_weights.register_fake
def _(point_image, normal_image, cos_power, z_ref, w_floor, edge_weight):
    return point_image.new_empty((point_image.shape[1], point_image.shape[2]), dtype=torch.float32)


@_op("raycast", mutates_args=())
def raycast(tsdf: Tensor, weight: Tensor, color: Optional[Tensor], dims: List[int], origin: List[float],
            voxel_size: float, trunc_margin: float, intr: List[float], height: int, width: int, z_near: float,
            z_far: float) -> Tuple[Tensor, Tensor, Tensor]:
    """Depth (H,W), normals (H,W,3) and packed colours (H,W) of the fused surface seen from the camera
    (ofx_raycast; new capability, no reference twin)."""
    nbx = (int(dims[0]) + 7) // 8
    desc = _volume_desc(dims, [0, nbx], origin, voxel_size, trunc_margin, 0)
    cam = _camera(intr, height, width)
    depth = torch.empty((height, width), dtype=torch.float32, device=tsdf.device)
    normals = torch.empty((height, width, 3), dtype=torch.float32, device=tsdf.device)
    colors = torch.empty((height, width), dtype=torch.float32, device=tsdf.device)
    call("ofx_raycast", byref(desc), byref(cam), ptr(tsdf), ptr(weight), ptr(color), float(z_near), float(z_far),
         ptr(depth), ptr(normals), ptr(colors), _stream(tsdf))
    return depth, normals, colors


@raycast.register_fake
def _(tsdf, weight, color, dims, origin, voxel_size, trunc_margin, intr, height, width, z_near, z_far):
    return (tsdf.new_empty((height, width)), tsdf.new_empty((height, width, 3)), tsdf.new_empty((height, width)))


# --------------------------------------------------------------------------------------------- skinning
@_op("skin_points", mutates_args=())
def skin_points(points: Tensor, nodes: Tensor, node_coverage: float, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """WarpField.skin (warpfield.py:83-129): k nearest nodes, exp(-d²/2σ²) weights normalised by Σ + 1e-6,
    4σ cut-off -> (anchors int32 (P,k), weights f32 (P,k), valid bool (P,))."""
    P = points.shape[0]
    anchors = torch.empty((P, k), dtype=torch.int32, device=points.device)
    weights = torch.empty((P, k), dtype=torch.float32, device=points.device)
    valid = torch.empty(P, dtype=torch.uint8, device=points.device)
    call("ofx_skin_points", ptr(points), P, ptr(nodes), nodes.shape[0], float(node_coverage), int(k), ptr(anchors),
         ptr(weights), ptr(valid), _stream(points))
    return anchors, weights, valid.bool()


@skin_points.register_fake
def _(points, nodes, node_coverage, k):
    P = points.shape[0]
    return (points.new_empty((P, k), dtype=torch.int32), points.new_empty((P, k), dtype=torch.float32),
            points.new_empty((P,), dtype=torch.bool))


# --------------------------------------------------------------------------------------------- warp
@_op("deform_points", mutates_args=())
def deform_points(points: Tensor, anchors: Tensor, weights: Tensor, valid: Optional[Tensor], packed_nodes: Tensor,
                  normals: bool) -> Tensor:
    """ED_warp (NonRigidICP/model/geometry.py:9-25) of points with their skin; normals=True: the rotation-only
    blend of WarpField.deform_normals (warpfield.py:312-345). Points with valid == 0 keep their position."""
    out = torch.empty_like(points)
    v = None if valid is None else valid.to(torch.uint8)
    call("ofx_deform_points", ptr(points), points.shape[0], ptr(anchors), ptr(weights), ptr(v), anchors.shape[1],
         ptr(packed_nodes), packed_nodes.shape[0], 1 if normals else 0, ptr(out), _stream(points))
    return out


@deform_points.register_fake
def _(points, anchors, weights, valid, packed_nodes, normals):
    return torch.empty_like(points)


# --------------------------------------------------------------------------------------------- data association
@_op("associate", mutates_args=("state",))
def associate(state: Tensor, handle: int, points: Tensor, normals: Optional[Tensor], anchors: Tensor, weights: Tensor,
              valid: Optional[Tensor], packed_nodes: Tensor, point_image: Tensor, intr: List[float], dist_max: float,
              cos_min: float, edge_max: float, target_mode: int, max_matches: int
              ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """ofx_associate (new capability, no reference twin): projective association of the points (P,3), skinned with
    anchors / weights (P,4), warped by packed_nodes, with the vertex map point_image (3,H,W) -> per point code u8 (P,)
    (0 = accepted, 1..6 the first gate that rejected it), tgt (P,3), warped (P,3); compacted, at their full max_matches
    size (rows past count[1] are zero): match_idx i32, src (.,3), tgt (.,3), anchors i32 (.,4), weights (.,4); count
    int32[2] on the device = [accepted, emitted]. target_mode: 0 point, 1 plane foot (not `mode`: that name is taken by
    torch's functionalisation wrapper). `handle` is an ofx_assoc_create handle
    sized for at least P points; `state` is its ordering token (its scratch is hidden state)."""
    P, M = points.shape[0], int(max_matches)
    dev = points.device
    _, H, W = point_image.shape
    cam = _camera(intr, H, W)
    prm = _lib.AssocParams(float(dist_max), float(cos_min), float(edge_max), int(target_mode), M, 0)
    v = None if valid is None else valid.to(torch.uint8)
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt = torch.empty((P, 3), dtype=torch.float32, device=dev)
    warped = torch.empty((P, 3), dtype=torch.float32, device=dev)
    midx = torch.zeros(M, dtype=torch.int32, device=dev)
    src_o = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    tgt_o = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    a_o = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    w_o = torch.zeros((M, 4), dtype=torch.float32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    call("ofx_associate", _lib.c_void_p(handle), ptr(points), ptr(normals), ptr(anchors), ptr(weights), ptr(v), P,
         ptr(packed_nodes), packed_nodes.shape[0], byref(cam), ptr(point_image), H, W, byref(prm), ptr(code), ptr(tgt),
         ptr(warped), ptr(midx), ptr(src_o), ptr(tgt_o), ptr(a_o), ptr(w_o), ptr(count), _stream(points))
    return code, tgt, warped, midx, src_o, tgt_o, a_o, w_o, count


@associate.register_fake
def _(state, handle, points, normals, anchors, weights, valid, packed_nodes, point_image, intr, dist_max, cos_min,
      edge_max, target_mode, max_matches):
    P, M = points.shape[0], int(max_matches)
    f, i = torch.float32, torch.int32
    return (points.new_empty((P,), dtype=torch.uint8), points.new_empty((P, 3), dtype=f),
            points.new_empty((P, 3), dtype=f), points.new_empty((M,), dtype=i), points.new_empty((M, 3), dtype=f),
            points.new_empty((M, 3), dtype=f), points.new_empty((M, 4), dtype=i), points.new_empty((M, 4), dtype=f),
            points.new_empty((2,), dtype=i))


# --------------------------------------------------------------------------------------------- photometric association
@_op("photo_associate", mutates_args=("state",))
def photo_associate(state: Tensor, handle: int, points: Tensor, normals: Optional[Tensor], colors: Tensor,
                    anchors: Tensor, weights: Tensor, valid: Optional[Tensor], packed_nodes: Tensor,
                    point_image: Tensor, normal_image: Tensor, color_image: Tensor, intr: List[float], dist_max: float,
                    cos_min: float, color_max: float, geo_weight: float, radius: int, max_matches: int
                    ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor,
                               Tensor]:
    """ofx_photo_associate (new capability, no reference twin): for every point (P,3) with colour colors (P,3) — skinned
    and warped as in `associate` — the best colour match in the (2·radius + 1)² window around its pixel among the pixels
    of point_image / normal_image / color_image (3,H,W each) that pass associate's gates -> per point code u8 (P,) (0 =
    matched, 1..7), tgt (P,3), warped (P,3), pixel i32 (P,2), cost (P,); compacted, at their full max_matches size (rows
    past count[1] are zero): match_idx i32, src (.,3), tgt (.,3), anchors i32 (.,4), weights (.,4), pixel (.,2) f32; count
    int32[2] on the device = [accepted, emitted]. `handle` is an ofx_assoc_create handle sized for at least P points;
    `state` is its ordering token (its scratch is hidden state)."""
    P, M = points.shape[0], int(max_matches)
    dev = points.device
    _, H, W = point_image.shape
    if normal_image.shape != point_image.shape or color_image.shape != point_image.shape:
        raise ValueError("photo_associate: point, normal and colour image must all be (3, H, W)")
    if colors.shape[0] != P or colors.shape[1] != 3:
        raise ValueError(f"photo_associate: colors must be ({P}, 3), got {tuple(colors.shape)}")
    cam = _camera(intr, H, W)
    prm = _lib.PhotoParams(float(dist_max), float(cos_min), float(color_max), float(geo_weight), int(radius), M)
    v = None if valid is None else valid.to(torch.uint8)
    f, i = torch.float32, torch.int32
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    tgt = torch.empty((P, 3), dtype=f, device=dev)
    warped = torch.empty((P, 3), dtype=f, device=dev)
    pixel = torch.empty((P, 2), dtype=i, device=dev)
    cost = torch.empty(P, dtype=f, device=dev)
    midx = torch.zeros(M, dtype=i, device=dev)
    src_o = torch.zeros((M, 3), dtype=f, device=dev)
    tgt_o = torch.zeros((M, 3), dtype=f, device=dev)
    a_o = torch.zeros((M, 4), dtype=i, device=dev)
    w_o = torch.zeros((M, 4), dtype=f, device=dev)
    px_o = torch.zeros((M, 2), dtype=f, device=dev)
    count = torch.empty(2, dtype=i, device=dev)
    call("ofx_photo_associate", _lib.c_void_p(handle), ptr(points), ptr(normals), ptr(colors), ptr(anchors),
         ptr(weights), ptr(v), P, ptr(packed_nodes), packed_nodes.shape[0], byref(cam), ptr(point_image),
         ptr(normal_image), ptr(color_image), H, W, byref(prm), ptr(code), ptr(tgt), ptr(warped), ptr(pixel), ptr(cost),
         ptr(midx), ptr(src_o), ptr(tgt_o), ptr(a_o), ptr(w_o), ptr(px_o), ptr(count), _stream(points))
    return code, tgt, warped, pixel, cost, midx, src_o, tgt_o, a_o, w_o, px_o, count


@photo_associate.register_fake
def _(state, handle, points, normals, colors, anchors, weights, valid, packed_nodes, point_image, normal_image,
      color_image, intr, dist_max, cos_min, color_max, geo_weight, radius, max_matches):
    P, M = points.shape[0], int(max_matches)
    f, i = torch.float32, torch.int32
    return (points.new_empty((P,), dtype=torch.uint8), points.new_empty((P, 3), dtype=f),
            points.new_empty((P, 3), dtype=f), points.new_empty((P, 2), dtype=i), points.new_empty((P,), dtype=f),
            points.new_empty((M,), dtype=i), points.new_empty((M, 3), dtype=f), points.new_empty((M, 3), dtype=f),
            points.new_empty((M, 4), dtype=i), points.new_empty((M, 4), dtype=f), points.new_empty((M, 2), dtype=f),
            points.new_empty((2,), dtype=i))


# --------------------------------------------------------------------------------------------- sub-pixel match refinement
@_op("photo_refine", mutates_args=("px_out", "tgt_out", "status", "ssd"))
def photo_refine(template_image: Tensor, template_mask: Optional[Tensor], color_image: Tensor, point_image: Tensor,
                 template_px: Tensor, init_px: Tensor, tgt_in: Tensor, count: Tensor, half: int, iters: int, eps: float,
                 max_shift: float, min_eig: float, ssd_max: float, edge_max: float, px_out: Tensor, tgt_out: Tensor,
                 status: Tensor, ssd: Tensor) -> None:
    """ofx_photo_refine (new capability, no reference twin): the translation-only inverse compositional Lucas-Kanade
    refinement of photo_associate's matches. template_image / color_image / point_image f32 (3,H,W); template_mask u8 or
    bool (H,W) or None; template_px / init_px f32 (R,2); tgt_in f32 (R,3); count: photo_associate's int32[2] on the
    device (the rows are the first min(count[1], R)). Written in place for those rows, the rest left untouched: px_out
    f32 (R,2), tgt_out f32 (R,3), status u8 (R,), ssd f32 (R,). No handle, no hidden state."""
    R = init_px.shape[0]
    _, H, W = color_image.shape
    f = torch.float32
    if template_image.shape != color_image.shape or point_image.shape != color_image.shape or color_image.shape[0] != 3:
        raise ValueError("photo_refine: template, colour and point image must all be (3, H, W)")
    for name, t, shape, dt in (("template_image", template_image, (3, H, W), f), ("color_image", color_image, (3, H, W), f),
                               ("point_image", point_image, (3, H, W), f), ("template_px", template_px, (R, 2), f),
                               ("init_px", init_px, (R, 2), f), ("tgt_in", tgt_in, (R, 3), f),
                               ("count", count, (2,), torch.int32), ("px_out", px_out, (R, 2), f),
                               ("tgt_out", tgt_out, (R, 3), f), ("status", status, (R,), torch.uint8),
                               ("ssd", ssd, (R,), f)):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"photo_refine: {name} must be a contiguous {dt} tensor of shape {shape}")
    m = None
    if template_mask is not None:
        if tuple(template_mask.shape) != (H, W):
            raise ValueError(f"photo_refine: template_mask must be ({H}, {W})")
        m = template_mask.to(torch.uint8).contiguous()
    prm = _lib.RefineParams(int(half), int(iters), float(eps), float(max_shift), float(min_eig), float(ssd_max),
                            float(edge_max), 0)
    call("ofx_photo_refine", ptr(template_image), ptr(m), ptr(color_image), ptr(point_image), ptr(template_px),
         ptr(init_px), ptr(tgt_in), ptr(count), R, H, W, byref(prm), ptr(px_out), ptr(tgt_out), ptr(status), ptr(ssd),
         _stream(init_px))


@photo_refine.register_fake
def _(template_image, template_mask, color_image, point_image, template_px, init_px, tgt_in, count, half, iters, eps,
      max_shift, min_eig, ssd_max, edge_max, px_out, tgt_out, status, ssd):
    return None


# --------------------------------------------------------------------------------------------- rigid pre-alignment
@_op("rigid_icp", mutates_args=("state", "pose"))
def rigid_icp(state: Tensor, handle: int, points: Tensor, normals: Optional[Tensor], anchors: Tensor, weights: Tensor,
              valid: Optional[Tensor], packed_nodes: Tensor, point_image: Tensor, intr: List[float], dist_max: float,
              cos_min: float, edge_max: float, iters: int, min_matches: int, damping: float, stop_twist: float,
              pose: Tensor) -> Tuple[Tensor, Tensor]:
    """ofx_rigid_icp (new capability, no reference twin): `iters` point-to-plane ICP iterations of all the points (P,3)
    — skinned and warped as in `associate`, then moved by pose — against the vertex map point_image (3,H,W), with
    associate's gates. pose: f64 (3,4) [R|t] on the device, updated in place. -> code u8 (P,) of the last iteration that
    ran, systems f64 (iters, 32): per iteration the 21 upper entries of A, b, Σr², the accepted count, the status (0
    solved, 1 too few matches, 2 non-positive pivot, 3 drained), |ω|, |v|. `handle` is an ofx_rigid_create handle sized
    for at least P points; `state` is its ordering token (its scratch is hidden state)."""
    P = points.shape[0]
    dev = points.device
    _, H, W = point_image.shape
    if pose.dtype != torch.float64 or pose.numel() != 12 or not pose.is_contiguous():
        raise ValueError("rigid_icp: pose must be a contiguous float64 tensor of 12 elements ([R|t], row-major)")
    cam = _camera(intr, H, W)
    prm = _lib.RigidParams(float(dist_max), float(cos_min), float(edge_max), int(iters), int(min_matches),
                           float(damping), float(stop_twist))
    v = None if valid is None else valid.to(torch.uint8)
    code = torch.zeros(P, dtype=torch.uint8, device=dev)
    systems = torch.empty((int(iters), 32), dtype=torch.float64, device=dev)
    call("ofx_rigid_icp", _lib.c_void_p(handle), ptr(points), ptr(normals), ptr(anchors), ptr(weights), ptr(v), P,
         ptr(packed_nodes), packed_nodes.shape[0], byref(cam), ptr(point_image), H, W, byref(prm), ptr(pose), ptr(code),
         ptr(systems), _stream(points))
    return code, systems


@rigid_icp.register_fake
def _(state, handle, points, normals, anchors, weights, valid, packed_nodes, point_image, intr, dist_max, cos_min,
      edge_max, iters, min_matches, damping, stop_twist, pose):
    return (points.new_empty((points.shape[0],), dtype=torch.uint8),
            points.new_empty((int(iters), 32), dtype=torch.float64))


# --------------------------------------------------------------------------------------------- model z-buffer
@_op("splat_points", mutates_args=("state",))
def splat_points(state: Tensor, handle: int, points: Tensor, normals: Optional[Tensor], anchors: Tensor, weights: Tensor,
                 valid: Optional[Tensor], packed_nodes: Tensor, intr: List[float], height: int, width: int,
                 splat_radius: float, occl_margin: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """ofx_splat_points (new capability, no reference twin): the z-buffer of the points (P,3) — skinned and warped as in
    `associate`, each a disc of world radius splat_radius facing along its warped normal — in a height x width image
    under intr -> depth f32 (H,W) (0 = nothing), index i32 (H,W) (the point that owns the pixel, -1 = nothing), code u8
    (P,) (0 visible, 1 invalid skin, 2 off the image / behind / non-finite, 3 back-facing, 4 occluded: more than
    occl_margin behind the buffer at its own pixel), warped (P,3), warped_normals (P,3) ((0,3) without normals).
    `handle` is an ofx_splat_create handle sized for at least P points and height·width pixels; `state` is its ordering
    token (its z-buffer is hidden state)."""
    P = points.shape[0]
    dev = points.device
    H, W = int(height), int(width)
    cam = _camera(intr, H, W)
    prm = _lib.SplatParams(float(splat_radius), float(occl_margin))
    v = None if valid is None else valid.to(torch.uint8)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    index = torch.empty((H, W), dtype=torch.int32, device=dev)
    code = torch.empty(P, dtype=torch.uint8, device=dev)
    warped = torch.empty((P, 3), dtype=torch.float32, device=dev)
    wn = torch.empty((P if normals is not None else 0, 3), dtype=torch.float32, device=dev)
    call("ofx_splat_points", _lib.c_void_p(handle), ptr(points), ptr(normals), ptr(anchors), ptr(weights), ptr(v), P,
         ptr(packed_nodes), packed_nodes.shape[0], byref(cam), byref(prm), ptr(depth), ptr(index), ptr(code),
         ptr(warped), ptr(wn) if normals is not None else None, _stream(points))
    return depth, index, code, warped, wn


@splat_points.register_fake
def _(state, handle, points, normals, anchors, weights, valid, packed_nodes, intr, height, width, splat_radius,
      occl_margin):
    P, f = points.shape[0], torch.float32
    return (points.new_empty((height, width), dtype=f), points.new_empty((height, width), dtype=torch.int32),
            points.new_empty((P,), dtype=torch.uint8), points.new_empty((P, 3), dtype=f),
            points.new_empty((P if normals is not None else 0, 3), dtype=f))


# --------------------------------------------------------------------------------------------- depth preparation
@_op("prepare_depth", mutates_args=())
def prepare_depth(depth: Tensor, intr: List[float], radius: int, sigma_s: float, sigma_r: float, range_cut: float,
                  edge_max: float, normalizer: float, with_normals: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """ofx_prepare_depth (new capability, no reference twin): the bilateral-filtered depth of a frame, its vertex map and
    its normal map. depth (H,W): f32 metres or 16-bit integers (read as uint16, scaled by 1/normalizer); never written.
    -> depth f32 (H,W), point_image f32 (3,H,W), normals f32 (3,H,W) — the gate's target normal of point_image at every
    pixel under edge_max, zeros where it has none; with_normals=False skips the normal map and returns an empty (0,H,W)
    tensor in its place. radius 0..4 (0: no filtering), sigma_s in pixels, sigma_r and range_cut in metres."""
    if depth.dim() != 2:
        raise ValueError(f"prepare_depth: depth must be (H, W), got {tuple(depth.shape)}")
    is_u16 = depth.dtype != torch.float32
    if is_u16 and depth.dtype not in (torch.uint16, torch.int16):
        raise ValueError(f"prepare_depth: depth must be float32 or 16-bit integer, got {depth.dtype}")
    H, W = depth.shape
    d = depth.contiguous()
    cam = _camera(intr, H, W)
    prm = _lib.PrepareParams(int(radius), float(sigma_s), float(sigma_r), float(range_cut), float(edge_max),
                             float(normalizer))
    out = torch.empty((H, W), dtype=torch.float32, device=d.device)
    pimg = torch.empty((3, H, W), dtype=torch.float32, device=d.device)
    nimg = torch.empty((3 if with_normals else 0, H, W), dtype=torch.float32, device=d.device)
    call("ofx_prepare_depth", ptr(d), 1 if is_u16 else 0, H, W, byref(cam), byref(prm), ptr(out), ptr(pimg),
         ptr(nimg) if with_normals else None, _stream(d))
    return out, pimg, nimg


@prepare_depth.register_fake
def _(depth, intr, radius, sigma_s, sigma_r, range_cut, edge_max, normalizer, with_normals):
    H, W = depth.shape
    f = torch.float32
    return (depth.new_empty((H, W), dtype=f), depth.new_empty((3, H, W), dtype=f),
            depth.new_empty((3 if with_normals else 0, H, W), dtype=f))


# --------------------------------------------------------------------------------------------- surface points
@_op("surface_points", mutates_args=("state", "points", "normals", "anchors_out", "weights_out", "voxel", "valid", "code",
                                     "count"))
def surface_points(state: Tensor, handle: int, tsdf: Tensor, weight: Tensor, brick_list: Tensor, n_list: int,
                   skin_anchors: Tensor, skin_weights: Tensor, k: int, dims: List[int], origin: List[float],
                   voxel_size: float, trunc_margin: float, w_min: float, points: Tensor, normals: Tensor,
                   anchors_out: Tensor, weights_out: Tensor, voxel: Tensor, valid: Tensor, code: Optional[Tensor],
                   count: Tensor) -> None:
    """ofx_surface_points (new capability, no reference twin): the skinned surface points of a whole bricked volume
    (tsdf / weight) read through its skin cache (brick_list, n_list, skin_anchors u16 in int16 storage, skin_weights,
    k = 4), written into the caller's max_points-row outputs: points / normals f32 (M,3), anchors_out i32 (M,4),
    weights_out f32 (M,4), voxel i32 (M,), valid u8 (M,), code u8 (n_list*512,) or None, count i32 (2,) = [accepted,
    emitted] on the device. Rows past `emitted` are defined padding (valid 0, voxel -1, zeros). `handle` is an
    ofx_surface_create handle sized for at least n_list bricks; `state` is its ordering token."""
    M = points.shape[0]
    nbx = (int(dims[0]) + 7) // 8
    desc = _volume_desc(dims, [0, nbx], origin, voxel_size, trunc_margin, 0)
    if code is not None and code.shape[0] < int(n_list) * 512:
        raise ValueError(f"surface_points: code holds {code.shape[0]} entries, {int(n_list) * 512} are needed")
    for name, t, rows in (("normals", normals, 3), ("anchors_out", anchors_out, 4), ("weights_out", weights_out, 4)):
        if t.shape[0] != M or t.shape[1] != rows:
            raise ValueError(f"surface_points: {name} must be ({M}, {rows}), got {tuple(t.shape)}")
    if voxel.shape[0] != M or valid.shape[0] != M or count.shape[0] != 2:
        raise ValueError("surface_points: voxel / valid must have max_points rows and count two entries")
    call("ofx_surface_points", _lib.c_void_p(handle), byref(desc), ptr(tsdf), ptr(weight), ptr(brick_list), int(n_list),
         ptr(skin_anchors), ptr(skin_weights), int(k), float(w_min), M, ptr(points), ptr(normals), ptr(anchors_out),
         ptr(weights_out), ptr(voxel), ptr(valid), ptr(code), ptr(count), _stream(tsdf))


@surface_points.register_fake
def _(state, handle, tsdf, weight, brick_list, n_list, skin_anchors, skin_weights, k, dims, origin, voxel_size,
      trunc_margin, w_min, points, normals, anchors_out, weights_out, voxel, valid, code, count):
    return None


def surface_outputs(max_points, device, n_list=None):
    """Output tensors of torch.ops.ofx.surface_points for max_points rows (code for n_list bricks, None without):
    (points, normals, anchors, weights, voxel, valid, code, count)."""
    M = int(max_points)
    f, i = torch.float32, torch.int32
    return (torch.empty((M, 3), dtype=f, device=device), torch.empty((M, 3), dtype=f, device=device),
            torch.empty((M, 4), dtype=i, device=device), torch.empty((M, 4), dtype=f, device=device),
            torch.empty(M, dtype=i, device=device), torch.empty(M, dtype=torch.uint8, device=device),
            None if n_list is None else torch.empty(max(1, int(n_list)) * 512, dtype=torch.uint8, device=device),
            torch.empty(2, dtype=i, device=device))


# --------------------------------------------------------------------------------------------- graph growth
@_op("grow_nodes", mutates_args=("state", "nodes", "rotations", "translations", "edges", "edge_weights", "count"))
def grow_nodes(state: Tensor, handle: int, points: Tensor, anchors: Tensor, weights: Tensor, valid: Tensor,
               nodes: Tensor, n_nodes: int, rotations: Tensor, translations: Tensor, edges: Tensor,
               edge_weights: Tensor, node_coverage: float, min_dist: float, spacing: float, max_new: int,
               count: Tensor) -> None:
    """ofx_grow_nodes (new capability; the reference's twin is the host loop of EDGraph.update): new graph nodes at the
    model rows (points (M,3), anchors i32 (M,4), weights (M,4), valid u8 (M,), as surface_points writes them) that lie
    more than min_dist from every node, greedily `spacing` apart in row order, at most max_new. The caller's arrays hold
    n_nodes rows followed by room for max_new more — nodes (.,3), rotations (.,9) or (.,3,3), translations (.,3), edges
    i32 (.,K_e), edge_weights (.,K_e) — and receive the new rows: position, the translation the point's own skin gives
    it, the quaternion blend of its anchors' rotations, the K_e nearest other nodes and their weights. count i32 (3,) on
    the device = [candidates, selected, 1 if the cap cut the selection short]. `handle` is an ofx_grow_create handle
    sized for at least M rows and max_new nodes; `state` is its ordering token."""
    M, rows = points.shape[0], int(n_nodes) + int(max_new)
    for name, t, cols in (("anchors", anchors, 4), ("weights", weights, 4)):
        if t.shape[0] != M or t.shape[1] != cols:
            raise ValueError(f"grow_nodes: {name} must be ({M}, {cols}), got {tuple(t.shape)}")
    if valid.shape[0] != M or count.shape[0] != 3:
        raise ValueError("grow_nodes: valid must have one entry per row and count three entries")
    if edges.dim() != 2 or edge_weights.shape != edges.shape:
        raise ValueError("grow_nodes: edges and edge_weights must be (rows, K_e)")
    for name, t, per in (("nodes", nodes, 3), ("rotations", rotations, 9), ("translations", translations, 3),
                         ("edges", edges, edges.shape[1]), ("edge_weights", edge_weights, edges.shape[1])):
        if t.numel() < rows * per or not t.is_contiguous():
            raise ValueError(f"grow_nodes: {name} must be contiguous with room for n_nodes + max_new = {rows} rows")
    call("ofx_grow_nodes", _lib.c_void_p(handle), ptr(points), ptr(anchors), ptr(weights), ptr(valid), M, ptr(nodes),
         int(n_nodes), ptr(rotations), ptr(translations), ptr(edges), ptr(edge_weights), int(edges.shape[1]),
         float(node_coverage), float(min_dist), float(spacing), int(max_new), ptr(count), _stream(points))


@grow_nodes.register_fake
def _(state, handle, points, anchors, weights, valid, nodes, n_nodes, rotations, translations, edges, edge_weights,
      node_coverage, min_dist, spacing, max_new, count):
    return None


# --------------------------------------------------------------------------------------------- dense SPD solve
@_op("spd_solve", mutates_args=())
def spd_solve(A: Tensor, b: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """ofx_spd_solve on copies: A (n,n) f64 symmetric positive definite (only its lower triangle is read; a row stride
    >= n is passed on as lda), b (n) f64 -> (L (n,n): the Cholesky factor in the lower triangle, the strict upper triangle
    as given; x (n) = A⁻¹b; status int32[2] = [not positive definite / non-finite pivot, index of the first bad pivot],
    x = 0 then)."""
    if A.dim() != 2 or A.shape[0] != A.shape[1] or b.dim() != 1 or b.shape[0] != A.shape[0]:
        raise ValueError(f"spd_solve: A must be (n, n) and b (n); got {tuple(A.shape)}, {tuple(b.shape)}")
    if A.dtype != torch.float64 or b.dtype != torch.float64:
        raise ValueError("spd_solve: A and b must be float64")
    n = A.shape[0]
    lda = max(A.stride(0) if ((A.stride(1) == 1 or n == 1) and A.stride(0) >= n) else n, 1)
    buf = torch.empty((n, lda), dtype=torch.float64, device=A.device)
    L = buf[:, :n]
    L.copy_(A)
    x = b.clone().contiguous()
    status = torch.empty(2, dtype=torch.int32, device=A.device)
    call("ofx_spd_solve", ptr(buf), n, lda, ptr(x), ptr(status), _stream(A))
    return L.contiguous(), x, status


@spd_solve.register_fake
def _(A, b):
    n = A.shape[0]
    return (A.new_empty((n, n)), b.new_empty((n,)), A.new_empty((2,), dtype=torch.int32))


# --------------------------------------------------------------------------------------------- Gauss-Newton
def _gn_problem(nodes, edges, edge_weights, tpos, conf, src, anchors, weights, tgt, target_px, target_py, prev_rot,
                prev_trans, intr):
    pb = _lib.GnProblem()
    pb.n_nodes, pb.n_matches, pb.n_neighbors = nodes.shape[0], src.shape[0], edges.shape[1]
    pb.nodes, pb.edges, pb.edge_weights = ptr(nodes), ptr(edges), ptr(edge_weights)
    pb.target_node_pos, pb.node_conf = ptr(tpos), ptr(conf)
    pb.src, pb.anchors, pb.weights, pb.tgt = ptr(src), ptr(anchors), ptr(weights), ptr(tgt)
    pb.target_px, pb.target_py = ptr(target_px), ptr(target_py)
    pb.prev_rot, pb.prev_trans = ptr(prev_rot), ptr(prev_trans)
    pb.fx, pb.fy, pb.cx, pb.cy = (float(v) for v in intr[:4])
    return pb


def _gn_params(fparams, iparams):
    """fparams = [lambda_flow, lambda_depth, lambda_arap, lambda_motion, lm_factor, stop_loss_diff, pcg_tol,
    pcg_err_tol, precond_rot_tol]; iparams = [num_iter, use_edge_weighting, pcg_max_iter, pcg_warm, mode,
    precond_every(, precond: OFX_PRECOND_CLUSTER 0 / OFX_PRECOND_SCHWARZ 1 / OFX_PRECOND_AUTO 2 / OFX_PRECOND_DIRECT 3,
    default 0)]."""
    p = _lib.GnParams()
    (p.lambda_flow, p.lambda_depth, p.lambda_arap, p.lambda_motion, p.lm_factor, p.stop_loss_diff,
     p.pcg_tol, p.pcg_err_tol, p.precond_rot_tol) = (float(v) for v in fparams)
    p.num_iter, p.use_edge_weighting, p.pcg_max_iter, p.pcg_warm, p.mode, p.precond_every = (int(v) for v in iparams[:6])
    p.precond = int(iparams[6]) if len(iparams) > 6 else 0
    return p


def _gn_outputs(N, num_iter, device):
    # k_finish writes every element (status and all num_iter loss rows): no fill kernels
    return (torch.empty((N, 3, 3), device=device), torch.empty((N, 3), device=device),
            torch.empty(5, dtype=torch.int32, device=device),
            torch.empty((num_iter, 4), dtype=torch.float64, device=device))


def _gn_result(out):
    r = _lib.GnResult()
    r.rot, r.trans, r.status, r.loss_log = (ptr(t) for t in out)
    return r


@_op("gn_solve", mutates_args=("state",))
def gn_solve(state: Tensor, handle: int, nodes: Tensor, edges: Tensor, edge_weights: Tensor, tpos: Tensor,
             conf: Tensor, src: Tensor, anchors: Tensor, weights: Tensor, tgt: Tensor, target_px: Optional[Tensor],
             target_py: Optional[Tensor], prev_rot: Optional[Tensor], prev_trans: Optional[Tensor],
             intr: List[float], fparams: List[float], iparams: List[int]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """DeformNet.optimize (model/model.py:222-859) for one batch item on the device: -> (node_rotations (N,3,3),
    node_translations (N,3), status int32[5] = [valid, GN steps, PCG iterations, ill-posed, GN steps whose PCG hit
    pcg_max_iter], loss f64[num_iter,4])."""
    pb = _gn_problem(nodes, edges, edge_weights, tpos, conf, src, anchors, weights, tgt, target_px, target_py,
                     prev_rot, prev_trans, intr)
    prm = _gn_params(fparams, iparams)
    out = _gn_outputs(nodes.shape[0], int(iparams[0]), nodes.device)
    call("ofx_gn_solve", _lib.c_void_p(handle), byref(pb), byref(prm), byref(_gn_result(out)), _stream(nodes))
    return out


@gn_solve.register_fake
def _(state, handle, nodes, edges, edge_weights, tpos, conf, src, anchors, weights, tgt, target_px, target_py,
      prev_rot, prev_trans, intr, fparams, iparams):
    N = nodes.shape[0]
    return (nodes.new_empty((N, 3, 3)), nodes.new_empty((N, 3)), nodes.new_empty((5,), dtype=torch.int32),
            nodes.new_empty((int(iparams[0]), 4), dtype=torch.float64))


@_op("gn_prepare", mutates_args=("state",))
def gn_prepare(state: Tensor, handle: int, nodes: Tensor, edges: Tensor, edge_weights: Tensor, tpos: Tensor,
               conf: Tensor, src: Tensor, anchors: Tensor, weights: Tensor, tgt: Tensor, target_px: Optional[Tensor],
               target_py: Optional[Tensor], intr: List[float], fparams: List[float], iparams: List[int],
               trigger: int = 0, trigger_step: int = 0) -> None:
    """ofx_gn_prepare: prefetch the setup of the next gn_solve on this handle (host thread + the handle's own
    stream, ordered after the current stream's work); returns at once. The tensors must stay alive and
    unchanged until that solve. trigger != 0 (ofx_gn_prepare_after): the setup starts when the next gn_solve on
    handle `trigger` reaches GN step trigger_step (or returns)."""
    pb = _gn_problem(nodes, edges, edge_weights, tpos, conf, src, anchors, weights, tgt, target_px, target_py,
                     None, None, intr)
    prm = _gn_params(fparams, iparams)
    if trigger:
        call("ofx_gn_prepare_after", _lib.c_void_p(handle), byref(pb), byref(prm), _stream(nodes),
             _lib.c_void_p(trigger), int(trigger_step))
    else:
        call("ofx_gn_prepare", _lib.c_void_p(handle), byref(pb), byref(prm), _stream(nodes))


@gn_prepare.register_fake
def _(state, handle, nodes, *rest):
    return None


@_op("gn_setup", mutates_args=("state",))
def gn_setup(state: Tensor, handle: int, nodes: Tensor, edges: Tensor, edge_weights: Tensor, tpos: Tensor,
             conf: Tensor, src: Tensor, anchors: Tensor, weights: Tensor, tgt: Tensor, target_px: Optional[Tensor],
             target_py: Optional[Tensor], prev_rot: Optional[Tensor], prev_trans: Optional[Tensor],
             intr: List[float], fparams: List[float], iparams: List[int]) -> Tensor:
    """ofx_gn_setup: upload the problem and build the JᵀJ block pattern -> int64[2] (host) = [JᵀJ blocks, PCG
    rows] (one stream sync, as the C call)."""
    pb = _gn_problem(nodes, edges, edge_weights, tpos, conf, src, anchors, weights, tgt, target_px, target_py,
                     prev_rot, prev_trans, intr)
    prm = _gn_params(fparams, iparams)
    nnz = _lib.c_int64()
    h = _lib.c_void_p(handle)
    call("ofx_gn_setup", h, byref(pb), byref(prm), byref(nnz), _stream(nodes))
    info = (_lib.c_int64 * 5)()
    call("ofx_gn_info", h, info)
    return torch.tensor([nnz.value, info[4]], dtype=torch.int64)


@gn_setup.register_fake
def _(state, handle, nodes, *rest):
    return torch.empty(2, dtype=torch.int64, device="cpu")


@_op("gn_linearize", mutates_args=("state", "A", "rhs"))
def gn_linearize(state: Tensor, handle: int, it: int, m0: int, m1: int, regularizers: bool, A: Tensor,
                 rhs: Tensor) -> None:
    """One GN step's JᵀJ (BSR 6x6 f64 blocks, A) and -Jᵀr (rhs, + loss² tail) over matches [m0, m1), plus the
    ARAP / motion rows and the LM damping when `regularizers` (model.py:415-662)."""
    call("ofx_gn_linearize", _lib.c_void_p(handle), int(it), int(m0), int(m1), 1 if regularizers else 0, ptr(A),
         ptr(rhs), _stream(A))


@gn_linearize.register_fake
def _(state, handle, it, m0, m1, regularizers, A, rhs):
    return None


@_op("gn_step", mutates_args=("state",))
def gn_step(state: Tensor, handle: int, it: int, A: Tensor, rhs: Tensor) -> None:
    """Solve A x = rhs (PCG) and take the GN step (loss rule, kornia exp map, R ← exp(x)·R, t += x; model.py:
    694-748)."""
    call("ofx_gn_step", _lib.c_void_p(handle), int(it), ptr(A), ptr(rhs), _stream(A))


@gn_step.register_fake
def _(state, handle, it, A, rhs):
    return None


@_op("gn_finish", mutates_args=("state",))
def gn_finish(state: Tensor, handle: int, n_nodes: int, num_iter: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Results of the stepped solve (ofx_gn_finish): as gn_solve's outputs."""
    out = _gn_outputs(n_nodes, num_iter, state.device)
    call("ofx_gn_finish", _lib.c_void_p(handle), byref(_gn_result(out)), _stream(state))
    return out


@gn_finish.register_fake
def _(state, handle, n_nodes, num_iter):
    return (state.new_empty((n_nodes, 3, 3), dtype=torch.float32), state.new_empty((n_nodes, 3), dtype=torch.float32),
            state.new_empty((5,), dtype=torch.int32), state.new_empty((num_iter, 4), dtype=torch.float64))


@_op("gn_set_robust", mutates_args=("state",))
def gn_set_robust(state: Tensor, handle: int, match_weights: Optional[Tensor], kernel: int, scale: float) -> None:
    """ofx_gn_set_robust: per-match weights (f32 (M), or None = all 1) and a robust kernel (0 none / 1 Huber / 2 Tukey,
    scale in metres) on the data rows of the following solves on this handle, until replaced; no weights and kernel 0
    switch it off. The next gn_solve / gn_setup / gn_prepare on the handle copies the weights in its stream order:
    match_weights must stay alive and unchanged until that call has been enqueued. No device work here."""
    rb = _lib.GnRobust()
    rb.match_weights, rb.kernel, rb.scale = ptr(match_weights), int(kernel), float(scale)
    call("ofx_gn_set_robust", _lib.c_void_p(handle), byref(rb))


@gn_set_robust.register_fake
def _(state, handle, match_weights, kernel, scale):
    return None


# --------------------------------------------------------------------------------------------- motion completion
def _motion_rows(name, t, shape, dtype):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} "
                         f"{tuple(t.shape)}")


@_op("motion_forward", mutates_args=("state",))
def motion_forward(state: Tensor, handle: int, pos: Tensor, curr_motion: Tensor, hist: Tensor) -> Tensor:
    """ofx_motion_forward (motion_model.py:52-98, inference): the motion completion network on the graph the handle holds
    (ofx_motion_set_graph). pos f32 (N,3) centred node positions, curr_motion f32 (N,4) [normalised motion | visible],
    hist f32 (T,N,4), 1 <= T <= 16 -> f32 (N,4) = (mu, sigma). `handle` is an ofx_motion_create handle; `state` is its
    ordering token (its scratch is hidden state)."""
    N, T = pos.shape[0], hist.shape[0]
    _motion_rows("motion_forward: pos", pos, (N, 3), torch.float32)
    _motion_rows("motion_forward: curr_motion", curr_motion, (N, 4), torch.float32)
    _motion_rows("motion_forward: hist", hist, (T, N, 4), torch.float32)
    out = torch.empty((N, 4), dtype=torch.float32, device=pos.device)
    call("ofx_motion_forward", _lib.c_void_p(handle), ptr(pos), ptr(curr_motion), ptr(hist), T, N, ptr(out), _stream(pos))
    return out


@motion_forward.register_fake
def _(state, handle, pos, curr_motion, hist):
    return pos.new_empty((pos.shape[0], 4), dtype=torch.float32)


@_op("motion_complete", mutates_args=("state",))
def motion_complete(state: Tensor, handle: int, src: Tensor, dst: Tensor, visible: Tensor, conf_scale: float,
                    max_hist: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """ofx_motion_complete (run_motion_model.py:45-196): one frame of the motion completion runner. src / dst f64 (N,3)
    node positions at the source frame and at the tracked estimate, visible bool / u8 (N); conf_scale: 2 in the fusion
    runner, 4 in demo.py; max_hist: the handle's (it sizes the history output). -> node_motion f64 (N,3), confidence f64
    (N), status i32 (1) (bit 0: degenerate fit, outputs 0; bit 1: degenerate previous-frame fit), and the network's
    inputs and raw output as used: pos f32 (N,3), curr_motion f32 (N,4), hist f32 (max_hist,N,4) of which the first
    min(calls since reset, max_hist) rows are written (the rest 0), raw f32 (N,4). The history, the last src / visible
    and the std live on the handle: `state` is its ordering token."""
    N, dev = src.shape[0], src.device
    _motion_rows("motion_complete: src", src, (N, 3), torch.float64)
    _motion_rows("motion_complete: dst", dst, (N, 3), torch.float64)
    if visible.dtype not in (torch.bool, torch.uint8) or tuple(visible.shape) != (N,):
        raise ValueError(f"motion_complete: visible must be bool or uint8 of shape ({N},)")
    info = (_lib.c_int64 * 10)()
    call("ofx_motion_info", _lib.c_void_p(handle), info)
    if int(max_hist) != info[8]:
        raise ValueError(f"motion_complete: max_hist {max_hist} is not the handle's {info[8]}")
    vis = visible.to(torch.uint8).contiguous()
    node_motion = torch.empty((N, 3), dtype=torch.float64, device=dev)
    conf = torch.empty((N,), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    pos = torch.empty((N, 3), dtype=torch.float32, device=dev)
    cm = torch.empty((N, 4), dtype=torch.float32, device=dev)
    hist = torch.zeros((int(max_hist), N, 4), dtype=torch.float32, device=dev)
    raw = torch.empty((N, 4), dtype=torch.float32, device=dev)
    call("ofx_motion_complete", _lib.c_void_p(handle), ptr(src), ptr(dst), ptr(vis), N, float(conf_scale),
         ptr(node_motion), ptr(conf), ptr(status), ptr(pos), ptr(cm), ptr(hist), ptr(raw), _stream(src))
    return node_motion, conf, status, pos, cm, hist, raw


@motion_complete.register_fake
def _(state, handle, src, dst, visible, conf_scale, max_hist):
    N = src.shape[0]
    e = src.new_empty
    return (e((N, 3), dtype=torch.float64), e((N,), dtype=torch.float64), e((1,), dtype=torch.int32),
            e((N, 3), dtype=torch.float32), e((N, 4), dtype=torch.float32),
            e((int(max_hist), N, 4), dtype=torch.float32), e((N, 4), dtype=torch.float32))


OPS = ("integrate","integrate_points", "raycast", "skin_points", "deform_points", "gn_solve", "gn_prepare", "gn_setup",
       "gn_linearize", "gn_step", "gn_finish", "spd_solve", "associate", "surface_points",
       "rigid_icp", "splat_points", "prepare_depth", "grow_nodes", "photo_associate", "gn_set_robust",
       "integrate_weighted", "integrate_points_weighted", "observation_weights", "motion_forward", "motion_complete", "photo_refine")
