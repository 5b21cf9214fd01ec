"""Projective data association: the matches of a depth frame, found by the library itself.

Every solve here takes correspondences as an input; in the reference they come from learned front-ends (Lepard, the flow
net). ProjectiveAssociator produces them from geometry alone, the way a TSDF fusion system tracks: warp the model points
with the current estimate, look them up in the target depth frame's vertex map, gate by distance, depth edges and
normals, and hand the surviving pairs to GaussNewtonSolver.optimize (torch.ops.ofx.associate -> ofx_associate, one gather
kernel + an ordered compaction). It has no reference twin; its geometric relative there is the truncated chamfer term
(NonRigidICP/model/loss.py:275-292). icp_track is the loop around it that Registration.track and
FusionPipeline.track_step share; RigidAligner (torch.ops.ofx.rigid_icp -> ofx_rigid_icp) is its optional first stage, a
rigid point-to-plane ICP of all model points whose pose fold_rigid folds into the node transforms. This is the data term for what the camera sees: motion of occluded nodes still needs the
motion-completion input. ModelRenderer (torch.ops.ofx.splat_points -> ofx_splat_points) is the model's own z-buffer in the
live frame: with occlusion=True, icp_track keeps the points that the model itself hides out of both stages, and
WarpField.render_live shows the fused model where the camera is. ProjectiveAssociator.associate_photo
(torch.ops.ofx.photo_associate -> ofx_photo_associate) is the search by colour — the stand-in for the reference's flow
net: with photo=True, icp_track matches every point to the best colour match in a window around its pixel, which follows
motion along a surface that depth alone cannot see. ProjectiveAssociator.refine_photo (torch.ops.ofx.photo_refine ->
ofx_photo_refine) makes those whole-pixel matches sub-pixel: with photo_refine=True and a template, icp_track aligns a
small colour patch of the template around each match and takes the vertex map at the refined pixel as the target.
"""
import numpy as np
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.ofx.*)
from ._lib import byref, call

MODES = {"point": 0, "plane": 1}
CODE_NAMES = ("accepted", "invalid_skin", "off_image", "hole", "no_normal", "too_far", "normal_mismatch")
PHOTO_CODE_NAMES = CODE_NAMES + ("colour",)   # associate_photo's codes: associate's, and 7
ASSOC_DEFAULTS = dict(dist_max=0.05, cos_min=0.5, edge_max=0.03, mode="plane", max_matches=10000)
PHOTO_DEFAULTS = dict(radius=4, color_max=float("inf"), geo_weight=1.0)
REFINE_DEFAULTS = dict(half=3, iters=8, eps=1e-3, max_shift=4.0, min_eig=1e-6, ssd_max=float("inf"))
REFINE_CODE_NAMES = ("refined", "no_match", "template_off", "flat", "left_image", "too_far", "residual", "depth_edge")


class TooFewMatches(RuntimeError):
    """An association emitted fewer matches than a solve needs (4·K = 16): nothing was solved."""


def _f32(x, device, shape=None):
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    return t if shape is None else t.reshape(shape)


def pack_transforms(nodes, rot, trans, device):
    """(N,16) packed node records (ofx_pack_nodes) of node positions (N,3), rotations (N,3,3) or None (identity) and
    node-relative translations (N,3) or None (zero)."""
    g = _f32(nodes, device, (-1, 3))
    N = g.shape[0]
    R = _f32(rot, device, (N, 9)) if rot is not None else torch.eye(3, device=device).reshape(1, 9).repeat(N, 1)
    T = _f32(trans, device, (N, 3)) if trans is not None else torch.zeros((N, 3), device=device)
    out = torch.empty((N, 16), dtype=torch.float32, device=device)
    call("ofx_pack_nodes", _lib.ptr(R), _lib.ptr(T), _lib.ptr(g), N, _lib.ptr(out),
         _lib.stream_ptr(torch.cuda.current_stream(device)))
    return out


def _skinned(points, normals, anchors, weights, valid, warpfield_or_packed_nodes, device, capacity, what):
    """The skinned inputs every entry point takes, as the operators want them -> (pts (P,3), nrm (P,3) or None, anchors
    i32 (P,4), weights (P,4), valid u8 (P,) or None, packed (N,16), P). `what` names the owner of `capacity`."""
    d = device
    pts = _f32(points, d, (-1, 3))
    P = pts.shape[0]
    if P > capacity:
        raise ValueError(f"{P} points exceed the {what}'s capacity ({capacity})")
    packed = (warpfield_or_packed_nodes.packed_nodes() if hasattr(warpfield_or_packed_nodes, "packed_nodes")
              else _f32(warpfield_or_packed_nodes, d, (-1, 16)))
    a = anchors if isinstance(anchors, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(anchors))
    a = a.to(device=d, dtype=torch.int32).contiguous().reshape(P, 4)
    v = None
    if valid is not None:
        v = valid if isinstance(valid, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(valid))
        v = v.to(device=d).to(torch.uint8).contiguous().reshape(P)
    return pts, _f32(normals, d, (P, 3)), a, _f32(weights, d, (P, 4)), v, packed, P


class _Handle:
    """A device, a C handle made by `create`(*args, &handle) on it and freed by `destroy`, and the operator's ordering
    token."""
    _create = _destroy = None

    def _open(self, device, *args):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            call(self._create, *args, byref(self._h))
        self._state = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                getattr(_lib.lib, self._destroy)(h)
            except Exception:
                pass
        self._h = None


class ProjectiveAssociator(_Handle):
    """Owns an ofx_assoc handle (rank and tile scratch for up to max_points points) and the last call's outputs."""

    _create, _destroy = "ofx_assoc_create", "ofx_assoc_destroy"

    def __init__(self, max_points, device=None):
        self.max_points = int(max_points)
        self._open(device, self.max_points)
        self.last = None

    def associate(self, points, normals, anchors, weights, valid, warpfield_or_packed_nodes, point_image, intr,
                  dist_max=0.05, cos_min=0.5, edge_max=0.03, mode="plane", max_matches=10000):
        """Associate points (P,3) — skinned with anchors i32 (P,4) / weights (P,4), valid (P,) or None, unit normals
        (P,3) or None — with the target vertex map point_image (3,H,W) (backproject_depth_device) under the transforms
        of a WarpField or of a packed (N,16) node tensor (WarpField.packed_nodes / pack_transforms). intr: (fx, fy, cx,
        cy). Gates: dist_max and edge_max in metres, cos_min on the warped normal against the target's; mode "plane"
        targets the foot of the warped point on the target's tangent plane, "point" the vertex itself.

        Returns a dict: the compacted matches sliced to the emitted count — match_idx (point indices, ascending),
        src, tgt, anchors, weights — the per-point code (0 accepted, 1..6 the first gate that rejected the point;
        CODE_NAMES), tgt_all, warped, and accepted / emitted / histogram (counts per code).

        Reading the counts is the tracking loop's one host synchronisation per association; everything else is
        enqueued on torch's current stream."""
        d = self.device
        pts, nrm, a, w, v, packed, P = _skinned(points, normals, anchors, weights, valid, warpfield_or_packed_nodes, d,
                                                self.max_points, "associator")
        vm = _f32(point_image, d)
        assert vm.dim() == 3 and vm.shape[0] == 3, "point image must be (3, H, W)"
        out = torch.ops.ofx.associate(self._state, self._h.value, pts, nrm, a, w, v, packed, vm,
                                      [float(x) for x in intr[:4]], float(dist_max), float(cos_min), float(edge_max),
                                      MODES[mode], int(max_matches))
        code, tgt_all, warped, midx, src, tgt, a_o, w_o, count = out
        hist = torch.bincount(code.to(torch.int64), minlength=len(CODE_NAMES))
        host = torch.cat([count.to(torch.int64), hist]).cpu().tolist()   # the one host sync
        n_acc, n_emit = int(host[0]), int(host[1])
        self.last = {"match_idx": midx[:n_emit], "src": src[:n_emit], "tgt": tgt[:n_emit], "anchors": a_o[:n_emit],
                     "weights": w_o[:n_emit], "code": code, "tgt_all": tgt_all, "warped": warped, "accepted": n_acc,
                     "emitted": n_emit, "histogram": [int(x) for x in host[2:2 + len(CODE_NAMES)]]}
        return self.last


    def associate_photo(self, points, normals, colors, anchors, weights, valid, warpfield_or_packed_nodes, point_image,
                        normal_image, color_image, intr, dist_max=0.05, cos_min=0.5, color_max=float("inf"),
                        geo_weight=1.0, radius=4, max_matches=10000):
        """Photometric correspondence search (torch.ops.ofx.photo_associate -> ofx_photo_associate): inputs as
        `associate`, plus the points' colours (P,3) rgb in [0,1], the frame's normal map normal_image (3,H,W)
        (prepare_depth_device of the same frame: zeros where the gate has no normal) and its colour image color_image
        (3,H,W) rgb in [0,1]. Every point searches the (2·radius + 1)² window around its pixel (radius 0..8) for the
        pixel that passes associate's gates (dist_max, cos_min; a colour farther than color_max is refused too) with the
        smallest cost |Δcolour|² + geo_weight·|q − x'|²; that pixel's vertex is the target.

        Returns associate's dict (code 7 = "colour": PHOTO_CODE_NAMES; the histogram has one more entry), plus pixel
        (emitted rows, f32 (u, v) of the match: what the solver's target_px / target_py take), pixel_all i32 (P,2) and
        cost (P,) and count (the device int32[2] = [accepted, emitted]). The same single host read."""
        d = self.device
        pts, nrm, a, w, v, packed, P = _skinned(points, normals, anchors, weights, valid, warpfield_or_packed_nodes, d,
                                                self.max_points, "associator")
        col = _f32(colors, d, (P, 3))
        vm, nm, cm = _f32(point_image, d), _f32(normal_image, d), _f32(color_image, d)
        assert vm.dim() == 3 and vm.shape[0] == 3, "point image must be (3, H, W)"
        assert nm.shape == vm.shape and cm.shape == vm.shape, "normal and colour image must match the point image"
        out = torch.ops.ofx.photo_associate(self._state, self._h.value, pts, nrm, col, a, w, v, packed, vm, nm, cm,
                                            [float(x) for x in intr[:4]], float(dist_max), float(cos_min),
                                            float(color_max), float(geo_weight), int(radius), int(max_matches))
        code, tgt_all, warped, pixel_all, cost, midx, src, tgt, a_o, w_o, px_o, count = out
        hist = torch.bincount(code.to(torch.int64), minlength=len(PHOTO_CODE_NAMES))
        host = torch.cat([count.to(torch.int64), hist]).cpu().tolist()   # the one host sync
        n_acc, n_emit = int(host[0]), int(host[1])
        self.last = {"match_idx": midx[:n_emit], "src": src[:n_emit], "tgt": tgt[:n_emit], "anchors": a_o[:n_emit],
                     "weights": w_o[:n_emit], "pixel": px_o[:n_emit], "code": code, "tgt_all": tgt_all,
                     "warped": warped, "pixel_all": pixel_all, "cost": cost, "count": count, "accepted": n_acc,
                     "emitted": n_emit,
                     "histogram": [int(x) for x in host[2:2 + len(PHOTO_CODE_NAMES)]]}
        return self.last


    def refine_photo(self, match, template_image, template_px, color_image, point_image, edge_max,
                     template_mask=None, **refine):
        """Sub-pixel refinement of associate_photo's emitted matches (torch.ops.ofx.photo_refine -> ofx_photo_refine):
        `match` is associate_photo's result; template_image (3,H,W) rgb is the frame the model's colours came from,
        template_px f32 (rows,2) the (x, y) place of each emitted row's point in it (sub-pixel), template_mask (H,W) an
        optional validity mask of its pixels; color_image / point_image are the live frame's, as given to
        associate_photo; edge_max is the association's depth-edge gate, applied at the refined pixel. **refine:
        REFINE_DEFAULTS' keys. The (2·half + 1)² patch around template_px is aligned with the live frame from the
        match's pixel by `iters` translation-only inverse compositional Lucas-Kanade steps; a row that cannot be refined
        keeps its whole-pixel match.

        Returns the match dict with tgt and pixel replaced, plus refine_status u8 (REFINE_CODE_NAMES) and refine_ssd
        (the mean squared colour residual at the refined pixel). All device tensors; nothing is read back."""
        prm = refine_params(refine or True)
        d = self.device
        n = int(match["emitted"])
        tim, cim, vm = _f32(template_image, d), _f32(color_image, d), _f32(point_image, d)
        tpx = _f32(template_px, d, (n, 2))
        ipx, tgt = match["pixel"].contiguous(), match["tgt"].contiguous()
        mask = None
        if template_mask is not None:
            mask = template_mask if isinstance(template_mask, torch.Tensor) else torch.as_tensor(
                np.ascontiguousarray(template_mask))
            mask = mask.to(device=d)
        count = match["count"]   # the search's device [accepted, emitted]: the rows are read from it on the device
        px_o, tgt_o = torch.empty_like(ipx), torch.empty_like(tgt)
        status = torch.empty(n, dtype=torch.uint8, device=d)
        ssd = torch.empty(n, dtype=torch.float32, device=d)
        torch.ops.ofx.photo_refine(tim, mask, cim, vm, tpx, ipx, tgt, count, int(prm["half"]), int(prm["iters"]),
                                   float(prm["eps"]), float(prm["max_shift"]), float(prm["min_eig"]),
                                   float(prm["ssd_max"]), float(edge_max), px_o, tgt_o, status, ssd)
        out = dict(match)
        out.update(tgt=tgt_o, pixel=px_o, refine_status=status, refine_ssd=ssd)
        return out


class RigidAligner(_Handle):
    """Owns an ofx_rigid handle (the workgroup records of the reduction for up to max_points points): the rigid,
    6-unknown point-to-plane ICP in front of the non-rigid solve (torch.ops.ofx.rigid_icp -> ofx_rigid_icp)."""

    _create, _destroy = "ofx_rigid_create", "ofx_rigid_destroy"

    def __init__(self, max_points, device=None):
        self.max_points = int(max_points)
        self._open(device, self.max_points)

    def align(self, points, normals, anchors, weights, valid, warpfield_or_packed_nodes, point_image, intr, pose=None,
              iters=4, dist_max=0.05, cos_min=0.5, edge_max=0.03, damping=1e-6, min_matches=6, stop_twist=0.0,
              sync=False):
        """iters point-to-plane iterations of all the points (inputs as ProjectiveAssociator.associate) from pose — a
        (3,4) [R|t], None = the identity; never modified — under the transforms of a WarpField or of a packed (N,16) node
        tensor. Returns dict(pose (3,4) f64 on the device, systems (iters,32) f64, code u8 (P,)); the layout of a systems
        row is ofx_rigid_icp's. Everything is enqueued on torch's current stream and nothing is read back, unless
        sync=True: then pose_host / systems_host (numpy) and the per-iteration lists accepted / rms (sqrt(Σr²/count),
        nan without matches) / status are added, at the cost of one host synchronisation."""
        d = self.device
        pts, nrm, a, w, v, packed, P = _skinned(points, normals, anchors, weights, valid, warpfield_or_packed_nodes, d,
                                                self.max_points, "aligner")
        vm = _f32(point_image, d)
        assert vm.dim() == 3 and vm.shape[0] == 3, "point image must be (3, H, W)"
        if pose is None:
            p = torch.eye(3, 4, dtype=torch.float64, device=d)
        else:
            p = pose if isinstance(pose, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(pose, np.float64))
            p = p.to(device=d, dtype=torch.float64).reshape(3, 4).clone().contiguous()
        code, systems = torch.ops.ofx.rigid_icp(self._state, self._h.value, pts, nrm, a, w, v, packed, vm,
                                                [float(x) for x in intr[:4]], float(dist_max), float(cos_min),
                                                float(edge_max), int(iters), int(min_matches), float(damping),
                                                float(stop_twist), p)
        out = {"pose": p, "systems": systems, "code": code}
        if sync:
            host = torch.cat([p.reshape(-1), systems.reshape(-1)]).cpu().numpy()   # the one host sync
            sys_h = host[12:].reshape(-1, 32)
            with np.errstate(divide="ignore", invalid="ignore"):
                rms = np.sqrt(sys_h[:, 27] / sys_h[:, 28])
            out.update(pose_host=host[:12].reshape(3, 4), systems_host=sys_h,
                       accepted=[int(x) for x in sys_h[:, 28]], rms=[float(x) for x in rms],
                       status=[int(x) for x in sys_h[:, 29]])
        return out


class ModelRenderer(_Handle):
    """Owns an ofx_splat handle (a u64 z-buffer of max_pixels words and per-point scratch for up to max_points points):
    the live-frame z-buffer of the warped model points (torch.ops.ofx.splat_points -> ofx_splat_points) — the depth,
    index and normal image of the model where the camera is, and for every point whether the model itself hides it."""

    _create, _destroy = "ofx_splat_create", "ofx_splat_destroy"

    def __init__(self, max_points, max_pixels, device=None):
        self.max_points, self.max_pixels = int(max_points), int(max_pixels)
        self._open(device, self.max_points, self.max_pixels)

    def render(self, points, normals, anchors, weights, valid, warpfield_or_packed_nodes, intr, height, width,
               splat_radius, occl_margin=0.01, normal_map=False):
        """Splat the points (inputs as ProjectiveAssociator.associate) under the transforms of a WarpField or of a
        packed (N,16) node tensor into a height x width image: every point a disc of world radius splat_radius (metres)
        on its tangent plane (facing the camera without normals), the nearest disc per pixel. Returns a dict of device
        tensors: depth f32 (H,W) (0 = nothing), index i32 (H,W) (-1 = nothing), code u8 (P,) (SPLAT_CODE_NAMES; 4 =
        occluded: more than occl_margin metres behind the buffer at the point's own pixel), warped (P,3), visible u8
        (P,) (code == 0) and, with normal_map=True (normals required), normals f32 (3,H,W): the warped normal of the
        point that owns each pixel, zeros where none does. Everything is enqueued on torch's current stream; nothing is
        read back."""
        d = self.device
        H, W = int(height), int(width)
        pts, nrm, a, w, v, packed, P = _skinned(points, normals, anchors, weights, valid, warpfield_or_packed_nodes, d,
                                                self.max_points, "renderer")
        if H * W > self.max_pixels:
            raise ValueError(f"{H} x {W} pixels exceed the renderer's capacity ({self.max_pixels})")
        if normal_map and normals is None:
            raise ValueError("normal_map=True needs the points' normals")
        depth, index, code, warped, wn = torch.ops.ofx.splat_points(
            self._state, self._h.value, pts, nrm, a, w, v, packed, [float(x) for x in intr[:4]], H, W,
            float(splat_radius), float(occl_margin))
        out = {"depth": depth, "index": index, "code": code, "warped": warped, "visible": (code == 0).to(torch.uint8)}
        if normal_map:
            hit = index >= 0
            if P:
                nm = wn[index.clamp(min=0).reshape(-1).long()].reshape(H, W, 3)
                nm = torch.where(hit[..., None], nm, torch.zeros((), dtype=torch.float32, device=d))
            else:
                nm = torch.zeros((H, W, 3), dtype=torch.float32, device=d)
            out["normals"] = nm.permute(2, 0, 1).contiguous()
        return out


SPLAT_CODE_NAMES = ("visible", "invalid_skin", "off_image", "back_facing", "occluded")


def default_splat_radius(voxel_size, with_normals):
    """The disc radius the tracking layers use for a model sampled from a volume: the voxel size when the model carries
    normals (tilted discs tile the surface without covering what lies behind its silhouette), half of it without
    (fronto-parallel discs of a full voxel hide too much of a slanted surface)."""
    return float(voxel_size) if with_normals else 0.5 * float(voxel_size)


def fold_rigid(nodes, rot, trans, pose):
    """Fold a rigid pose [R|t] (3,4) into the node transforms: R_k' = R·R_k, T_k' = R·(g_k + T_k) + t − g_k, computed in
    f64 on the pose's device and rounded once to f32; rot / trans None = the identity. The ED warp of any point then
    becomes R·warp(x) + S·t (S: the sum of its skin weights), so nothing downstream needs a notion of a camera pose.
    -> (rot' (N,3,3) f32, trans' (N,3) f32) device tensors. No host read."""
    p = pose if isinstance(pose, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(pose, np.float64))
    p = p.to(dtype=torch.float64).reshape(3, 4)
    d = p.device
    g = (nodes if isinstance(nodes, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(nodes)))
    g = g.to(device=d, dtype=torch.float64).reshape(-1, 3)
    N = g.shape[0]
    R, t = p[:, :3], p[:, 3]
    if rot is None:
        Rk = torch.eye(3, dtype=torch.float64, device=d).expand(N, 3, 3)
    else:
        Rk = (rot if isinstance(rot, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rot)))
        Rk = Rk.to(device=d, dtype=torch.float64).reshape(N, 3, 3)
    gt = g
    if trans is not None:
        Tk = (trans if isinstance(trans, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(trans)))
        gt = g + Tk.to(device=d, dtype=torch.float64).reshape(N, 3)
    # explicit sums (j ascending) rather than a BLAS call: the order is fixed
    Rn = (R[None, :, 0, None] * Rk[:, None, 0, :] + R[None, :, 1, None] * Rk[:, None, 1, :]) \
        + R[None, :, 2, None] * Rk[:, None, 2, :]
    Tn = (((R[None, :, 0] * gt[:, 0, None] + R[None, :, 1] * gt[:, 1, None]) + R[None, :, 2] * gt[:, 2, None])
          + t[None, :]) - g
    return Rn.to(torch.float32).contiguous(), Tn.to(torch.float32).contiguous()


def photo_params(photo):
    """The photo= keyword of the tracking layers as associate_photo's keywords: None / False -> None (off), True ->
    PHOTO_DEFAULTS, a dict of radius / color_max / geo_weight -> the defaults with those; another key is a TypeError."""
    if photo is None or photo is False:
        return None
    pho = dict(PHOTO_DEFAULTS)
    if photo is not True:
        unknown = set(photo) - set(pho)
        if unknown:
            raise TypeError(f"unknown photo parameters {sorted(unknown)}")
        pho.update(photo)
    return pho


def refine_params(refine):
    """The photo_refine= keyword of the tracking layers as refine_photo's keywords, with photo_params' conventions: None
    / False -> None (off), True -> REFINE_DEFAULTS, a dict of half / iters / eps / max_shift / min_eig / ssd_max -> the
    defaults with those; another key is a TypeError."""
    if refine is None or refine is False:
        return None
    prm = dict(REFINE_DEFAULTS)
    if refine is not True:
        unknown = set(refine) - set(prm)
        if unknown:
            raise TypeError(f"unknown photo_refine parameters {sorted(unknown)}")
        prm.update(refine)
    return prm


def icp_track(associator, solver, graph_nodes, graph_edges, graph_edges_weights, points, normals, anchors, weights,
              valid, depth, intr, prev_rot=None, prev_trans=None, complete_node_motion_data=None, icp_iters=3,
              rigid_iters=0, rigid=None, occlusion=False, renderer=None, splat_radius=None, occl_margin=0.01,
              depth_filter=None, photo=None, colors=None, color_image=None, robust=None, photo_refine=None,
              template=None, **assoc):
    """Track one depth frame without given matches: backproject depth (H,W) to the vertex map, then icp_iters times
    associate the points under the current estimate (prev_rot / prev_trans, None = identity) and solve on the emitted
    matches from that estimate (solver.optimize). Without motion data the nodes are their own targets with confidence
    0, so the motion rows vanish. An association that emits fewer than 4·K = 16 matches raises TooFewMatches before any
    solve. -> (the last optimize result, [per iteration dict(accepted, emitted, histogram)], vertex map).

    rigid_iters > 0 puts the rigid stage in front: before the first association, rigid_iters point-to-plane iterations
    of all the points (rigid: a RigidAligner, required then) from the identity pose around the current estimate, with
    the association's gates; the pose is folded into the estimate (fold_rigid) and the loop goes on from there. The
    stage reads nothing back: a failed rigid stage folds an unchanged pose. The result then gains "rigid": dict(pose,
    systems), device tensors.

    occlusion=True puts the model's own z-buffer in front of every stage (renderer: a ModelRenderer, and splat_radius,
    both required then): before the rigid stage and before every association the model is rendered under the current
    estimate (ModelRenderer.render with splat_radius / occl_margin) and valid & visible takes the place of valid for
    that stage, so a point that another part of the model hides is not matched to the surface in front of it. The mask
    stays on the device (no added host synchronisation), and the iteration's packed node tensor is built once for the
    render and the association. The result then gains "render": the last render's dict. occlusion=False is the loop
    as it was.

    depth_filter: None — the vertex map is backproject_depth_device of the raw depth, the loop as it was; True — the
    frame is prepared first (image_proc.prepare_depth_device with its defaults: the bilateral-filtered depth's vertex
    map); a dict overrides radius / sigma_s / sigma_r / range_cut (another key is a TypeError). The prepared vertex map
    is what the rigid stage and every association read and what is returned as the third value; the association's own
    edge_max keeps governing the gate, and the z-buffer stage does not read the frame.

    photo: None — the loop as it was; True, or a dict of radius / color_max / geo_weight (PHOTO_DEFAULTS; another key is
    a TypeError) — every iteration calls ProjectiveAssociator.associate_photo in place of associate: each point's target
    is the vertex of the best colour match in a window around its pixel, which also constrains motion along the surface
    that depth alone cannot see. It needs the model's colours `colors` (P,3) and the frame's colour image `color_image`
    (3,H,W), both rgb in [0,1] (a ValueError without them, before any device work). The frame's normal map comes from
    prepare_depth_device with the association's edge_max: radius 0 without depth_filter (its vertex map is then the raw
    one bit for bit), the filter's settings with it. `mode` is ignored under photo: the target is always the vertex.
    The rigid stage and the occlusion gate work as before.

    photo_refine: None — the loop as it was; True, or a dict of half / iters / eps / max_shift / min_eig / ssd_max
    (REFINE_DEFAULTS; another key is a TypeError) — every iteration refines the search's emitted matches before the solve
    (ProjectiveAssociator.refine_photo): the targets become sub-pixel. It needs photo and `template` = (image (3,H,W),
    px (P,2): the (x, y) place of every model point in that image, optional mask (H,W)) — the frame the model's colours
    came from (a ValueError without either, before any device work). The template pixel of emitted row i is
    px[match_idx[i]]; edge_max is the association's. No host read is added.

    robust: None — the loop as it was; "huber", "tukey" or a dict of kernel / scale (registration.ROBUST_DEFAULTS; another
    key is a TypeError, an unknown kernel a ValueError, before any device work) — forwarded to every solver.optimize of
    the loop: an M-estimator on the data rows, so a match just inside dist_max no longer pulls like a perfect one."""
    from .registration import robust_params
    robust_params(robust)
    rob = {} if robust is None else {"robust": robust}
    from .image_proc import PREPARE_DEFAULTS, backproject_depth_device, prepare_depth_device
    rigid_iters = int(rigid_iters)
    if rigid_iters < 0:
        raise ValueError("rigid_iters must not be negative")
    if int(icp_iters) < 1:
        raise ValueError("icp_iters must be at least 1")
    if rigid_iters > 0 and rigid is None:
        raise ValueError("rigid_iters > 0 needs a RigidAligner (rigid=...)")
    if occlusion and (renderer is None or splat_radius is None):
        raise ValueError("occlusion=True needs a ModelRenderer (renderer=...) and a splat_radius")
    filt = None
    if depth_filter is not None and depth_filter is not False:
        filt = dict(PREPARE_DEFAULTS)
        if depth_filter is not True:
            unknown = set(depth_filter) - set(filt)
            if unknown:
                raise TypeError(f"unknown depth_filter parameters {sorted(unknown)}")
            filt.update(depth_filter)
    pho = photo_params(photo)
    if pho is not None and (colors is None or color_image is None):
        raise ValueError("photo needs the model's colours (colors=...) and the frame's colour image (color_image=...)")
    ref = refine_params(photo_refine)
    if ref is not None and pho is None:
        raise ValueError("photo_refine refines the photometric search's matches: it needs photo=...")
    if ref is not None and template is None:
        raise ValueError("photo_refine needs the template (template=(image, px, mask or None)): the frame the model's "
                         "colours came from and every model point's pixel in it")
    d = solver.device
    prm = dict(ASSOC_DEFAULTS)
    unknown = set(assoc) - set(prm)
    if unknown:
        raise TypeError(f"unknown association parameters {sorted(unknown)}")
    prm.update(assoc)
    if int(prm["max_matches"]) > solver.max_matches:
        prm["max_matches"] = solver.max_matches
    fx, fy, cx, cy = (float(v) for v in intr[:4])
    dep = depth if isinstance(depth, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(depth, np.float32))
    dep = dep.to(device=d, dtype=torch.float32)
    nm = cim = None
    if pho is not None:
        prep = prepare_depth_device(dep, fx, fy, cx, cy, normals=True, edge_max=float(prm["edge_max"]),
                                    **(filt if filt is not None else dict(PREPARE_DEFAULTS, radius=0)))
        vm, nm = prep["point_image"], prep["normals"]
        cim = _f32(color_image, d)
        if cim.shape != vm.shape:
            raise ValueError(f"color_image must be {tuple(vm.shape)}, got {tuple(cim.shape)}")
    elif filt is None:
        vm = backproject_depth_device(dep, fx, fy, cx, cy)
    else:
        vm = prepare_depth_device(dep, fx, fy, cx, cy, normals=False, **filt)["point_image"]
    if ref is not None:
        t_im, t_px = _f32(template[0], d), _f32(template[1], d, (-1, 2))
        t_mask = template[2] if len(template) > 2 else None
        if t_im.shape != vm.shape:
            raise ValueError(f"the template image must be {tuple(vm.shape)}, got {tuple(t_im.shape)}")
    tloc, tconf = complete_node_motion_data if complete_node_motion_data is not None else (None, None)
    rot, trans, out, log = prev_rot, prev_trans, None, []
    rig = None
    ren = None
    H, W = int(vm.shape[1]), int(vm.shape[2])

    def seen(packed):
        """valid & visible under the packed transforms (device u8), and the render it came from"""
        r = renderer.render(points, normals, anchors, weights, valid, packed, (fx, fy, cx, cy), H, W, splat_radius,
                            occl_margin)
        if valid is None:
            return r["visible"], r
        v = valid if isinstance(valid, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(valid))
        return (v.to(device=d).reshape(-1) != 0).to(torch.uint8) & r["visible"], r

    if rigid_iters > 0:
        gates = {k: prm[k] for k in ("dist_max", "cos_min", "edge_max")}
        packed = pack_transforms(graph_nodes, rot, trans, d)
        v_stage = valid
        if occlusion:
            v_stage, ren = seen(packed)
        r = rigid.align(points, normals, anchors, weights, v_stage, packed, vm,
                        (fx, fy, cx, cy), pose=None, iters=rigid_iters, **gates)
        rot, trans = fold_rigid(graph_nodes, rot, trans, r["pose"])
        rig = {"pose": r["pose"], "systems": r["systems"]}
    for it in range(int(icp_iters)):
        packed = pack_transforms(graph_nodes, rot, trans, d)
        v_stage = valid
        if occlusion:
            v_stage, ren = seen(packed)
        if pho is None:
            m = associator.associate(points, normals, anchors, weights, v_stage, packed, vm, (fx, fy, cx, cy), **prm)
        else:
            m = associator.associate_photo(points, normals, colors, anchors, weights, v_stage, packed, vm, nm, cim,
                                           (fx, fy, cx, cy), dist_max=prm["dist_max"], cos_min=prm["cos_min"],
                                           max_matches=prm["max_matches"], **pho)
        log.append({"accepted": m["accepted"], "emitted": m["emitted"], "histogram": m["histogram"]})
        if m["emitted"] < 16:
            raise TooFewMatches(f"projective association {it} emitted {m['emitted']} matches of {m['accepted']} accepted "
                                f"({dict(zip(PHOTO_CODE_NAMES, m['histogram']))}); at least 16 (4·K) are needed to solve")
        if ref is not None:
            m = associator.refine_photo(m, t_im, t_px[m["match_idx"].long()], cim, vm, prm["edge_max"], t_mask, **ref)
        out = solver.optimize(graph_nodes, graph_edges, graph_edges_weights, tloc, tconf, m["src"], m["anchors"],
                              m["weights"], m["tgt"], (fx, fy, cx, cy), prev_rot=rot, prev_trans=trans, **rob)
        rot, trans = out["node_rotations"], out["node_translations"]
    if rig is not None:
        out["rigid"] = rig
    if ren is not None:
        out["render"] = ren
    return out, log, vm
