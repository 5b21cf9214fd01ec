"""FusionPipeline — the per-frame loop of the reference's working driver
(fusion_with_occlusion/fusion_tests/lepard_nicp_test.py:401-540, test4) restricted to the hot path:

    solve (GN, DeformNet.optimize formulation)  ->  warpfield.update_transformations
    ->  tsdf.integrate(target frame)  (skin cache -> ED warp -> project -> TSDF/weight/colour)

Learned front-ends (Lepard scene flow, OcclusionFusion motion completion), marching cubes and graph
updates are outside the hot path; their outputs (matches, node motion targets + confidence) are
inputs here. Everything stays device-resident across frames; no host copies inside step().
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from .registration import GaussNewtonSolver
from .tsdf import TSDFVolume, fusion_weight_params, resolve_w_min
from .warpfield import EDGraph, WarpField


@dataclass
class FrameInputs:
    im: torch.Tensor        # (6,H,W) f32 device
    src: torch.Tensor       # (M,3)
    anchors: torch.Tensor   # (M,4) i32
    weights: torch.Tensor   # (M,4) f32
    tgt: torch.Tensor       # (M,3)
    tpos: torch.Tensor      # (N,3)
    conf: torch.Tensor      # (N,)


class FusionPipeline:
    def __init__(self, seq, origin, voxel_size, dims, n_matches=10000, device=None, shard=None, gn_params=None,
                 with_color=True, overlap=False, fusion_weights=None):
        """fusion_weights (None / True / a dict of cos_power, z_ref, w_floor, edge_weight, max_weight, filter): every
        frame is fused with per-pixel observation weights and, with max_weight, a cap on the accumulated weight
        (TSDFVolume.integrate_device's weighted form; tsdf.FUSION_WEIGHT_DEFAULTS). The map is built where the frame is
        staged, from the vertex and normal maps of the filtered frame (filter: what depth_filter takes, default True);
        the integrated depth stays the raw frame. None (the default) is the reference's plain running average: the
        calls made are the ones made without this keyword."""
        self.fusion_weights = fusion_weight_params(fusion_weights)   # (TypeError / ValueError before any device work)
        self.seq = seq
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        cam = seq.cam
        self.intr = (cam.fx, cam.fy, cam.cx, cam.cy)
        self.fopt = SimpleNamespace(source_frame=0, skip_rate=1)
        self.vol = TSDFVolume.from_grid(origin, voxel_size, dims, self.intr, self.fopt, device=self.device, shard=shard)
        self.vol.with_color = with_color
        self.vol.fusion_weights = self.fusion_weights
        self.graph = EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage)
        self.wf = WarpField(self.graph, self.vol)
        self.nodes_t = torch.from_numpy(seq.nodes).to(self.device)
        self.edges_t = torch.from_numpy(seq.edges).to(self.device)
        self.ew_t = torch.from_numpy(seq.edge_weights).to(self.device)
        self.n_matches = n_matches
        self.solver = GaussNewtonSolver(seq.nodes.shape[0], n_matches, self.device, **(gn_params or {}))
        self.prev_rot = None
        self.prev_trans = None
        self.last = None
        # overlap=True: frame t's integrate runs on a stream of its own, ordered after frame t's solve but not before
        # frame t+1's — the next solve needs frame t's transforms, not its volume (bit for bit the sequential result;
        # a caller reading the volume synchronises the device, not only its own stream)
        self.overlap = overlap
        self.int_stream = None
        self._vmodel = None       # track_step(model="volume"): the last sampled volume model (padded device arrays)
        self.model_counts = []    # ... and each sampling's device [accepted, emitted]
        self._grow_frames = 0     # track_step(grow_every=): volume-model frames tracked with growth switched on

    def prepare(self, t):
        """Host-side synthetic inputs of frame t -> device (outside any timed region)."""
        d = self.device
        src, tgt, tpos, conf = self.seq.solver_inputs(t, self.n_matches)
        a, w, v = self.wf.skin_device(src)
        keep = v
        return FrameInputs(im=torch.from_numpy(self.seq.frame(t)).to(d), src=torch.from_numpy(src).to(d)[keep],
                           anchors=a[keep], weights=w[keep], tgt=torch.from_numpy(tgt).to(d)[keep],
                           tpos=torch.from_numpy(tpos).to(d), conf=torch.from_numpy(conf).to(d))

    def integrate_source(self, fi):
        self.vol.integrate({"im": fi.im, "id": 0})
        self.wf.skin_tsdf_cache()
        self.set_source_colors(fi.im)

    def set_source_colors(self, im):
        """Keep the source frame's rgb planes (a reference, no copy, no device work): what track_step(model=
        "canonical", photo=...) colours the canonical points with, at their own pixels."""
        self._source_rgb = im[:3]
        self._ccolors = None
        self._ctemplate = None

    def _canonical_template(self):
        """track_step(model="canonical", photo_refine=...)'s template: the source frame's rgb (3,H,W) on the device and
        (P,2) f32, each canonical point's own (x, y) projection into it (sub-pixel), computed once. No mask."""
        if getattr(self, "_ctemplate", None) is None:
            rgb = self._source_rgb
            rgb = rgb if isinstance(rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rgb, np.float32))
            rgb = rgb.to(self.device, torch.float32).contiguous()
            p = torch.from_numpy(np.ascontiguousarray(self.seq.canonical_points, np.float32)).to(self.device)
            fx, fy, cx, cy = (float(x) for x in self.intr[:4])
            z = p[:, 2].clamp(min=1e-6)
            px = torch.stack([p[:, 0] * fx / z + cx, p[:, 1] * fy / z + cy], 1).contiguous()
            self._ctemplate = (rgb, px, None)
        return self._ctemplate

    def _canonical_colors(self):
        """(P,3) f32 rgb of seq.canonical_points: the source frame's colour at each point's pixel (the rounded
        projection, clamped into the image), computed once."""
        if getattr(self, "_ccolors", None) is None:
            rgb = self._source_rgb
            rgb = rgb if isinstance(rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rgb, np.float32))
            rgb = rgb.to(self.device, torch.float32)
            p = torch.from_numpy(np.ascontiguousarray(self.seq.canonical_points, np.float32)).to(self.device)
            fx, fy, cx, cy = (float(x) for x in self.intr[:4])
            H, W = int(rgb.shape[1]), int(rgb.shape[2])
            z = p[:, 2].clamp(min=1e-6)
            u = torch.round(p[:, 0] * fx / z + cx).long().clamp(0, W - 1)
            v = torch.round(p[:, 1] * fy / z + cy).long().clamp(0, H - 1)
            self._ccolors = rgb[:, v, u].t().contiguous()
        return self._ccolors

    def problem(self, fi):
        """Frame fi's GN problem as GaussNewtonSolver.optimize(prefetch=) takes it."""
        return dict(graph_nodes=self.nodes_t, graph_edges=self.edges_t, graph_edges_weights=self.ew_t,
                    target_node_position=fi.tpos, node_confidence=fi.conf, source_points=fi.src, anchors=fi.anchors,
                    weights=fi.weights, target_points=fi.tgt)

    def solve(self, fi, next_fi=None):
        """GN solve of frame fi; next_fi: the next frame, whose solver setup is prefetched concurrently. Frame fi's
        depth/colour unpacking for its integrate is enqueued first (TSDFVolume.stage), so the host work between the
        solve's return and the integrate launch is only the integrate's own."""
        self.vol.fusion_weights = self.fusion_weights
        self.vol.stage(fi.im)
        out = self.solver.optimize(self.nodes_t, self.edges_t, self.ew_t, fi.tpos, fi.conf, fi.src, fi.anchors,
                                   fi.weights, fi.tgt, self.intr, prev_rot=self.prev_rot, prev_trans=self.prev_trans,
                                   sync=False, prefetch=None if next_fi is None else self.problem(next_fi))
        self.prev_rot, self.prev_trans = out["node_rotations"], out["node_translations"]
        return out

    def integrate(self, fi, t, count_updates=False, after=None):
        """Frame t's warp + integrate. overlap=True: on the pipeline's integrate stream, ordered after frame t's solve,
        and enqueued by the host inside the NEXT solve (GaussNewtonSolver.defer_to_next_solve: while that solve's host
        loop waits for its first PCG chunk), so the host work of the enqueue no longer sits between two solves;
        flush() runs a pending one now. after(): more work for that stream, right after the integrate. Returns a list
        that gets the integrate's (start, end) timing events once it is enqueued (overlap) or None."""
        if not (self.overlap and self.device.type == "cuda"):
            self._integrate(fi, t, count_updates)
            if after is not None:
                after()
            return None
        if self.int_stream is None:
            self.int_stream = torch.cuda.Stream(self.device)
        s = self.int_stream
        solved = torch.cuda.Event()
        solved.record()   # (the solve's stream: frame t's transforms are final here)
        staged, self.vol._staged = getattr(self.vol, "_staged", None), None   # (frame t's unpacked depth / colour)
        R, T = self.prev_rot, self.prev_trans
        events = []

        def enqueue():
            s.wait_event(solved)
            for x in (R, T) + (tuple(staged[1:]) if staged is not None else ()):
                if isinstance(x, torch.Tensor) and x.is_cuda:
                    x.record_stream(s)   # (made on the solve's stream: kept from reuse until the integrate has run)
            cur = getattr(self.vol, "_staged", None)
            self.vol._staged = staged
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                self.wf.set_node_transforms(R, T)
                self.wf.frame_id = t
                self.vol.update(fi.im, t)
                self.vol.integrate_device(count_updates=count_updates)
                e1.record()
                if after is not None:
                    after()
            self.vol._staged = cur
            events.extend((e0, e1))

        self.solver.defer_to_next_solve(enqueue)
        return events

    def flush(self):
        """Enqueue a deferred (overlapped) integrate now: before reading the volume or timing the loop's end."""
        self.solver.flush_deferred()

    def _integrate(self, fi, t, count_updates=False):
        self.wf.set_node_transforms(self.prev_rot, self.prev_trans)
        self.wf.frame_id = t
        self.vol.update(fi.im, t)
        self.vol.integrate_device(count_updates=count_updates)

    def step(self, fi, t, count_updates=False, next_fi=None):
        self.last = self.solve(fi, next_fi)
        self.integrate(fi, t, count_updates)
        return self.last

    def sample_model(self, max_model_points, w_min=None):
        """(Re)sample the volume model on torch's current stream (WarpField.surface_points, sync=False: no host read):
        max_model_points padded rows and their valid mask. model_counts keeps a device copy of every sampling's
        [accepted, emitted] (read them at the end of a run, not per frame). w_min (accumulated weight) None: 1.0, or the
        fusion weights' w_floor when the volume fuses with them (tsdf.resolve_w_min)."""
        w_min = resolve_w_min(w_min, self.vol.fusion_weights)
        m = self.wf.surface_points(int(max_model_points), w_min, sync=False)
        self._vmodel = m
        self.model_counts.append(m["count"].clone())
        return m

    def _rigid_aligner(self, rigid_iters, n_points):
        """The pipeline's RigidAligner, (re)made for n_points points; None while no rigid stage is asked for."""
        from .association import RigidAligner
        if int(rigid_iters) <= 0:
            return None
        if getattr(self, "_rigid", None) is None or self._rigid.max_points < n_points:
            self._rigid = RigidAligner(n_points, self.device)
        return self._rigid

    def _occlusion(self, occlusion, splat_radius, occl_margin, n_points, depth, with_normals):
        """icp_track's occlusion keywords: the pipeline's ModelRenderer, (re)made for n_points points and the depth
        image's pixels, and the default splat radius (the voxel size with normals, half of it without); {} while no
        occlusion gate is asked for."""
        from .association import ModelRenderer, default_splat_radius
        if not occlusion:
            return {}
        n_pix = int(depth.shape[0]) * int(depth.shape[1])
        ren = getattr(self, "_renderer", None)
        if ren is None or ren.max_points < n_points or ren.max_pixels < n_pix:
            self._renderer = ModelRenderer(n_points, n_pix, self.device)
        if splat_radius is None:
            splat_radius = default_splat_radius(self.vol._voxel_size, with_normals)
        return dict(occlusion=True, renderer=self._renderer, splat_radius=splat_radius, occl_margin=occl_margin)

    def grow_graph(self, max_model_points=65536, w_min=None, resample=False, **grow):
        """Grow the graph from the fused volume (WarpField.grow_from_volume; **grow: its keywords) under the transforms
        of the last integrated frame, and let the loop follow: the graph tensors and the previous transforms get the new
        rows, the solver is replaced by a larger one with the same parameters when the graph outgrows it, and the volume
        model is sampled again, because skins changed (resample=True: also when no node was added — the loop's frames that
        left the sampling after their integrate to this call). One host read (the counts). -> grow_from_volume's dict."""
        M = int(max_model_points)
        w_min = resolve_w_min(w_min, self.vol.fusion_weights)   # (None: 1.0, or the fusion weights' w_floor)
        grow.setdefault("max_points", M)
        grow.setdefault("w_min", w_min)
        self.flush()
        if self.int_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.int_stream)
        res = self.wf.grow_from_volume(**grow)
        if res["added"]:
            wf = self.wf
            N = wf.num_nodes
            self.nodes_t = wf.nodes_t
            self.edges_t = torch.from_numpy(np.ascontiguousarray(wf.graph.edges, np.int32)).to(self.device)
            self.ew_t = torch.from_numpy(np.ascontiguousarray(wf.graph.edges_weights, np.float32)).to(self.device)
            self.prev_rot, self.prev_trans = wf.R_t.clone(), wf.T_t.clone()
            if N > self.solver.max_nodes:
                old = self.solver
                self.solver = GaussNewtonSolver(min(max(N, N + N // 2), 16384), old.max_matches, self.device, **old.params)
        if self._vmodel is not None and (res["added"] or resample):
            self.sample_model(self._vmodel["points"].shape[0], w_min)
        return res

    def _motion(self, fi):
        """fi's motion term for the current graph: inputs sized for the graph before it grew (by track_step(grow_every=)
        or by grow_graph()) are padded — a new node is its own target (its current position) with confidence 0; inputs
        of the graph's size are passed on as they are."""
        tpos, conf = fi.tpos, fi.conf
        n, N = tpos.shape[0], self.nodes_t.shape[0]
        if n < N:
            tpos = torch.cat([tpos, self.nodes_t[n:] + self.prev_trans[n:]])
            conf = torch.cat([conf, torch.zeros(N - n, dtype=conf.dtype, device=conf.device)])
        return tpos, conf

    def _visible_nodes(self):
        """The nodes the last integrated frame sees (TSDFVolume.get_visible_nodes' check on the pipeline's own transforms,
        fusion.py:143), bool (N) on the host; a pending overlapped integrate is enqueued and waited for first."""
        self.flush()
        if self.int_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.int_stream)
        if not hasattr(self.vol, "depth_t"):
            raise ValueError("motion_net needs an integrated frame: integrate_source(fi) first")
        dn = self.nodes_t if self.prev_trans is None else self.nodes_t + self.prev_trans
        return self.vol.check_visibility(dn.to(torch.float32))[0]

    def _track_volume(self, fi, t, icp_iters, count_updates, motion, max_model_points, w_min, rigid_iters, assoc,
                      occ=(False, None, 0.01), depth_filter=None, grow_every=0, grow=None, photo=None, robust=None,
                      fusion=None):
        from .association import ProjectiveAssociator, icp_track, photo_params
        M = int(max_model_points)
        self.vol.fusion_weights = fusion   # (the frame staged and integrated below is fused with these, or plainly)
        if getattr(self, "_vassoc", None) is None or self._vassoc.max_points < M:
            self._vassoc = ProjectiveAssociator(M, self.device)
        if getattr(self, "_vmodel", None) is None or self._vmodel["points"].shape[0] != M:
            self.flush()
            if self.int_stream is not None:   # (an overlapped integrate of an earlier step() may still be running)
                torch.cuda.current_stream(self.device).wait_stream(self.int_stream)
            self.model_counts = []
            self.sample_model(M, w_min)       # the volume as integrate_source (or the frames so far) left it
        m = self._vmodel
        pho = {}
        if photo_params(photo) is not None:
            if not self.vol.with_color:
                raise ValueError("photo needs the model's colours: the volume does not fuse colour")
            if "colors" not in m:   # the sampled points' fused colours, once per sampling
                self.wf.surface_colors(m)
            pho = dict(photo=photo, colors=m["colors"], color_image=fi.im[:3])
        assoc.setdefault("max_matches", self.n_matches)
        self.vol.stage(fi.im)
        out, log, _ = icp_track(self._vassoc, self.solver, self.nodes_t, self.edges_t, self.ew_t, m["points"],
                                m["normals"], m["anchors"], m["weights"], m["valid"], fi.im[-1], self.intr,
                                self.prev_rot, self.prev_trans,
                                self._motion(fi) if motion else None, icp_iters,
                                rigid_iters=rigid_iters, rigid=self._rigid_aligner(rigid_iters, M),
                                depth_filter=depth_filter, robust=robust, **pho,
                                **self._occlusion(*occ, M, fi.im[-1], True), **assoc)
        out["assoc"] = log
        self.prev_rot, self.prev_trans = out["node_rotations"], out["node_translations"]
        self.last = out
        # integrate, then re-sample in the integrate's stream order; the next association reads the refreshed model, so
        # an overlapped integrate is enqueued now (flush) and this stream waits for it: no integrate / solve overlap here
        done = torch.cuda.Event()
        due = bool(grow_every) and (self._grow_frames + 1) % int(grow_every) == 0

        def resample():
            if not due:   # (a frame that grows samples after the growth: the skins change there)
                self.sample_model(M, w_min)
            done.record()
        self.integrate(fi, t, count_updates, after=resample)
        self.flush()
        torch.cuda.current_stream(self.device).wait_event(done)
        if grow_every:
            self._grow_frames += 1
            if due:
                out["grow"] = self.grow_graph(M, w_min, resample=True, **(grow or {}))
        return out

    def track_step(self, fi, t, icp_iters=3, count_updates=False, motion=True, model="canonical",
                   max_model_points=65536, w_min=None, rigid_iters=0, occlusion=False, splat_radius=None,
                   occl_margin=0.01, depth_filter=None, grow_every=0, grow=None, photo=None, robust=None,
                   fusion_weights=None, motion_net=None, photo_refine=None, **assoc):
        """step() without given matches (optional; step / solve / prepare are untouched): frame fi's depth is tracked
        by projective association of the pipeline's canonical points (seq.canonical_points, skinned once) and
        icp_iters GN solves (association.icp_track: fi's matches are not read; fi.tpos / fi.conf are the motion term
        unless motion=False), then integrated. **assoc: dist_max, cos_min, edge_max, mode, max_matches (default: the
        pipeline's n_matches). The result carries "assoc": per ICP iteration the accepted / emitted counts and the code
        histogram.

        model="volume": the tracked model is the fused volume itself instead of seq.canonical_points — surface points
        sampled from the TSDF with their voxels' cached skin and their normals (WarpField.surface_points: at most
        max_model_points rows, voxels observed with weight >= w_min), sampled once from the volume as integrate_source
        left it and again after every integrate, so that newly fused surface becomes a tracking target; a depth stream
        alone then drives the loop. The padded arrays and their valid mask go to the association as they are (no host
        read for the model; model_counts holds each sampling's device [accepted, emitted]). The re-sampling follows the
        integrate in its stream order and the next association waits for it: with overlap=True the pending integrate is
        enqueued at once (flush()), so the integrate / solve overlap does not apply in this mode.

        rigid_iters > 0 (both models): that many rigid point-to-plane iterations of all model points
        (association.RigidAligner) run before the first association; their pose is folded into the node transforms, so
        the solve and the integrate see only node transforms. The result then carries "rigid": {"pose", "systems"}.

        occlusion=True (both models): the model's own z-buffer goes in front of the rigid stage and of every association
        (association.ModelRenderer, owned by the pipeline): points that the model itself hides under the current
        estimate, by more than occl_margin metres, are left out of that stage. splat_radius defaults to the volume's
        voxel size for the volume model (it carries normals) and to half of it for the canonical points (they do not).
        The result then carries "render": the last render's dict of device tensors. No host read is added.

        depth_filter (both models; None / True / a dict of radius, sigma_s, sigma_r, range_cut): the tracker reads the
        bilateral-filtered frame's vertex map (image_proc.prepare_depth_device) instead of the raw one's; the staged
        and integrated frame stays the raw one, so the fused volume does not change with the filter itself.

        grow_every > 0 (model="volume" only): after every grow_every-th frame's integrate the graph grows from the fused
        volume (grow_graph -> WarpField.grow_from_volume; grow: a dict of its keywords), so that surface which first
        appears in a later frame gets nodes, is fused and becomes a tracking target; the result of such a frame carries
        "grow": its counts. The graph tensors, the previous transforms, the solver's capacity and the sampled model
        follow; fi.tpos / fi.conf sized for the graph before it grew are padded (a new node is its own target with
        confidence 0). One host read per growth. grow_every=0 leaves the loop as it is.

        photo (both models; None / True / a dict of radius, color_max, geo_weight): every association is the
        photometric search (ProjectiveAssociator.associate_photo): a point's target is the vertex of the best colour
        match in a window around its pixel, so that motion along the surface, which depth alone cannot see, is
        followed. The frame's colour image is fi.im[:3] (rgb in [0,1]). The volume model's colours are the fused ones
        (TSDFVolume.voxel_rgb of the sampled voxels); the canonical points take the source frame's rgb at their own
        pixels (set_source_colors(im), called by integrate_source; a ValueError without it, before any device work).
        `mode` is ignored then: the target is always the vertex. None leaves the loop as it is.

        photo_refine (model="canonical"; None / True / a dict of half, iters, eps, max_shift, min_eig, ssd_max; needs
        photo): every association's emitted matches are refined to sub-pixel before the solve
        (ProjectiveAssociator.refine_photo): the template is the source frame's rgb (kept by set_source_colors) and each
        canonical point's template pixel is its own projection into the source frame. model="volume" is a ValueError: a
        template of the rendered model is not built. None leaves the loop as it is.

        robust (both models; None / "huber" / "tukey" / {"kernel", "scale"}): every solve of the tracking loop runs with
        that robust kernel on its data rows (GaussNewtonSolver.optimize's robust=). None leaves the loop as it is.

        fusion_weights (both models; None / True / a dict, as the constructor takes it; None: the constructor's): the
        frame this call integrates is fused with per-pixel observation weights (and the weight cap max_weight). Its map
        is built where the frame is staged, ahead of the solve, from the filtered frame's vertex and normal maps
        (`filter`; not shared with depth_filter's own ofx_prepare_depth call), and an overlapped integrate gets it with
        the depth and the colour. w_min=None is 1.0 without fusion weights and their w_floor with them (fractional
        weights: 1.0 would empty the sampled model after the source frame); max_weight must not lie below it.

        motion_net (model="canonical"; None / a motion.MotionCompleter whose graph is set): the motion term comes from
        the motion completion network instead of fi.tpos / fi.conf (fusion.py:142-151). The loop above runs with no
        motion term; the nodes deformed at the previous frame and at the tracked estimate, with the previous frame's
        visible nodes (TSDFVolume.get_visible_nodes: one host read, and a pending overlapped integrate is enqueued
        first), go through the completer; one more association and solve (icp_iters=1, no rigid stage) runs from the
        tracked transforms with target_node_pos = deformed_at_source + node_motion and node_conf = confidence. The
        result carries "motion": {"node_motion", "confidence", "visible", "status"} (device tensors) and the log of
        all the associations. None leaves the loop as it is."""
        from .association import photo_params, refine_params
        from .registration import robust_params
        photo_params(photo)   # (an unknown key is a TypeError before anything is touched)
        if refine_params(photo_refine) is not None:
            if model == "volume":
                raise ValueError("photo_refine with model='volume': the template of the rendered model is not built "
                                 "(use model='canonical')")
            if photo_params(photo) is None:
                raise ValueError("photo_refine refines the photometric search's matches: it needs photo=...")
        robust_params(robust)
        fw = fusion_weight_params(fusion_weights) if fusion_weights is not None else getattr(self, "fusion_weights", None)
        w_min = resolve_w_min(w_min, fw)   # (a ValueError for a cap below it, before any device work)
        if grow_every and model != "volume":
            raise ValueError("grow_every needs model='volume': the graph grows from the fused volume")
        if model == "volume":
            if motion_net is not None:
                raise ValueError("motion_net needs model='canonical'")
            return self._track_volume(fi, t, icp_iters, count_updates, motion, max_model_points, w_min, rigid_iters,
                                      assoc, (occlusion, splat_radius, occl_margin), depth_filter, grow_every, grow,
                                      photo, robust, fw)
        if model != "canonical":
            raise ValueError(f"model must be 'canonical' or 'volume', got {model!r}")
        from .association import ProjectiveAssociator, icp_track
        pho = {}
        if photo_params(photo) is not None:
            if getattr(self, "_source_rgb", None) is None:
                raise ValueError("photo needs the model's colours: integrate_source(fi) (or set_source_colors(im)) "
                                 "takes them from the source frame")
            pho = dict(photo=photo, colors=self._canonical_colors(), color_image=fi.im[:3])
            if refine_params(photo_refine) is not None:
                pho.update(photo_refine=photo_refine, template=self._canonical_template())
        if getattr(self, "_track", None) is None:
            pts = torch.from_numpy(np.ascontiguousarray(self.seq.canonical_points, np.float32)).to(self.device)
            a, w, v = self.wf.skin_device(pts)
            self._track = (pts, a, w, v, ProjectiveAssociator(pts.shape[0], self.device))
        pts, a, w, v, assoc_h = self._track
        assoc.setdefault("max_matches", self.n_matches)
        self.vol.fusion_weights = fw
        self.vol.stage(fi.im)
        if motion_net is None:
            out, log, _ = icp_track(assoc_h, self.solver, self.nodes_t, self.edges_t, self.ew_t, pts, None, a, w, v,
                                    fi.im[-1], self.intr, self.prev_rot, self.prev_trans,
                                    self._motion(fi) if motion else None, icp_iters,
                                    rigid_iters=rigid_iters, rigid=self._rigid_aligner(rigid_iters, pts.shape[0]),
                                    depth_filter=depth_filter, robust=robust, **pho,
                                    **self._occlusion(occlusion, splat_radius, occl_margin, pts.shape[0], fi.im[-1], False),
                                    **assoc)
        else:
            from .motion import motion_term
            kw = dict(depth_filter=depth_filter, robust=robust, **pho,
                      **self._occlusion(occlusion, splat_radius, occl_margin, pts.shape[0], fi.im[-1], False), **assoc)
            first, log, _ = icp_track(assoc_h, self.solver, self.nodes_t, self.edges_t, self.ew_t, pts, None, a, w, v,
                                      fi.im[-1], self.intr, self.prev_rot, self.prev_trans, None, icp_iters,
                                      rigid_iters=rigid_iters, rigid=self._rigid_aligner(rigid_iters, pts.shape[0]), **kw)
            term, info = motion_term(motion_net, self.nodes_t, self.prev_trans, first["node_translations"],
                                     self._visible_nodes())
            out, log2, _ = icp_track(assoc_h, self.solver, self.nodes_t, self.edges_t, self.ew_t, pts, None, a, w, v,
                                     fi.im[-1], self.intr, first["node_rotations"], first["node_translations"], term, 1,
                                     **kw)
            log = log + log2
            out["motion"] = info
            if "rigid" in first:
                out["rigid"] = first["rigid"]
        out["assoc"] = log
        self.prev_rot, self.prev_trans = out["node_rotations"], out["node_translations"]
        self.last = out
        self.integrate(fi, t, count_updates)
        return out
