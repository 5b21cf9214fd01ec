"""Gauss-Newton non-rigid registration behind the reference's solver APIs, backed by libofx.

* GaussNewtonSolver.optimize — DeformNet.optimize (model/model.py:222-859) for one batch item:
  same inputs (graph nodes/edges, motion-complete node targets + confidence, source points with
  anchors/weights, target points, intrinsics, prev rot/trans), same outputs (node_rotations,
  node_translations, valid_solve, convergence_info).
* Registration.optimize — NonRigidICP/model/registration_fusion.py:98-145 API (returns
  node_rotations, node_translations, deformed_nodes_to_target, warped_verts, convergence_info,
  source/target frame ids) with the GN solver in place of the Adam/lietorch loop.
* GaussNewtonSolver.arap — DeformNet.arap (model/model.py:1639-1986): the graph-update solve that moves
  only the invalid (invisible / new) nodes under ARAP with the valid nodes held at their transforms.
* optimize_distributed — match-sharded multi-GPU solve: every rank assembles JᵀJ/Jᵀr over its own
  matches, one all-reduce (sum) of the block-sparse accumulators per GN iteration, identical solve
  on every rank.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.ofx.*)
from ._lib import call, byref
from .sharding import match_range

GN_DEFAULTS = dict(num_iter=10, lambda_flow=0.0, lambda_depth=1.0, lambda_arap=0.5, lambda_motion=1.0,
                   lm_factor=1e-7, stop_loss_diff=1.0, use_edge_weighting=False, pcg_max_iter=2000, pcg_tol=2e-6,
                   pcg_warm=True, precond_every=10, pcg_err_tol=2e-6, precond_rot_tol=0.3, precond="auto")
# PCG preconditioner (ofx_gn_params.precond): overlapping additive Schwarz, the 8-node cluster blocks, or
# auto (Schwarz for graphs of >= 1536 nodes). precond="direct" is not a preconditioner but the linear solver itself:
# every GN step solved exactly by a dense f64 Cholesky on the device (ofx_spd_solve), for graphs of <= 512 nodes — the
# reference's own LU, no PCG and no stop rule (pcg_* / precond_* ignored, pcg_iterations = 0); a larger graph raises
# OfxError. "auto" never picks it.
_PRECOND = {"cluster": 0, "schwarz": 1, "auto": 2, "direct": 3}
# Robust kernels of the data rows (ofx_gn_set_robust) and their default scales in metres: the Huber delta and the Tukey c
ROBUST_DEFAULTS = {"huber": 0.005, "tukey": 0.03}
MAX_MATCHES_EVAL = 10000   # settings/custom_settings.py:36


def _t(x, device, dtype):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.dtype == dtype and x.device == device and x.is_contiguous():
            return x   # per-frame fast path (host time: no .to / .contiguous dispatch)
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x), device=device).to(dtype).contiguous()


def robust_params(robust):
    """The robust= keyword of optimize and of the tracking layers -> (OFX_ROBUST_* code, scale in metres), or None for
    off (None / False / kernel "none"). "huber" / "tukey" take ROBUST_DEFAULTS' scale; a dict gives {"kernel": ...,
    "scale": ...} (scale optional). Another key is a TypeError; an unknown kernel, or a scale that is not finite and
    > 0, a ValueError."""
    if robust is None or robust is False:
        return None
    if isinstance(robust, str):
        kernel, scale = robust, None
    else:
        unknown = set(robust) - {"kernel", "scale"}
        if unknown:
            raise TypeError(f"unknown robust parameters {sorted(unknown)}")
        if "kernel" not in robust:
            raise ValueError("robust needs a kernel: 'huber' or 'tukey'")
        kernel, scale = robust["kernel"], robust.get("scale")
    if kernel is None or kernel == "none":
        return None
    if kernel not in ROBUST_DEFAULTS:
        raise ValueError(f"unknown robust kernel {kernel!r}: one of {sorted(ROBUST_DEFAULTS)}")
    scale = float(ROBUST_DEFAULTS[kernel] if scale is None else scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"robust scale must be finite and > 0 metres, got {scale}")
    return _lib.ROBUST_KERNELS[kernel], scale


def _prefetch_lead(num_iter):
    """OFX_PREFETCH_LEAD (A/B only): an integer clamped to [0, num_iter]; anything else is the default 1."""
    try:
        v = int(os.environ.get("OFX_PREFETCH_LEAD", "1"))
    except ValueError:
        return 1
    return min(max(v, 0), int(num_iter))


_IDLE_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p)   # ofx_gn_set_idle_hook's fn


class GaussNewtonSolver:
    def __init__(self, max_nodes, max_matches=MAX_MATCHES_EVAL, device=None, **params):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.params = dict(GN_DEFAULTS)
        self.params.update(params)
        self.max_nodes, self.max_matches = int(max_nodes), int(max_matches)
        self._keep = []
        # solver slots (handle, ordering token): a second one is made by the first prefetch (optimize(prefetch=)),
        # which sets up the next problem on the slot the current solve does not use
        self._slots = [self._new_slot()]
        self._rob = [False]             # per slot: its handle holds match weights or a robust kernel (_set_robust)
        self._last = 0                  # index of the last solve's slot
        self._cur = 0                   # slot of the next optimize()
        self._pending = [None, None]    # a prefetched problem's tensors, alive until its solve
        self._deferred = None           # defer_to_next_solve: (fn, handle) pending
        self._deferred_cb = None        # its ctypes callback, kept alive
        self._deferred_exc = None       # an exception it raised inside a solve, re-raised by the next call
        self._side = None               # torch stream that orders a prefetch before the current solve
        # GN steps of the current solve a prefetch overlaps: its setup starts when the solve begins step
        # num_iter - prefetch_lead (ofx_gn_prepare_after); 0 = when the solve's host loop returns
        self.prefetch_lead = _prefetch_lead(self.params["num_iter"])   # (env: A/B only)
        self._h, self._state = self._slots[0]   # the last solve's slot (info / stats / stopped / arap / distributed)

    def _new_slot(self):
        h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            call("ofx_gn_create", self.max_nodes, self.max_matches, byref(h))
        return h, torch.zeros(1, dtype=torch.int32, device=self.device)   # ofx::gn_* ordering token (ops.py)

    def __del__(self):
        for h, _ in getattr(self, "_slots", []):
            if h is not None and h.value:
                try:
                    _lib.lib.ofx_gn_destroy(h)
                except Exception:
                    pass
        self._slots = []
        self._h = None

    def timing(self, enable=True):
        """(pcg_ms, k_pcg_iter launches, timed PCG solves) recorded since the last call over all slots; then
        (re)arm."""
        tot = [0.0, 0, 0]
        for h, _ in self._slots:
            ms, n, ns = _lib.c_double(), _lib.c_int64(), _lib.c_int64()
            call("ofx_gn_timing", h, 1 if enable else 0, byref(ms), byref(n), byref(ns))
            tot = [tot[0] + ms.value, tot[1] + n.value, tot[2] + ns.value]
        return tuple(tot)

    def prefetch_stats(self):
        """(solves that used a prefetched setup, solves that discarded one) over all slots."""
        used = missed = 0
        for h, _ in self._slots:
            u, m = _lib.c_int64(), _lib.c_int64()
            call("ofx_gn_prefetch_stats", h, byref(u), byref(m))
            used, missed = used + u.value, missed + m.value
        return used, missed

    def defer_to_next_solve(self, fn):
        """Run fn() once inside the next optimize(), while its host loop waits for the first GN step's PCG chunk
        (ofx_gn_set_idle_hook: the host only spins there), or at that optimize's return if it never waited. A frame
        loop enqueues the previous frame's integrate this way without delaying the next solve's first launches.
        flush_deferred() runs a pending fn now."""
        self.flush_deferred()
        h = self._slots[self._cur][0]

        def hook(_arg):
            self._run_deferred()
        self._deferred_cb = _IDLE_HOOK(hook)
        self._deferred = (fn, h)
        call("ofx_gn_set_idle_hook", h, ctypes.cast(self._deferred_cb, ctypes.c_void_p), None)

    def _run_deferred(self):
        d, self._deferred = self._deferred, None
        if d is None:
            return
        try:
            d[0]()
        except BaseException as e:   # (inside the library's host loop: kept, raised by the next Python-level call)
            self._deferred_exc = e

    def flush_deferred(self):
        """Run a pending defer_to_next_solve() fn now (and raise what a deferred fn raised)."""
        if self._deferred is not None:
            call("ofx_gn_set_idle_hook", self._deferred[1], None, None)
            self._run_deferred()
        if self._deferred_exc is not None:
            e, self._deferred_exc = self._deferred_exc, None
            raise e

    def drain(self):
        """Order the current stream after any prefetched setup still in flight (ofx_gn_prepare_wait): a
        synchronisation afterwards covers it."""
        s = _lib.stream_ptr(torch.cuda.current_stream(self.device))
        for h, _ in self._slots:
            call("ofx_gn_prepare_wait", h, s)

    def info(self):
        """[n_nodes, n_matches, JᵀJ block count, residual terms, PCG rows] of the last solve's setup."""
        arr = (ctypes.c_int64 * 5)()
        call("ofx_gn_info", self._h, arr)
        return list(arr)

    def precond_info(self):
        """The last setup's preconditioner: dict(schwarz, clusters, segments, sources, gathered_rows, subdomain_rows,
        row_length, launches_per_iteration)
        (ofx_gn_precond_info; synchronises the device: tools and bench only)."""
        arr = (ctypes.c_int64 * 8)()
        call("ofx_gn_precond_info", self._h, arr)
        return dict(zip(("schwarz", "clusters", "segments", "sources", "gathered_rows", "subdomain_rows", "row_length",
                         "launches_per_iteration"), list(arr)))

    def solver_info(self):
        """The last setup's linear solver: dict(direct, unknowns, panel_width, launches_per_gn_step)
        (ofx_gn_solver_info; direct = 1 when precond="direct" served the problem, 0 under the PCG)."""
        arr = (ctypes.c_int64 * 4)()
        call("ofx_gn_solver_info", self._h, arr)
        return dict(zip(("direct", "unknowns", "panel_width", "launches_per_gn_step"), list(arr)))

    def stopped(self):
        """The solve's stop flag as the host sees it (ofx_gn_stopped: no synchronisation)."""
        f = ctypes.c_int32()
        call("ofx_gn_stopped", self._h, byref(f))
        return bool(f.value)

    def pcg_waves(self):
        """Waves per cluster workgroup of the PCG iteration kernel in the last setup (2 up to 384 clusters, else 1;
        1 under OFX_PCG_W1=1)."""
        w = ctypes.c_int32()
        call("ofx_gn_pcg_waves", self._h, byref(w))
        return w.value

    def step_fused(self):
        """True if the last GN step's update was taken by its converging PCG launch (include/ofx.h
        ofx_gn_step_fused): its stop flag is then already visible to the host."""
        f = ctypes.c_int32()
        call("ofx_gn_step_fused", self._h, byref(f))
        return bool(f.value)

    def row_order(self):
        """PCG row -> node of the last setup (-1: padding row); the order of rhs / the state rows."""
        rows = self.info()[4]
        arr = np.empty(rows, np.int32)
        call("ofx_gn_row_order", self._h, arr.ctypes.data_as(ctypes.c_void_p), rows)
        return arr

    def stats(self):
        """Per GN step of the last solve: (PCG iterations, |b|², loss) rows; steps that did not run are 0."""
        n = int(self.params["num_iter"])
        arr = (ctypes.c_double * (3 * max(1, n)))()
        call("ofx_gn_stats", self._h, arr, n)
        return np.array(arr[:3 * n], dtype=np.float64).reshape(n, 3)

    def _plist(self, mode=0, pcg_tol=None):
        """GN parameters as the ofx::gn_* operators take them (ops._gn_params)."""
        q = self.params
        fp = [float(q["lambda_flow"]), float(q["lambda_depth"]), float(q["lambda_arap"]), float(q["lambda_motion"]),
              float(q["lm_factor"]), float(q["stop_loss_diff"]), float(q["pcg_tol"] if pcg_tol is None else pcg_tol),
              float(q.get("pcg_err_tol", 0.0)), float(q.get("precond_rot_tol", 0.0))]
        ip = [int(q["num_iter"]), int(bool(q["use_edge_weighting"])), int(q["pcg_max_iter"]), int(bool(q["pcg_warm"])),
              int(mode), int(q.get("precond_every", 1)), _PRECOND[q.get("precond", "cluster")]]
        return fp, ip

    def _match_weights(self, match_weights, M):
        if match_weights is None:
            return None
        mw = _t(match_weights, self.device, torch.float32).reshape(-1)
        if mw.shape[0] != M:
            raise ValueError(f"match_weights has {mw.shape[0]} entries for {M} matches")
        return mw

    def _set_robust(self, slot, mw, rp):
        """The slot's handle takes exactly this setting (torch.ops.ofx.gn_set_robust: mw a device f32 (M) tensor or None,
        rp robust_params' pair or None); off on a handle that is off already is no call at all, so a solver that never
        uses the feature issues what it always did."""
        on = mw is not None or rp is not None
        if not on and not self._rob[slot]:
            return
        h, st = self._slots[slot]
        kernel, scale = rp if rp is not None else (0, 0.0)
        torch.ops.ofx.gn_set_robust(st, h.value, mw, kernel, scale)
        self._rob[slot] = on

    def _problem(self, graph_nodes, graph_edges, graph_edges_weights, target_node_position, node_confidence,
                 source_points, anchors, weights, target_points, intrinsics, target_px, target_py, prev_rot,
                 prev_trans, keep=True):
        """Device tensors of one problem in the ofx::gn_* operators' argument order (+ N, M)."""
        d = self.device
        nodes = _t(graph_nodes, d, torch.float32).reshape(-1, 3)
        N = nodes.shape[0]
        src = _t(source_points, d, torch.float32).reshape(-1, 3)
        M = src.shape[0]
        if N > self.max_nodes or M > self.max_matches:
            raise ValueError(f"problem ({N} nodes, {M} matches) exceeds solver capacity "
                             f"({self.max_nodes}, {self.max_matches})")
        args = [nodes, _t(graph_edges, d, torch.int32).reshape(N, -1), _t(graph_edges_weights, d, torch.float32),
                (_t(target_node_position, d, torch.float32).reshape(N, 3) if target_node_position is not None
                 else nodes.clone()),
                (_t(node_confidence, d, torch.float32).reshape(N) if node_confidence is not None
                 else torch.zeros(N, device=d)),
                src, _t(anchors, d, torch.int32).reshape(M, 4), _t(weights, d, torch.float32).reshape(M, 4),
                _t(target_points, d, torch.float32).reshape(M, 3), _t(target_px, d, torch.float32),
                _t(target_py, d, torch.float32), _t(prev_rot, d, torch.float32), _t(prev_trans, d, torch.float32),
                [float(v) for v in np.asarray(intrinsics, np.float64).reshape(-1)[:4]]]
        if keep:
            self._keep = args   # the last problem's inputs (arap reads prev_trans back)
        return args, N, M

    @staticmethod
    def _pack(out, sync):
        rot, trans, status, loss = out
        res = {"node_rotations": rot, "node_translations": trans, "_status": status, "_loss": loss}
        if sync:
            st = status.cpu().numpy()
            loss = loss.cpu().numpy()[:st[1]]
            res["valid_solve"] = int(st[0])
            res["convergence_info"] = {"total": loss[:, 0].tolist(), "data": loss[:, 1].tolist(),
                                       "arap": loss[:, 2].tolist(), "motion": loss[:, 3].tolist(),
                                       "valid": int(st[0]), "gn_iterations": int(st[1]),
                                       "pcg_iterations": int(st[2]), "pcg_capped_steps": int(st[4]),
                                       "errors": ["Solver failed: Ill-posed system!"] if st[3] else []}
        return res

    def optimize(self, graph_nodes, graph_edges, graph_edges_weights, target_node_position, node_confidence,
                 source_points, anchors, weights, target_points, intrinsics, target_px=None, target_py=None,
                 prev_rot=None, prev_trans=None, sync=True, prefetch=None, match_weights=None, robust=None):
        """model.py:222-859 (batch item) through torch.ops.ofx.gn_solve. Returns torch device tensors (+ host
        convergence info if sync).

        match_weights: (M) per-match weights, or None = all 1: match m's residual and Jacobian rows are multiplied by
        it, as correspondence_weights does in DeformNet.forward (model.py:1338,1374-1378; its weight in the objective
        is the square). robust: None, "huber", "tukey" or {"kernel": ..., "scale": metres} (ROBUST_DEFAULTS: Huber
        0.005, Tukey 0.03) — an M-estimator on the data rows, reweighted at every GN step from the match's geometric
        distance |p - tgt| (ofx_gn_set_robust). Every call sets the solving slot to what it asks, so neither carries over
        to a later call; both None is the solve as it was.

        prefetch: the NEXT frame's problem as a dict of this method's argument names (graph_nodes ...
        target_points, optional target_px / target_py; intrinsics default to this call's; no pose). Its setup
        (upload, JᵀJ pattern, with the setup's host sync) is started on the other solver slot when this solve's
        host loop returns, ordered before this solve, and runs concurrently with this frame's tail
        (torch.ops.ofx.gn_prepare); the next optimize() with that problem (the same device tensors) then skips
        its setup. The prefetched tensors must not change until
        that call. The dict may carry match_weights / robust too: the next optimize() must then be given the same
        weight tensor (device f32) and the same robust setting, or the prefetched setup is discarded."""
        rp = robust_params(robust)
        args, N, M = self._problem(graph_nodes, graph_edges, graph_edges_weights, target_node_position,
                                   node_confidence, source_points, anchors, weights, target_points, intrinsics,
                                   target_px, target_py, prev_rot, prev_trans)
        mw = self._match_weights(match_weights, M)
        fp, ip = self._plist()
        cur = self._cur
        h, st = self._slots[cur]
        if prefetch is not None:
            # The prefetch problem's tensors are made first (any conversion / default it needs runs on the current
            # stream), then the prefetch is ordered after the work enqueued so far (those producers, its inputs,
            # the other slot's last solve) but not after this solve: it is started when this solve's host loop
            # returns, so its kernels overlap this frame's tail (the drained PCG launches, the integrate) instead
            # of the PCG chain. Inputs that need conversion are new tensors on every call, so such a prefetch is
            # correct but never matches the next solve (it is set up inline then: prefetch_stats counts a miss).
            q = dict(prefetch)
            pa, _, _ = self._problem(q["graph_nodes"], q["graph_edges"], q["graph_edges_weights"],
                                     q["target_node_position"], q["node_confidence"], q["source_points"],
                                     q["anchors"], q["weights"], q["target_points"], q.get("intrinsics", intrinsics),
                                     q.get("target_px"), q.get("target_py"), None, None, keep=False)
            pr = (self._match_weights(q.get("match_weights"), pa[5].shape[0]), robust_params(q.get("robust")))
            before = torch.cuda.Event()
            before.record()
            lead = int(self.prefetch_lead)
            if lead > 0:   # queued now, started by this solve at GN step num_iter - lead (or when it returns)
                self._prefetch(pa, before, h, int(self.params["num_iter"]) - lead, fp, ip, pr)
        self._set_robust(cur, mw, rp)
        if self._deferred is not None and self._deferred[1].value != h.value:   # (hooked on another slot)
            self.flush_deferred()
        out = torch.ops.ofx.gn_solve(st, h.value, *args, fp, ip)
        self.flush_deferred()   # (a deferred fn the solve never reached — no PCG wait — runs now; its exception too)
        self._pending[cur] = None
        self._h, self._state, self._last = h, st, cur
        if prefetch is not None:
            if lead <= 0:
                self._prefetch(pa, before, None, 0, fp, ip, pr)
            self._cur = 1 - cur
        return self._pack(out, sync)

    def _prefetch(self, pa, before, trigger, step, fp, ip, pr=(None, None)):
        """Queue the next problem's setup on the other slot, ordered after `before` (torch.ops.ofx.gn_prepare), under
        the match weights / robust setting pr that the problem comes with."""
        nxt = 1 - self._cur
        if len(self._slots) < 2:
            self._slots.append(self._new_slot())
            self._rob.append(False)
            call("ofx_gn_share_history", self._slots[1][0], self._slots[0][0])
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        h1, st1 = self._slots[nxt]
        with torch.cuda.stream(self._side):
            self._side.wait_event(before)
            self._set_robust(nxt, *pr)
            torch.ops.ofx.gn_prepare(st1, h1.value, *pa[:11], pa[13], fp, ip, trigger.value if trigger else 0,
                                     max(step, 0))
        self._pending[nxt] = (pa, pr[0])

    def arap(self, graph_nodes, source_node_position, target_node_position, valid_nodes_mask, original_graph_nodes,
             graph_edges, graph_edges_weights, graph_clusters, R_current, t_current, sync=True, pcg_tol=1e-10):
        """model.py:1639-1986. graph_nodes (N,3) at the source; source/target_node_position (V,3) of the
        V valid nodes (mask order); only invalid nodes are updated. The reference builds its ARAP rows on
        original_graph_nodes and its data rows on graph_nodes; its only caller passes the same array for
        both (run_model.py:604-619), which this solver requires. Returns node_rotations (N,3,3),
        node_translations (N,3), deformed_nodes_to_target (V,3), valid_solve, convergence_info."""
        d = self.device
        nodes = _t(graph_nodes, d, torch.float32).reshape(-1, 3)
        N = nodes.shape[0]
        if original_graph_nodes is not None and not torch.equal(_t(original_graph_nodes, d, torch.float32).reshape(N, 3),
                                                                nodes):
            raise ValueError("arap: original_graph_nodes must equal graph_nodes (run_model.py:604-619)")
        valid = _t(valid_nodes_mask, d, torch.bool).reshape(N)
        vidx = torch.nonzero(valid).reshape(-1)
        conv = {"total": [], "arap": [], "data": [], "condition_numbers": [], "valid": 0, "errors": []}
        if vidx.numel() == 0:                          # model.py:1683-1687
            conv["errors"].append("Solver failed: No valid correspondences after filtering")
            return {"convergence_info": conv}
        src = _t(source_node_position, d, torch.float32).reshape(-1, 3)
        if not torch.equal(src, nodes[vidx]):
            raise ValueError("arap: source_node_position must be graph_nodes[valid_nodes_mask] (tsdf.py:660-661)")
        tpos = torch.zeros((N, 3), device=d)
        tpos[vidx] = _t(target_node_position, d, torch.float32).reshape(-1, 3)
        z3 = np.zeros((0, 3), np.float32)
        args, N, _ = self._problem(nodes, graph_edges, graph_edges_weights, tpos, valid.float(), z3,
                                   np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), z3, (1.0, 1.0, 0.0, 0.0),
                                   None, None, R_current, t_current)
        fp, ip = self._plist(mode=1, pcg_tol=pcg_tol)
        self._set_robust(self._last, None, None)   # (no data rows to weigh)
        out = torch.ops.ofx.gn_solve(self._state, self._h.value, *args, fp, ip)
        res = self._pack(out, sync)
        t_init = self._keep[12]                              # prev_trans as uploaded
        t0 = t_init[vidx] if t_init is not None else torch.zeros_like(src)
        res["deformed_nodes_to_target"] = src + t0          # valid nodes never move (model.py:1719,1961-1962)
        if sync:
            ci = res["convergence_info"]
            res["convergence_info"] = {"total": ci["total"], "arap": ci["arap"], "data": ci["data"],
                                       "condition_numbers": [], "valid": ci["valid"], "errors": ci["errors"],
                                       "gn_iterations": ci["gn_iterations"], "pcg_iterations": ci["pcg_iterations"],
                                       "pcg_capped_steps": ci["pcg_capped_steps"]}
        return res

    def optimize_distributed(self, graph_nodes, graph_edges, graph_edges_weights, target_node_position,
                             node_confidence, source_points, anchors, weights, target_points, intrinsics,
                             target_px=None, target_py=None, prev_rot=None, prev_trans=None, group=None, sync=True,
                             timer=None):
        """Match-sharded solve over torch.distributed: rank r assembles matches [r*M/W, (r+1)*M/W);
        A and rhs are all-reduced (sum) once per GN iteration; rank 0 adds ARAP + motion rows.
        timer: a list that receives (start, end) CUDA events around each GN step's all-reduce."""
        import torch.distributed as dist
        args, N, M = self._problem(graph_nodes, graph_edges, graph_edges_weights, target_node_position,
                                   node_confidence, source_points, anchors, weights, target_points, intrinsics,
                                   target_px, target_py, prev_rot, prev_trans)
        fp, ip = self._plist()
        h = self._h.value
        self._set_robust(self._last, None, None)   # (the sharded solve takes no match weights)
        nnz, rows = (int(v) for v in torch.ops.ofx.gn_setup(self._state, h, *args, fp, ip))
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        m0, m1 = match_range(M, rank, world)
        A = torch.empty(nnz * 36, dtype=torch.float64, device=self.device)
        rhs = torch.empty(6 * rows + 4, dtype=torch.float64, device=self.device)   # include/ofx.h: ofx_gn_linearize
        for it in range(int(self.params["num_iter"])):
            torch.ops.ofx.gn_linearize(self._state, h, it, m0, m1, rank == 0, A, rhs)
            if timer is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            dist.all_reduce(A, group=group)
            dist.all_reduce(rhs, group=group)
            if timer is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                timer.append((e0, e1))
            torch.ops.ofx.gn_step(self._state, h, it, A, rhs)
            # The stop decision of step `it` is identical on every rank (identical all-reduced systems). A step fused
            # into its converging PCG launch stored the stop flag before the convergence flag the host already saw;
            # otherwise (k_step as its own launch, after pcg_max_iter launches) the flag is written asynchronously:
            # read it only after the step has run, so that every rank leaves the loop after the same step and the
            # collectives stay matched.
            if not self.step_fused():
                torch.cuda.current_stream(self.device).synchronize()
            if self.stopped():
                break
        out = torch.ops.ofx.gn_finish(self._state, h, N, int(self.params["num_iter"]))
        return self._pack(out, sync)


def spd_solve(A, b):
    """Dense f64 solve A x = b of a symmetric positive definite A on the device (torch.ops.ofx.spd_solve, on copies):
    -> (L, x, status). A (n,n) / b (n): CUDA float64 tensors or arrays (uploaded to the current device); only A's lower
    triangle is read; 1 <= n <= 3072 (else OfxError). status = [not positive definite, first bad pivot]; x = 0 then."""
    d = A.device if isinstance(A, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    At = A if isinstance(A, torch.Tensor) else torch.as_tensor(np.asarray(A, np.float64), device=d)
    bt = b if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, np.float64), device=d)
    return torch.ops.ofx.spd_solve(At, bt)


def depth_2_pc_device(depth, intrin):
    from .image_proc import depth_2_pc_device as f
    return f(depth, intrin)


class Registration:
    """registration_fusion.py:37-397 API with the Gauss-Newton solver (DeformNet.optimize formulation)."""

    def __init__(self, canonical_vertices, graph, warpfield, K, vis=None, max_matches=MAX_MATCHES_EVAL, seed=0,
                 **gn_params):
        self.graph = graph
        self.warpfield = warpfield
        self.intrinsics = np.asarray(K, np.float64)
        self.vis = vis
        self.device = warpfield.device
        self.max_matches = max_matches
        self.rng = np.random.default_rng(seed)
        self.solver = GaussNewtonSolver(graph.nodes.shape[0], max_matches, self.device, **gn_params)
        self.prev_rot = None
        self.prev_trans = None
        self.update(canonical_vertices)

    def update(self, canonical_vertices, colors=None, template=None):
        """registration_fusion.py:66-85: skin the canonical vertices, keep the valid ones. colors: optional rgb in [0,1]
        of the vertices, (V,3): kept for the valid ones as source_colors, what track(photo=...) matches with. template:
        optional (image (3,H,W) rgb, px (V,2): every vertex's (x, y) place in it, sub-pixel, optional mask (H,W)) — the
        frame the colours came from: kept, with the valid vertices' px, as source_template, what track(photo_refine=...)
        refines the matches against."""
        a, w, v = self.warpfield.skin_device(canonical_vertices)
        self.valid_source_verts = v.cpu().numpy()
        vt = torch.as_tensor(np.ascontiguousarray(canonical_vertices, np.float32), device=self.device)
        self.source_pcd = vt[v]
        self.point_anchors = a[v]
        self.anchor_weight = w[v]
        self.source_normals = None   # (set by update_from_volume only: caller-given vertices carry no normals)
        self.source_colors = None
        if colors is not None:
            self.source_colors = torch.as_tensor(np.ascontiguousarray(colors, np.float32),
                                                 device=self.device).reshape(-1, 3)[v]
        self.source_template = None
        if template is not None:
            px = torch.as_tensor(np.ascontiguousarray(template[1], np.float32), device=self.device).reshape(-1, 2)[v]
            self.source_template = (template[0], px, template[2] if len(template) > 2 else None)

    def update_from_volume(self, max_points=None, w_min=1.0):
        """The model from the fused volume instead of caller-given vertices (the reference's per-frame
        optimizer.update(tsdf.get_canonical_model()[0]), fusion_tests/lepard_nicp_test.py:537, without the mesh and
        the k-NN skin): WarpField.surface_points — surface voxels of the TSDF observed with weight >= w_min, with the
        skin the integrate warps them with — becomes source_pcd / point_anchors / anchor_weight, every point valid, and
        source_normals holds their unit normals, which track() then gates with. max_points: None keeps every accepted
        voxel (one more host read to size the arrays), else they are thinned evenly to at most that many. Needs the
        warp field's skin cache (skin_tsdf_cache()). A volume that fuses colour also gives source_colors: the points'
        fused rgb (TSDFVolume.voxel_rgb), what track(photo=...) matches with. -> the number of model points."""
        wf = self.warpfield
        if max_points is None:
            max_points = wf.surface_points(0, w_min)["accepted"]
        m = wf.surface_points(int(max_points), w_min)
        self.source_colors = wf.surface_colors(m) if getattr(wf.tsdf, "with_color", False) else None
        self.source_template = None   # (a template of the rendered model is not built)
        self.source_pcd = m["points"].clone()
        self.point_anchors = m["anchors"].clone()
        self.anchor_weight = m["weights"].clone()
        self.source_normals = m["normals"].clone()
        self.valid_source_verts = np.ones(m["emitted"], bool)
        return m["emitted"]

    def grow_from_volume(self, **kw):
        """Grow the graph from the fused volume (WarpField.grow_from_volume, its keywords) and follow it: the previous
        transforms get the new nodes' rows, the solver is replaced by a larger one with the same parameters when the
        graph outgrows it, and the model is taken from the volume again (update_from_volume with the same max_points /
        w_min), because skins changed. -> grow_from_volume's dict."""
        wf = self.warpfield
        res = wf.grow_from_volume(**kw)
        if res["added"]:
            self.graph = wf.graph
            N = wf.num_nodes
            self.prev_rot, self.prev_trans = wf.R_t.clone(), wf.T_t.clone()
            if N > self.solver.max_nodes:
                old = self.solver
                self.solver = GaussNewtonSolver(min(max(N, N + N // 2), 16384), old.max_matches, self.device, **old.params)
        self.update_from_volume(kw.get("max_points", 65536), kw.get("w_min", 1.0))
        return res

    def _intr4(self):
        K = self.intrinsics
        return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(-1)[:4])

    def optimize(self, optical_flow_data, scene_flow_data, complete_node_motion_data, target_frame_data,
                 landmarks=None):
        im = target_frame_data.get("im") if isinstance(target_frame_data, dict) else None
        if im is not None:   # registration_fusion.py:104-109: target cloud + pixel map (ofx_depth_to_pc)
            depth = torch.as_tensor(np.ascontiguousarray(im[-1], np.float32), device=self.device)
            self.tgt_pcd, self.pix_2_pcd = depth_2_pc_device(depth, self.intrinsics)
        tm = np.asarray(scene_flow_data["target_matches"], np.float32)[self.valid_source_verts]
        vv = np.asarray(scene_flow_data["valid_verts"], bool)
        sel = np.nonzero(vv[: self.source_pcd.shape[0]])[0]
        if sel.size > self.max_matches:           # model.py:319-334 (reference: unseeded randperm)
            sel = np.sort(self.rng.choice(sel, self.max_matches, replace=False))
        idx = torch.as_tensor(sel, device=self.device, dtype=torch.int64)
        tloc, tconf = complete_node_motion_data if complete_node_motion_data is not None else (None, None)
        # per-vertex correspondence weights of the target frame, if it brings any (DeformNet.forward's
        # correspondence_weights, model.py:1338,1374-1378): the selected matches' go to the solve as match_weights
        cw = target_frame_data.get("correspondence_weights") if isinstance(target_frame_data, dict) else None
        if cw is not None:
            cw = np.asarray(cw, np.float32).reshape(-1)[self.valid_source_verts][sel]
        out = self.solver.optimize(self.graph.nodes, self.graph.edges, self.graph.edges_weights, tloc, tconf,
                                   self.source_pcd[idx], self.point_anchors[idx], self.anchor_weight[idx],
                                   tm[sel], self._intr4(), prev_rot=self.prev_rot, prev_trans=self.prev_trans,
                                   match_weights=cw)
        R, T = out["node_rotations"], out["node_translations"]
        self.prev_rot, self.prev_trans = R.clone(), T.clone()
        nodes_t = torch.as_tensor(self.graph.nodes, device=self.device)
        self.warpfield.set_node_transforms(R, T)
        warped = self.warpfield.deform_device(self.source_pcd, self.point_anchors, self.anchor_weight)
        # dtypes as registration_fusion.py:363-377: rotations numpy f64 (scipy as_matrix), translations a CPU
        # tensor, deformed nodes and warped vertices device tensors
        res = {"warped_verts": warped, "node_rotations": R.cpu().numpy().astype(np.float64), "node_translations": T.cpu(),
               "deformed_nodes_to_target": nodes_t + T, "convergence_info": out["convergence_info"],
               "valid_solve": out["valid_solve"],
               "source_frame_id": optical_flow_data["source_id"], "target_frame_id": optical_flow_data["target_id"]}
        return res

    def track(self, target_frame_data, complete_node_motion_data=None, source_normals=None, icp_iters=3,
              rigid_iters=0, occlusion=False, splat_radius=None, occl_margin=0.01, depth_filter=None, photo=None,
              robust=None, motion_net=None, photo_refine=None, **assoc):
        """Register the target depth frame without given matches (no reference twin: the reference's matches come from
        learned front-ends). target_frame_data: {"im": (6,H,W) image, depth last, optional "id"}. The depth is
        backprojected to the vertex map (and tgt_pcd / pix_2_pcd are set as optimize does); then icp_iters times:
        projective association (association.ProjectiveAssociator, ofx_associate) of source_pcd under the current
        prev_rot / prev_trans, and a GN solve on the emitted matches from that estimate. source_normals: unit normals of
        the canonical vertices given to update() (all of them, or the valid ones only), or None (no normal gate; after
        update_from_volume(): the volume model's own normals).
        **assoc: dist_max, cos_min, edge_max, mode ("plane" / "point"), max_matches. Without motion data the motion
        rows vanish (nodes as targets, confidence 0). Raises association.TooFewMatches, with no solve launched, if an
        association emits fewer than 4·K = 16 matches. Returns optimize's result dict (frame ids: None and the
        target's "id") plus "assoc": per ICP iteration the accepted count, the emitted count and the histogram of the
        codes. One host synchronisation per association (its counts) besides the solves' own.
        rigid_iters > 0: that many rigid point-to-plane iterations of all of source_pcd (association.RigidAligner,
        ofx_rigid_icp) run first and their pose is folded into the estimate the loop starts from; the result then has
        "rigid": {"pose" (3,4) f64, "systems"} as device tensors. The stage adds no host synchronisation.
        occlusion=True: before the rigid stage and every association the model is rendered under the current estimate
        (association.ModelRenderer, ofx_splat_points, owned by this object) and the points the model itself hides —
        more than occl_margin metres behind its z-buffer — are left out of that stage; splat_radius (metres) defaults
        to the volume's voxel size when the model carries normals and to half of it when it does not. The result then
        has "render": the last render's dict of device tensors. No host synchronisation is added.
        depth_filter (None / True / a dict of radius, sigma_s, sigma_r, range_cut): the rigid stage and the associations
        read the bilateral-filtered frame's vertex map (image_proc.prepare_depth_device) instead of the raw one's; tgt_pcd
        / pix_2_pcd are still the raw depth's. None is the loop as it was.
        photo (None / True / a dict of radius, color_max, geo_weight): every association is the photometric search
        (ProjectiveAssociator.associate_photo, ofx_photo_associate) — each point's target is the vertex of the best
        colour match in a window around its pixel, among the pixels that pass the geometric gates — which also follows
        motion along the surface that depth alone cannot see. The frame's colour image is im[:3] (rgb in [0,1]); the
        model's colours are source_colors (update(colors=...), or update_from_volume() of a volume that fuses colour):
        without them a ValueError, before any device work. `mode` is ignored then: the target is always the vertex.
        None is the loop as it was.
        photo_refine (None / True / a dict of half, iters, eps, max_shift, min_eig, ssd_max; needs photo): every
        association's emitted matches are refined to sub-pixel before the solve (ProjectiveAssociator.refine_photo,
        ofx_photo_refine) against source_template (update(vertices, colors=, template=)): without photo or without the
        template a ValueError, before any device work. None is the loop as it was.
        robust (None / "huber" / "tukey" / {"kernel", "scale"}): every solve of the loop runs with that robust kernel on
        its data rows (GaussNewtonSolver.optimize's robust=); None is the loop as it was.
        motion_net (None / a motion.MotionCompleter whose graph is set): the motion term comes from the motion completion
        network (fusion.py:142-151) instead of complete_node_motion_data: the loop runs with no motion term; the nodes
        deformed at the source (graph.nodes + prev_trans) and at the tracked estimate, with the visible nodes of the
        warp field's volume at its last frame (TSDFVolume.get_visible_nodes; a ValueError without a volume), go through
        the completer; one more association and solve (icp_iters=1, no rigid stage) runs from the tracked transforms
        with target_node_pos = deformed_at_source + node_motion and node_conf = confidence. The result then has
        "motion": {"node_motion", "confidence", "visible", "status"}. None is the loop as it was."""
        robust_params(robust)   # (refused before anything is touched)
        from .association import (ModelRenderer, ProjectiveAssociator, RigidAligner, default_splat_radius, icp_track,
                                  photo_params, refine_params)
        pho = {}
        if refine_params(photo_refine) is not None:
            if photo_params(photo) is None:
                raise ValueError("photo_refine refines the photometric search's matches: it needs photo=...")
            if getattr(self, "source_template", None) is None:
                raise ValueError("photo_refine needs the template: update(vertices, colors=..., template=(image, px, "
                                 "mask or None))")
        if photo_params(photo) is not None:
            if getattr(self, "source_colors", None) is None:
                raise ValueError("photo needs the model's colours: update(vertices, colors=...) or update_from_volume() "
                                 "of a volume that fuses colour")
            pho = dict(photo=photo, colors=self.source_colors, color_image=target_frame_data["im"][:3])
            if refine_params(photo_refine) is not None:
                pho.update(photo_refine=photo_refine, template=self.source_template)
        depth = torch.as_tensor(np.ascontiguousarray(target_frame_data["im"][-1], np.float32), device=self.device)
        self.tgt_pcd, self.pix_2_pcd = depth_2_pc_device(depth, self.intrinsics)
        P = self.source_pcd.shape[0]
        if getattr(self, "_assoc", None) is None or self._assoc.max_points < P:
            self._assoc = ProjectiveAssociator(P, self.device)
        nrm = getattr(self, "source_normals", None)   # a model from the volume (update_from_volume) brings its normals
        if source_normals is not None:
            nrm = torch.as_tensor(np.ascontiguousarray(source_normals, np.float32), device=self.device).reshape(-1, 3)
            if nrm.shape[0] != P:
                nrm = nrm[torch.as_tensor(self.valid_source_verts, device=self.device)]
        assoc.setdefault("max_matches", self.max_matches)
        if int(rigid_iters) > 0 and (getattr(self, "_rigid", None) is None or self._rigid.max_points < P):
            self._rigid = RigidAligner(P, self.device)
        occ = {}
        if occlusion:
            if splat_radius is None:
                vol = getattr(self.warpfield, "tsdf", None)
                if vol is None:
                    raise ValueError("occlusion=True needs a splat_radius: the warp field has no volume to take it from")
                splat_radius = default_splat_radius(vol._voxel_size, nrm is not None)
            n_pix = int(depth.shape[0]) * int(depth.shape[1])
            ren = getattr(self, "_renderer", None)
            if ren is None or ren.max_points < P or ren.max_pixels < n_pix:
                self._renderer = ModelRenderer(P, n_pix, self.device)
            occ = dict(occlusion=True, renderer=self._renderer, splat_radius=splat_radius, occl_margin=occl_margin)
        if motion_net is not None and getattr(self.warpfield, "tsdf", None) is None:
            raise ValueError("motion_net needs the warp field's volume (its last frame gives the visible nodes)")
        out, log, _ = icp_track(self._assoc, self.solver, self.graph.nodes, self.graph.edges, self.graph.edges_weights,
                                self.source_pcd, nrm, self.point_anchors, self.anchor_weight, None, depth,
                                self._intr4(), self.prev_rot, self.prev_trans,
                                complete_node_motion_data if motion_net is None else None, icp_iters,
                                rigid_iters=rigid_iters, rigid=getattr(self, "_rigid", None),
                                depth_filter=depth_filter, robust=robust, **pho, **occ, **assoc)
        minfo = None
        if motion_net is not None:
            from .motion import motion_term
            first = out
            term, minfo = motion_term(motion_net, self.graph.nodes, self.prev_trans, first["node_translations"],
                                      self.warpfield.tsdf.get_visible_nodes())
            out, log2, _ = icp_track(self._assoc, self.solver, self.graph.nodes, self.graph.edges,
                                     self.graph.edges_weights, self.source_pcd, nrm, self.point_anchors,
                                     self.anchor_weight, None, depth, self._intr4(), first["node_rotations"],
                                     first["node_translations"], term, 1, depth_filter=depth_filter, robust=robust,
                                     **pho, **occ, **assoc)
            log = log + log2
            if "rigid" in first:
                out["rigid"] = first["rigid"]
        R, T = out["node_rotations"], out["node_translations"]
        self.prev_rot, self.prev_trans = R.clone(), T.clone()
        nodes_t = torch.as_tensor(self.graph.nodes, device=self.device)
        self.warpfield.set_node_transforms(R, T)
        warped = self.warpfield.deform_device(self.source_pcd, self.point_anchors, self.anchor_weight)
        res = {"warped_verts": warped, "node_rotations": R.cpu().numpy().astype(np.float64),
               "node_translations": T.cpu(), "deformed_nodes_to_target": nodes_t + T,
               "convergence_info": out["convergence_info"], "valid_solve": out["valid_solve"],
               "source_frame_id": None, "target_frame_id": target_frame_data.get("id"), "assoc": log}
        if "rigid" in out:
            res["rigid"] = out["rigid"]
        if "render" in out:
            res["render"] = out["render"]
        if minfo is not None:
            res["motion"] = minfo
        return res


def run_arap(solver, reduced_graph_dict, model_data, graph, log=None):
    """run_model.py:448-627 (Model.run_arap): initialise every invalid node from its highest-weight already-
    updated graph neighbour (queue ordered by the number of valid neighbours, descending), then the device
    DeformNet.arap GN (GaussNewtonSolver.arap) on all nodes. Returns node_rotations (N,3,3), node_translations
    (N,3), deformed_nodes_to_target (N,3), source/target frame ids, convergence_info, valid_solve.
    np.argsort's tie order in the reference is unspecified (quicksort); here it is stable."""
    for k in ("node_rotations", "node_translations", "deformed_nodes_to_target"):
        assert np.asarray(model_data[k]).dtype == np.float32, f"model_data[{k}] not np.float32"
    valid = np.asarray(reduced_graph_dict["valid_nodes_mask"]).reshape(-1).astype(bool)
    N = len(graph.nodes)
    assert len(valid) == N, f"Valid nodes not from current graph. Expected:{N} got:{len(valid)}"
    R = np.tile(np.eye(3, dtype=np.float32)[None], (N, 1, 1))
    T = np.zeros((N, 3), np.float32)
    R[valid] = model_data["node_rotations"]
    T[valid] = model_data["node_translations"]
    invalid = np.where(~valid)[0]
    n_edges = np.sum(graph.edges != -1, axis=1)
    vis = [np.sum(valid[graph.edges[n, :n_edges[n]]]) for n in invalid]
    queue = list(invalid[np.argsort(vis, kind="stable")[::-1]])
    g = np.asarray(reduced_graph_dict["all_nodes_at_source"], np.float32)
    updated = valid.copy()
    while updated.sum() < N:
        L = len(queue)
        for i in range(L):
            ind = queue[i]
            nb = graph.edges[ind, :n_edges[ind]]
            cand = np.where(updated[nb])[0]
            if len(cand) == 0:
                queue.append(ind)
                continue
            c = graph.edges[ind, cand[np.argmax(graph.edges_weights[ind, cand])]]
            R[ind] = R[c]
            T[ind] = R[ind] @ (g[ind] - g[c]) + T[c] + g[c] - g[ind]
            updated[ind] = True
        del queue[:L]
        if len(queue) == 0 or len(queue) == L:
            break
    res = solver.arap(g, reduced_graph_dict["valid_nodes_at_source"], model_data["deformed_nodes_to_target"], valid, g,
                      graph.edges, graph.edges_weights, graph.clusters, R, T)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    out["deformed_nodes_to_target"] = g + out["node_translations"]
    out["source_frame_id"] = model_data.get("source_frame_id")
    out["target_frame_id"] = model_data.get("target_frame_id")
    return out
