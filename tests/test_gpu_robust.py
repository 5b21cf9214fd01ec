"""GPU: per-match weights and Huber / Tukey robust data rows in the Gauss-Newton solve (ofx_gn_set_robust,
torch.ops.ofx.gn_set_robust, GaussNewtonSolver.optimize(match_weights=, robust=), the robust= keyword of the trackers)
against the dense f64 restatement tests/robust_ref.py (pinned on the CPU by test_robust_ref.py). Problem:
gn_params_ref.base() — gn_small.npz, 257 nodes, 600 matches.

* off is the solver as it was: optimize(match_weights=None, robust=None), and optimize after a robust solve on the same
  handle, are bitwise a fresh solver's plain solve (k_terms<false>, the kernel without the feature);
* weights of all 1.0 through k_terms<true> are bitwise the plain solve (w·1.0 and r·1.0 are exact);
* duplication identity on the device (precond="direct"): weights from {0, 1, 2} against the device's own solve of the
  problem with each match repeated w² times, within 1e-9; both within 1e-5 of the reference;
* reference parity at the project's bars (transforms 1e-5, loss logs 1e-6 relative): the outlier fixture under Tukey,
  Huber and weights x Tukey through the exact solve, the cluster PCG and the forced Schwarz PCG; once with flow rows;
* edges: all weights zero; a node whose every match is Tukey-rejected; -1-padded edge rows with weights; M = 597 (600 and
  597 are no multiples of 64: the block tail); a NaN weight gives valid_solve == 0;
* prefetch: a setup prefetched with weights is used and bitwise the inline path's; changing only the robust setting
  between prepare and solve is a miss, and the result is still right;
* the operator equals the direct C-ABI call bitwise and passes opcheck;
* tracker: icp_track(robust=None) is the loop as it was, icp_track(robust="tukey") is associate + optimize(robust="tukey")
  by hand, iteration by iteration, both bitwise.
"""
import ctypes

import numpy as np
import pytest
import torch

import gn_params_ref as P
import robust_ref as RR

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
TOL = 1e-5
LOSS_RTOL = 1e-6


def _solver(tag="default", max_matches=1000, **kw):
    from occlusionfusion_amd import GaussNewtonSolver
    prm = P.params(tag)
    prm.update(kw)
    return GaussNewtonSolver(P.base()["nodes"].shape[0], max_matches, **prm)


def _rob(robust):
    return None if robust is None else {"kernel": robust[0], "scale": robust[1]}


def _run(name, precond, solver=None):
    """The named case of robust_ref on the device -> (solver, result)."""
    tag, args, kw, mw, robust = RR.problem(name)
    s = solver if solver is not None else _solver(tag, precond=precond)
    return s, s.optimize(*args, **kw, match_weights=mw, robust=_rob(robust))


def _same(a, b):
    return (torch.equal(a["node_rotations"], b["node_rotations"]) and
            torch.equal(a["node_translations"], b["node_translations"]) and torch.equal(a["_loss"], b["_loss"]) and
            torch.equal(a["_status"], b["_status"]))


def _check(out, ref, what):
    """test_gpu_gn_params._check_solve's bars."""
    ci, rc = out["convergence_info"], ref["convergence_info"]
    dr = np.abs(out["node_rotations"].cpu().numpy() - ref["node_rotations"]).max()
    dt = np.abs(out["node_translations"].cpu().numpy() - ref["node_translations"]).max()
    print(f"robust {what}: max|R - R_ref| = {dr:.3e}, max|t - t_ref| = {dt:.3e}, GN steps {ci['gn_iterations']}, "
          f"PCG iterations {ci['pcg_iterations']}, capped steps {ci['pcg_capped_steps']}")
    assert out["valid_solve"] == ref["valid_solve"] == 1, what
    assert ci["gn_iterations"] == len(rc["total"]), (what, ci["gn_iterations"], len(rc["total"]))
    for k in ("total", "data", "arap", "motion"):
        np.testing.assert_allclose(ci[k], rc[k], rtol=LOSS_RTOL, atol=0, err_msg=f"{what} {k}")
    assert ci["pcg_capped_steps"] == 0, what
    assert dr <= TOL and dt <= TOL, (what, dr, dt)


def _posed():
    d = P.base()
    return dict(prev_rot=d["R0"], prev_trans=d["t0"])


# ---------------------------------------------------------------------------- off, and weights of one
@pytest.mark.parametrize("precond", ["direct", "cluster"])
def test_off_is_the_solver_as_it_was(cuda, precond):
    args, kw = P.inputs("default"), _posed()
    fresh = _solver(precond=precond).optimize(*args, **kw)                       # no new keyword at all
    assert _same(_solver(precond=precond).optimize(*args, **kw, match_weights=None, robust=None), fresh)
    s = _solver(precond=precond)
    rob = s.optimize(*args, **kw, match_weights=RR.weights012(), robust="tukey")
    assert rob["valid_solve"] == 1 and not torch.equal(rob["node_translations"], fresh["node_translations"])
    assert s._rob == [True]
    assert _same(s.optimize(*args, **kw), fresh)                                 # the setting does not carry over
    assert s._rob == [False]
    assert _same(s.optimize(*args, **kw, robust={"kernel": "none"}), fresh)


@pytest.mark.parametrize("precond", ["direct", "schwarz"])
def test_unit_weights_through_the_robust_kernel_are_the_plain_solve(cuda, precond):
    args, kw = P.inputs("mixed", True), dict(_posed(), **P.flow_targets("mixed"))
    fresh = _solver("mixed", precond=precond).optimize(*args, **kw)
    s = _solver("mixed", precond=precond)
    ones = s.optimize(*args, **kw, match_weights=np.ones(600, np.float32))
    assert s._rob == [True] and _same(ones, fresh)
    # a weight's sign is immaterial: every product that reaches A, b and the loss holds two factors of it
    neg = s.optimize(*args, **kw, match_weights=-np.ones(600, np.float32))
    assert torch.equal(neg["node_rotations"], fresh["node_rotations"])
    assert torch.equal(neg["node_translations"], fresh["node_translations"]) and torch.equal(neg["_loss"], fresh["_loss"])


# ---------------------------------------------------------------------------- duplication identity
def test_duplication_identity_on_the_device(cuda):
    w = RR.weights012()
    rows = RR.duplicated(w)
    ref = RR.solve("w012")
    s = _solver(precond="direct", max_matches=2400)
    a = s.optimize(*P.inputs("default"), **_posed(), match_weights=w)
    b = _solver(precond="direct", max_matches=2400).optimize(*RR.with_matches(P.inputs("default"), rows), **_posed())
    dr = (a["node_rotations"].double() - b["node_rotations"].double()).abs().max().item()
    dt = (a["node_translations"].double() - b["node_translations"].double()).abs().max().item()
    print(f"duplication identity on the device: max|dR| {dr:.3e} max|dt| {dt:.3e}, {len(rows)} duplicated matches")
    _check(a, ref, "weights {0,1,2} direct")
    _check(b, ref, "duplicated matches direct")
    assert dr <= 1e-9 and dt <= 1e-9, (dr, dt)
    np.testing.assert_allclose(a["_loss"].cpu().numpy(), b["_loss"].cpu().numpy(), rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------- reference parity
@pytest.mark.parametrize("precond", ["direct", "cluster", "schwarz"])
@pytest.mark.parametrize("name", ["tukey", "huber", "w_tukey"])
def test_outlier_fixture_matches_the_reference(cuda, name, precond):
    s, out = _run(name, precond)
    assert s.solver_info()["direct"] == (1 if precond == "direct" else 0)
    if precond != "direct":
        assert s.precond_info()["schwarz"] == (1 if precond == "schwarz" else 0)
    _check(out, RR.solve(name), f"{name} {precond}")
    if name == "tukey" and precond == "direct":        # and it does what it is for, on the device too
        clean, plain = RR.solve("clean"), RR.solve("plain")
        err = np.abs(out["node_translations"].cpu().numpy() - clean["node_translations"]).max()
        assert err <= RR.max_t_err(plain, clean) / 5


@pytest.mark.parametrize("precond", ["direct", "cluster"])
def test_flow_rows_are_scaled_too(cuda, precond):
    s, out = _run("flow_tukey", precond)
    _check(out, RR.solve("flow_tukey"), f"flow_1e-3 tukey {precond}")
    assert RR.max_t_err(RR.solve("flow_tukey"), RR.solve("tukey")) > 1e-5        # the flow rows matter here


# ---------------------------------------------------------------------------- edges
@pytest.mark.parametrize("name,precond", [("zeros", "direct"), ("zeros", "cluster"), ("isolated", "cluster"),
                                          ("isolated", "schwarz"), ("pad_w_huber", "schwarz"),
                                          ("pad_w_huber", "direct"), ("m597", "direct"), ("m597", "cluster")])
def test_edge_cases_match_the_reference(cuda, name, precond):
    s, out = _run(name, precond)
    _check(out, RR.solve(name), f"{name} {precond}")
    if name == "zeros":
        assert all(v == 0.0 for v in out["convergence_info"]["data"])            # only ARAP, motion and LM remain


def test_nan_weight_invalidates_the_solve(cuda):
    w = np.ones(600, np.float32)
    w[123] = np.nan
    s = _solver(precond="direct")
    out = s.optimize(*P.inputs("default"), **_posed(), match_weights=w)
    assert out["valid_solve"] == 0
    assert _same(s.optimize(*P.inputs("default"), **_posed()), _solver(precond="direct").optimize(
        *P.inputs("default"), **_posed()))                                        # and the handle recovers


# ---------------------------------------------------------------------------- prefetch
def _device_problem(cuda, pad):
    """test_gpu_gn_params._device_problem: the problem as device tensors in the solver's own dtypes (a converted tensor
    would be a new problem to the prefetch)."""
    d = P.base()

    def dev(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.astype(np.int32 if x.dtype.kind == "i" else np.float32)).to(cuda)
    pb = dict(graph_nodes=dev(d["nodes"]), graph_edges=dev(d["edges_pad" if pad else "edges"]),
              graph_edges_weights=dev(d["ew_a"]), target_node_position=dev(d["tpos"]), node_confidence=dev(d["conf"]),
              source_points=dev(d["src"]), anchors=dev(d["anchors"]), weights=dev(d["weights"]),
              target_points=dev(RR.outlier_targets()[0]))
    return pb, dict(intrinsics=d["intr"], prev_rot=dev(d["R0"]), prev_trans=dev(d["t0"]))


def test_prefetch_carries_the_weights_and_the_setting(cuda):
    pa, kw = _device_problem(cuda, False)
    pb, _ = _device_problem(cuda, True)
    wa = torch.from_numpy(np.ascontiguousarray(RR.weights012())).to(cuda)
    wb = torch.flip(wa, [0]).contiguous()
    tuk, hub = "tukey", {"kernel": "huber", "scale": 0.005}
    fresh_b = {k: _solver().optimize(**pb, **kw, match_weights=wb, robust=r) for k, r in (("tukey", tuk), ("huber", hub))}
    fresh_plain = _solver().optimize(**pb, **kw)
    assert not _same(fresh_b["tukey"], fresh_b["huber"]) and not _same(fresh_b["tukey"], fresh_plain)
    s = _solver()
    s.optimize(**pa, **kw, match_weights=wa, robust=tuk, prefetch=dict(pb, match_weights=wb, robust=tuk))
    assert _same(s.optimize(**pb, **kw, match_weights=wb, robust=tuk), fresh_b["tukey"])
    s.drain()
    assert s.prefetch_stats() == (1, 0)
    # only the robust setting changes between prepare and solve: a miss, and still the right result
    s.optimize(**pa, **kw, match_weights=wa, robust=tuk, prefetch=dict(pb, match_weights=wb, robust=tuk))
    assert _same(s.optimize(**pb, **kw, match_weights=wb, robust=hub), fresh_b["huber"])
    s.drain()
    assert s.prefetch_stats() == (1, 1)
    # prepared with a setting, solved without: a miss too, and the plain result
    s.optimize(**pa, **kw, prefetch=dict(pb, match_weights=wb, robust=tuk))
    assert _same(s.optimize(**pb, **kw), fresh_plain)
    s.drain()
    assert s.prefetch_stats() == (1, 2)
    # prepared without, solved without: used, as before the feature
    s.optimize(**pa, **kw, prefetch=pb)
    assert _same(s.optimize(**pb, **kw), fresh_plain)
    s.drain()
    torch.cuda.synchronize()
    assert s.prefetch_stats() == (2, 2)


# ---------------------------------------------------------------------------- operator
def test_op_equals_c_abi_and_opcheck(cuda):
    from occlusionfusion_amd import _lib
    tag, args, kw, mw, robust = RR.problem("w_tukey")
    w = torch.from_numpy(np.ascontiguousarray(mw)).to(cuda)
    outs = []
    for how in ("op", "abi"):
        s = _solver(precond="direct")
        a, N, M = s._problem(*args, None, None, None, None)
        fp, ip = s._plist()
        h, st = s._slots[0]
        if how == "op":
            torch.ops.ofx.gn_set_robust(st, h.value, w, 2, 0.03)
        else:
            rb = _lib.GnRobust(_lib.ptr(w), 2, 0, 0.03)
            _lib.call("ofx_gn_set_robust", h, ctypes.byref(rb))
        outs.append(torch.ops.ofx.gn_solve(st, h.value, *a, fp, ip))
    for x, y in zip(*outs):
        assert x.dtype == y.dtype and torch.equal(x, y)
    ref = _solver(precond="direct").optimize(*args, **kw, match_weights=w, robust="tukey")
    assert torch.equal(outs[0][0], ref["node_rotations"]) and torch.equal(outs[0][3], ref["_loss"])
    _check(ref, RR.solve("w_tukey"), "op / C ABI / optimize, w_tukey direct")
    s = _solver()
    h, st = s._slots[0]
    torch.library.opcheck(torch.ops.ofx.gn_set_robust.default, (st, h.value, w, 2, 0.03))
    torch.library.opcheck(torch.ops.ofx.gn_set_robust.default, (st, h.value, None, 0, 0.0))
    with pytest.raises(_lib.OfxError, match="unknown robust kernel"):
        torch.ops.ofx.gn_set_robust(st, h.value, w, 7, 0.03)
    with pytest.raises(_lib.OfxError, match="scale"):
        torch.ops.ofx.gn_set_robust(st, h.value, None, 1, 0.0)


# ---------------------------------------------------------------------------- tracker plumbing
def test_icp_track_forwards_robust_to_every_solve(cuda):
    """Config 1's scene (199 nodes, 320x224), frame 0 -> 20 from the identity, 2000 canonical points, two ICP iterations,
    the exact solve."""
    from occlusionfusion_amd import GaussNewtonSolver
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.association import ProjectiveAssociator, icp_track, pack_transforms
    from occlusionfusion_amd.image_proc import backproject_depth_device
    seq = S.config_sequence(1, device=cuda)
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    cp = seq.canonical_points
    pts = torch.from_numpy(np.ascontiguousarray(
        cp[np.sort(np.random.default_rng(5).choice(cp.shape[0], 2000, replace=False))], np.float32)).to(cuda)
    nodes = torch.from_numpy(np.ascontiguousarray(seq.nodes, np.float32)).to(cuda)
    a, w, v = torch.ops.ofx.skin_points(pts, nodes, float(seq.node_coverage), 4)
    pts, a, w = pts[v], a[v].contiguous(), w[v].contiguous()
    depth = torch.from_numpy(np.ascontiguousarray(seq.frame(20)[5], np.float32)).to(cuda)
    MM, iters = 2000, 2
    graph = (seq.nodes, seq.edges, seq.edge_weights)

    def tracked(**kw):
        assoc, solver = ProjectiveAssociator(pts.shape[0], cuda), GaussNewtonSolver(len(seq.nodes), MM, precond="direct")
        out, log, _ = icp_track(assoc, solver, *graph, pts, None, a, w, None, depth, intr, icp_iters=iters,
                                max_matches=MM, **kw)
        return out

    def by_hand(**kw):
        assoc, solver = ProjectiveAssociator(pts.shape[0], cuda), GaussNewtonSolver(len(seq.nodes), MM, precond="direct")
        vm = backproject_depth_device(depth, *intr)
        rot = trans = out = None
        for _ in range(iters):
            m = assoc.associate(pts, None, a, w, None, pack_transforms(seq.nodes, rot, trans, cuda), vm, intr,
                                max_matches=MM)
            assert m["emitted"] >= 100
            out = solver.optimize(*graph, None, None, m["src"], m["anchors"], m["weights"], m["tgt"], intr,
                                  prev_rot=rot, prev_trans=trans, **kw)
            rot, trans = out["node_rotations"], out["node_translations"]
        return out

    plain = by_hand()
    assert plain["valid_solve"] == 1
    assert _same(tracked(), plain) and _same(tracked(robust=None), plain)
    tukey = by_hand(robust="tukey")
    assert tukey["valid_solve"] == 1 and not torch.equal(tukey["node_translations"], plain["node_translations"])
    assert _same(tracked(robust="tukey"), tukey)
    assert _same(tracked(robust={"kernel": "tukey", "scale": 0.03}), tukey)
