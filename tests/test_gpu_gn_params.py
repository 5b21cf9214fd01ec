"""GPU: every ofx_gn_params weight and switch against the f64 oracle (problem and sets: gn_params_ref.py; the oracle
side and the conditions on the inputs: test_gn_params_ref.py).

The rest of the suite solves at lambda_flow = 0, use_edge_weighting = 0 and the default lambdas only. Here:

* assembly (gn_setup + gn_linearize against fo.gn_system, rtol 1e-9 / atol 1e-12 as test_gn_assembly_matches_dense_system):
  the flow residual and Jacobian entries, the target_px / target_py upload, NB·w_e read through the row permutation,
  -1-padded edge rows, non-default lambdas, from the identity pose and from a non-identity one (at the identity
  R_k(x - g_k) cannot tell R from its transpose), the three loss partials one by one, the LM schedule at gn_iter = 2;
* the same linearisation and one exact solve under a camera with fy = 1.25 fx (every golden camera has fx = fy);
* match shards summing to the whole; target_px = None as explicit zeros;
* the exact solve, the cluster PCG and the forced Schwarz PCG: valid_solve, accepted steps, per-step loss logs (rtol
  1e-6) and transforms (1e-5) against the oracle; flow_1e-2 and flow_1 under the exact solve only, flow_ref (the
  reference's lambda_flow = 5, cond 2.5e8) for one exact step;
* arap() with edge weighting; a parameter change on a live handle, with and without a prefetched setup.
"""
import numpy as np
import pytest
import torch

import gn_params_ref as P
from oracle import fusion_oracle as fo

# (the shared problem's arrays are read-only; the solver only uploads them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]
TOL = 1e-5
LOSS_RTOL = 1e-6
PADS = pytest.mark.parametrize("pad", [False, True], ids=["full", "padded"])


def _solver(tag, **kw):
    from occlusionfusion_amd import GaussNewtonSolver
    prm = P.params(tag)
    prm.update(kw)
    return GaussNewtonSolver(P.base()["nodes"].shape[0], 1000, **prm)


def _start(identity):
    d = P.base()
    return (None, None) if identity else (d["R0"], d["t0"])


def _setup(s, tag, pad, identity, targets=None, intr=None):
    """gn_setup of the set's problem on s -> (problem size, block count, rows, row order)."""
    ft = P.flow_targets(tag) if targets is None else targets
    args, N, M = s._problem(*P.inputs(tag, pad, intr), ft.get("target_px"), ft.get("target_py"), *_start(identity))
    fp, ip = s._plist()
    nnz, rows = (int(v) for v in torch.ops.ofx.gn_setup(s._state, s._h.value, *args, fp, ip))
    assert rows == s.info()[4]
    perm = s.row_order()
    assert len(perm) == rows and rows % 8 == 0 and sorted(perm[perm >= 0].tolist()) == list(range(N))
    return N, M, nnz, rows, perm


def _linearize(s, cuda, nnz, rows, gn_iter, m0, m1, add_reg):
    A = torch.empty(nnz * 36, dtype=torch.float64, device=cuda)
    rhs = torch.empty(6 * rows + 4, dtype=torch.float64, device=cuda)
    torch.ops.ofx.gn_linearize(s._state, s._h.value, gn_iter, m0, m1, add_reg, A, rhs)
    torch.cuda.synchronize()
    return A.cpu().numpy(), rhs.cpu().numpy()


def _check_system(A, rb, perm, rows, N, sysd, lm, what):
    """Block-sparse A / rhs of the device against the dense oracle system (node-major order), as
    test_gn_assembly_matches_dense_system does, plus the three loss partials one by one."""
    p = fo.node_major_perm(N)
    Ad = sysd["A"][np.ix_(p, p)]
    bd = sysd["b"][p]
    Ab = A.reshape(-1, 6, 6)
    blocks_dense = Ad.reshape(N, 6, N, 6).transpose(0, 2, 1, 3)
    nzmask = np.abs(blocks_dense).sum((2, 3)) > 0
    n_pad = int((perm < 0).sum())
    assert Ab.shape[0] >= nzmask.sum() + n_pad, what
    pad_diag = np.tile((lm * np.eye(6)).reshape(-1), n_pad)
    np.testing.assert_allclose(np.sort(Ab.reshape(-1)), np.sort(np.concatenate(
        [blocks_dense[nzmask].reshape(-1), pad_diag, np.zeros((Ab.shape[0] - nzmask.sum() - n_pad) * 36)])),
        rtol=1e-9, atol=1e-12, err_msg=what)
    real = perm >= 0
    np.testing.assert_allclose(rb[:6 * rows].reshape(rows, 6)[real], bd.reshape(N, 6)[perm[real]], rtol=1e-9, atol=1e-12,
                               err_msg=what)
    assert not rb[:6 * rows].reshape(rows, 6)[~real].any(), what
    for k, name in enumerate(("data", "arap", "motion")):
        np.testing.assert_allclose(rb[6 * rows + k], sysd["loss2_" + name], rtol=1e-9, atol=0, err_msg=f"{what} {name}")
    assert rb[6 * rows + 3] == 0.0, what      # the non-finite flag


def _lm(tag, gn_iter):
    lm = P.params(tag).get("lm_factor", fo.GN_DEFAULTS["lm_factor"])
    for k in range(gn_iter + 1):
        if k % 3 == 2:
            lm /= 2
    return lm


# ---------------------------------------------------------------------------- 1. assembly
@PADS
@pytest.mark.parametrize("identity", [True, False], ids=["identity", "posed"])
@pytest.mark.parametrize("tag", list(P.SETS))
def test_assembly_matches_dense_system(cuda, tag, identity, pad):
    s = _solver(tag)
    N, M, nnz, rows, perm = _setup(s, tag, pad, identity)
    A, rb = _linearize(s, cuda, nnz, rows, 0, 0, M, True)
    _check_system(A, rb, perm, rows, N, P.system(tag, pad, identity), _lm(tag, 0), f"{tag} identity={identity} pad={pad}")


def test_assembly_lm_schedule_halves_at_the_third_step(cuda):
    s = _solver("mixed")
    N, M, nnz, rows, perm = _setup(s, "mixed", True, False)
    A, rb = _linearize(s, cuda, nnz, rows, 2, 0, M, True)
    assert _lm("mixed", 2) == 0.5e-5
    _check_system(A, rb, perm, rows, N, P.system("mixed", True, False, gn_iter=2), 0.5e-5, "mixed gn_iter=2")
    A0, _ = _linearize(s, cuda, nnz, rows, 0, 0, M, True)
    assert np.abs(A0 - A).max() == pytest.approx(0.5e-5, rel=1e-6)     # the damping is all that differs


@pytest.mark.parametrize("tag", ["default", "flow_1e-3", "mixed", "flow_ref"])
def test_assembly_tells_fx_from_fy(cuda, tag):
    """Every golden camera has fx = fy: fx/z for fy/z in J[10], or any other exchange of the two, changes nothing under
    it (and in "default" the mfx / mfy rotation terms of the reference's precedence quirk stay). The same linearisation
    under a camera with fy = 1.25 fx and another cy."""
    s = _solver(tag)
    N, M, nnz, rows, perm = _setup(s, tag, True, False, intr=P.ANISO)
    A, rb = _linearize(s, cuda, nnz, rows, 0, 0, M, True)
    sysd = P.system(tag, True, False, intr=P.ANISO)
    assert np.abs(sysd["A"] - P.system(tag, True, False)["A"]).max() > 1e-3 * np.abs(sysd["A"]).max()
    _check_system(A, rb, perm, rows, N, sysd, _lm(tag, 0), f"{tag} fy = 1.25 fx")


def test_exact_solve_with_unequal_focal_lengths(cuda):
    d = P.base()
    tag = "flow_1e-3"
    out = _solver(tag, precond="direct").optimize(*P.inputs(tag, True, P.ANISO), prev_rot=d["R0"], prev_trans=d["t0"],
                                                  **P.flow_targets(tag))
    ref = P.oracle(tag, True, True, P.ANISO)
    assert len(ref["convergence_info"]["total"]) == 10
    _check_solve(out, ref, f"{tag} padded direct, fy = 1.25 fx")


# ---------------------------------------------------------------------------- 2. shards
@pytest.mark.parametrize("tag", ["flow_1e-3", "mixed"])
def test_match_shards_sum_to_the_whole(cuda, tag):
    s = _solver(tag)
    N, M, nnz, rows, perm = _setup(s, tag, True, False)
    whole_A, whole_b = _linearize(s, cuda, nnz, rows, 0, 0, M, True)
    cuts = [0, M // 3 + 1, 2 * M // 3 - 1, M]
    parts = [_linearize(s, cuda, nnz, rows, 0, cuts[r], cuts[r + 1], r == 0) for r in range(3)]
    sum_A, sum_b = sum(p[0] for p in parts), sum(p[1] for p in parts)
    assert np.abs(sum_A - whole_A).max() <= 1e-12 * np.abs(whole_A).max()
    assert np.abs(sum_b - whole_b).max() <= 1e-12 * np.abs(whole_b).max()
    lm = _lm(tag, 0)
    _check_system(sum_A, sum_b, perm, rows, N, P.system(tag, True, False), lm, f"{tag} shard sum")
    reg_A, reg_b = _linearize(s, cuda, nnz, rows, 0, 0, 0, True)       # the share of a rank without matches
    _check_system(reg_A, reg_b, perm, rows, N, P.system(tag, True, False, include_data=False), lm, f"{tag} no data")
    dat_A, dat_b = _linearize(s, cuda, nnz, rows, 0, 0, M, False)      # data rows alone carry no damping
    sysd = P.system(tag, True, False, include_reg=False)
    sysd["A"] = sysd["A"] - lm * np.eye(6 * N)
    _check_system(dat_A, dat_b, perm, rows, N, sysd, 0.0, f"{tag} no regularisers")


# ---------------------------------------------------------------------------- 3. target_px = None
def test_missing_flow_targets_are_zeros(cuda):
    """lambda_flow > 0 without target_px / target_py: the upload's NULL default is the oracle's, zeros — the same bits as
    explicit zero arrays, in the assembled system and through the exact solve."""
    tag = "flow_1e-4"
    M = P.base()["src"].shape[0]
    zeros = dict(target_px=np.zeros(M, np.float32), target_py=np.zeros(M, np.float32))
    got = []
    for targets in ({}, zeros):
        s = _solver(tag)
        N, M, nnz, rows, perm = _setup(s, tag, False, False, targets)
        got.append(_linearize(s, cuda, nnz, rows, 0, 0, M, True) + (perm,))
    assert np.array_equal(got[0][2], got[1][2])
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    i = P.inputs(tag)
    R, t = P.pose()
    sysd = fo.gn_system(i[0], i[1], *i[3:], R, t, graph_edges_weights=i[2], **P.params(tag))
    _check_system(got[0][0], got[0][1], got[0][2], len(got[0][2]), N, sysd, _lm(tag, 0), "flow targets None")
    d = P.base()
    outs = [_solver(tag, precond="direct").optimize(*i, prev_rot=d["R0"], prev_trans=d["t0"], **targets)
            for targets in ({}, zeros)]
    assert torch.equal(outs[0]["node_rotations"], outs[1]["node_rotations"])
    assert torch.equal(outs[0]["node_translations"], outs[1]["node_translations"])
    assert torch.equal(outs[0]["_loss"], outs[1]["_loss"])
    ref = fo.gn_optimize_sparse(*i, prev_rot=R, prev_trans=t, **P.params(tag))
    _check_solve(outs[0], ref, "flow targets None, direct")


# ---------------------------------------------------------------------------- 4./5. solves
def _check_solve(out, ref, what):
    ci, rc = out["convergence_info"], ref["convergence_info"]
    dr = np.abs(out["node_rotations"].cpu().numpy() - ref["node_rotations"]).max()
    dt = np.abs(out["node_translations"].cpu().numpy() - ref["node_translations"]).max()
    print(f"GN params {what}: max|R - R_ref| = {dr:.3e}, max|t - t_ref| = {dt:.3e}, GN steps {ci['gn_iterations']}, "
          f"PCG iterations {ci['pcg_iterations']}, capped steps {ci['pcg_capped_steps']}")
    assert out["valid_solve"] == ref["valid_solve"] == 1, what
    assert ci["gn_iterations"] == len(rc["total"]), (what, ci["gn_iterations"], len(rc["total"]))
    for k in ("total", "data", "arap", "motion"):
        np.testing.assert_allclose(ci[k], rc[k], rtol=LOSS_RTOL, atol=0, err_msg=f"{what} {k}")
    assert ci["pcg_capped_steps"] == 0, what
    assert dr <= TOL and dt <= TOL, (what, dr, dt)
    return max(dr, dt)


def _solve(tag, pad, precond):
    d = P.base()
    s = _solver(tag, precond=precond)
    args = P.inputs(tag, pad)
    kw = dict(prev_rot=d["R0"], prev_trans=d["t0"], **P.flow_targets(tag))
    return s, s.optimize(*args, **kw), (lambda: s.optimize(*args, **kw))


@PADS
@pytest.mark.parametrize("tag", P.DIRECT_SETS)
def test_exact_solve_matches_oracle(cuda, tag, pad):
    """precond="direct". flow_1 runs the default stop rule: the oracle accepts one step and stops at the second, whose
    loss rises by more than stop_loss_diff, and so must the device; flow_ref is one step (num_iter = 1)."""
    s, out, _ = _solve(tag, pad, "direct")
    ref = P.oracle(tag, pad)
    if tag in ("flow_1", "flow_ref"):
        assert len(ref["convergence_info"]["total"]) == 1
    _check_solve(out, ref, f"{tag} {'padded' if pad else 'full'} direct")
    assert s.solver_info()["direct"] == 1 and out["convergence_info"]["pcg_iterations"] == 0


@PADS
@pytest.mark.parametrize("precond", ["cluster", "schwarz"])
@pytest.mark.parametrize("tag", P.ALL_SETS)
def test_pcg_solve_matches_oracle(cuda, tag, precond, pad):
    s, out, again = _solve(tag, pad, precond)
    assert s.precond_info()["schwarz"] == (1 if precond == "schwarz" else 0)
    assert s.solver_info()["direct"] == 0 and out["convergence_info"]["pcg_iterations"] > 0
    _check_solve(out, P.oracle(tag, pad), f"{tag} {'padded' if pad else 'full'} {precond}")
    b = again()
    assert torch.equal(out["node_rotations"], b["node_rotations"])
    assert torch.equal(out["node_translations"], b["node_translations"])
    assert torch.equal(out["_loss"], b["_loss"])


# ---------------------------------------------------------------------------- 6. arap
def test_arap_with_edge_weighting_matches_dense_oracle(cuda):
    """GaussNewtonSolver.arap with use_edge_weighting and non-uniform weights (uniform(0.5, 2)/8 per entry): the
    "nonrigid" case of test_gn_arap_matches_dense_oracle at its tolerances. lambda_flow stays 0 (no parity is claimed
    for arap otherwise: DESIGN §6)."""
    from occlusionfusion_amd import GaussNewtonSolver
    from occlusionfusion_amd import synthetic as S
    rng = np.random.default_rng(4)
    pts = rng.normal(size=(3000, 3))
    pts = 0.3 * pts / np.linalg.norm(pts, axis=1, keepdims=True) + np.array([0, 0, 1.4])
    nodes = S.sample_nodes(pts.astype(np.float32), 0.08, 5)
    e, _ = S.euclidean_edges(nodes, 8)
    N = len(nodes)
    valid = np.ones(N, bool)
    valid[rng.choice(N, N // 3, replace=False)] = False
    R = fo.angle_axis_to_rotation_matrix(rng.normal(0, 0.03, (N, 3))).astype(np.float32)
    t = rng.normal(0, 0.01, (N, 3)).astype(np.float32)
    tgt = (nodes[valid] + t[valid] + rng.normal(0, 0.002, (valid.sum(), 3))).astype(np.float32)
    w = (rng.uniform(0.5, 2.0, e.shape) / e.shape[1]).astype(np.float32)
    ref = fo.gn_arap(nodes, nodes[valid], tgt, valid, nodes, e, w, R, t, use_edge_weighting=True)
    plain = fo.gn_arap(nodes, nodes[valid], tgt, valid, nodes, e, w, R, t)
    assert np.abs(ref["node_translations"] - plain["node_translations"]).max() > 1e-4   # the weights matter here
    s = GaussNewtonSolver(N, 16, use_edge_weighting=True)
    out = s.arap(nodes, nodes[valid], tgt, valid, nodes, e, w, None, R, t)
    assert out["valid_solve"] == ref["valid_solve"] == 1
    Rg, tg = out["node_rotations"].cpu().numpy(), out["node_translations"].cpu().numpy()
    np.testing.assert_array_equal(Rg[valid], R[valid])
    np.testing.assert_array_equal(tg[valid], t[valid])
    dr, dt = np.abs(Rg - ref["node_rotations"]).max(), np.abs(tg - ref["node_translations"]).max()
    print(f"arap with edge weighting: max|dR| {dr:.3e} max|dt| {dt:.3e}")
    assert dr < 1e-5 and dt < 1e-5
    ci = out["convergence_info"]
    assert len(ci["total"]) == len(ref["convergence_info"]["total"])
    np.testing.assert_allclose(ci["total"], ref["convergence_info"]["total"], rtol=3e-4)
    np.testing.assert_allclose(out["deformed_nodes_to_target"].cpu().numpy(), ref["deformed_nodes_to_target"], atol=1e-7)


# ---------------------------------------------------------------------------- 7. live handle
def _device_problem(cuda, pad):
    """The problem as device tensors that every set can share: edge weights "a" and the flow targets are given to every
    solve (a set without edge weighting / flow rows must not read them)."""
    d = P.base()

    def dev(x):   # in the solver's own dtypes, so that no call converts (a converted tensor is a new problem)
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.astype(np.int32 if x.dtype.kind == "i" else np.float32)).to(cuda)
    pb = dict(graph_nodes=dev(d["nodes"]), graph_edges=dev(d["edges_pad" if pad else "edges"]),
              graph_edges_weights=dev(d["ew_a"]), target_node_position=dev(d["tpos"]), node_confidence=dev(d["conf"]),
              source_points=dev(d["src"]), anchors=dev(d["anchors"]), weights=dev(d["weights"]),
              target_points=dev(d["tgt"]), target_px=dev(d["tpx"]), target_py=dev(d["tpy"]))
    return pb, dict(intrinsics=d["intr"], prev_rot=dev(d["R0"]), prev_trans=dev(d["t0"]))


def _same(a, b):
    return (torch.equal(a["node_rotations"], b["node_rotations"]) and
            torch.equal(a["node_translations"], b["node_translations"]) and torch.equal(a["_loss"], b["_loss"]) and
            torch.equal(a["_status"], b["_status"]))


def test_parameter_change_on_a_live_handle(cuda):
    """One solver: default, then s.params <- mixed on the same device tensors (the setup must be redone: the edge
    weights are read again, the coefficients change), then default again; each equals a fresh solver's bit for bit, and
    the oracle within the bar (default here = the "default" set: edge weights and flow targets present but unused)."""
    pb, kw = _device_problem(cuda, False)
    fresh = {tag: _solver(tag).optimize(**pb, **kw) for tag in ("default", "mixed")}
    for tag in ("default", "mixed"):
        _check_solve(fresh[tag], P.oracle(tag, False), f"{tag} device tensors")
    assert not torch.equal(fresh["default"]["node_translations"], fresh["mixed"]["node_translations"])
    s = _solver("default")
    for tag in ("default", "mixed", "default", "default", "mixed"):
        s.params.update(fo.GN_DEFAULTS)
        s.params.update(P.params(tag))
        assert _same(s.optimize(**pb, **kw), fresh[tag]), tag


def test_parameter_change_with_a_prefetched_setup(cuda):
    """A setup prefetched under the old parameters is not the next solve's: it is discarded (a miss) and redone; one
    prefetched under the same parameters is used. Either way the result is a fresh solver's bit for bit."""
    pa, kw = _device_problem(cuda, False)
    pb, _ = _device_problem(cuda, True)
    fresh_b = {tag: _solver(tag).optimize(**pb, **kw) for tag in ("default", "mixed")}
    _check_solve(fresh_b["mixed"], P.oracle("mixed", True), "mixed padded device tensors")
    s = _solver("default")
    s.optimize(**pa, **kw, prefetch=pb)              # B set up ahead under the default parameters
    s.params.update(P.params("mixed"))
    assert _same(s.optimize(**pb, **kw), fresh_b["mixed"])
    s.drain()
    assert s.prefetch_stats() == (0, 1)
    s.optimize(**pa, **kw, prefetch=pb)              # B set up ahead under mixed
    assert _same(s.optimize(**pb, **kw), fresh_b["mixed"])
    assert s.prefetch_stats() == (1, 1)
    s.params.update(fo.GN_DEFAULTS)
    s.optimize(**pa, **kw, prefetch=pb)              # and under the default parameters again
    assert _same(s.optimize(**pb, **kw), fresh_b["default"])
    s.drain()
    torch.cuda.synchronize()
    assert s.prefetch_stats() == (2, 1)
