"""CPU: the oracle side of the Gauss-Newton parameter tests (gn_params_ref.py, test_gpu_gn_params.py).

* fo.gn_system with lambda_flow / use_edge_weighting / target_px / target_py is the linearisation gn_optimize solves: one
  solve of its A x = b from the start pose, applied as R <- exp(x_rot) R, t += x_t, reproduces gn_optimize(num_iter=1)
  to 1e-12, its loss is convergence_info["total"][0], its include_data / include_reg shares sum to the whole, and
  without the new arguments it is what it was.
* Two conditions on the inputs (not on any code under test): every set that the iterative solvers are held to has
  cond(A) <= 1e5 over its ten GN steps, and for every set the dense and the sparse f64 oracle (two summation orders)
  agree to 1e-9 on R and t at the level the set is used. An input change that breaks either changes the input.
* flow_ref (the reference's lambda_flow = 5, cond 2.5e8): a Cholesky and an LU solve of the oracle's A agree to 1e-7 in
  the update, which is what lets the GPU's exact solve be asserted on it for one step.
"""
import numpy as np
import pytest

import gn_params_ref as P
from oracle import fusion_oracle as fo

KAPPA_MAX = 1e5


def _apply(x, R, t):
    N = R.shape[0]
    return fo.angle_axis_to_rotation_matrix(x[:3 * N].reshape(N, 3)) @ R, t + x[3 * N:].reshape(N, 3)


def _lm(tag, gn_iter):
    lm = P.params(tag).get("lm_factor", fo.GN_DEFAULTS["lm_factor"])
    for k in range(gn_iter + 1):
        if k % 3 == 2:
            lm /= 2
    return lm


def test_problem_builder_shapes_and_ranges():
    d = P.base()
    N, NB = d["edges"].shape
    assert (N, NB, d["src"].shape[0]) == (257, 8, 600)
    assert np.all(d["edge_weights"] == np.float32(1 / 8))           # why the golden file cannot exercise edge weighting
    assert len(np.unique(d["anchors"])) == 176
    a, b = NB * d["ew_a"].astype(np.float64), NB * d["ew_b"].astype(np.float64)
    assert 0.5 <= a.min() and a.max() <= 2.0 and a.std() > 0.3
    assert b.min() < 1e-4 and b.max() > 5.0
    np.testing.assert_allclose(d["ew_b"].sum(1), 1.0, rtol=1e-6)
    ep = d["edges_pad"]
    kept = np.ones(N, bool)
    kept[::3] = False
    kept[P.PAD_BARE] = False
    assert (ep[P.PAD_BARE] == -1).all() and (ep[::3, -2:] == -1).all() and (ep[kept] == d["edges"][kept]).all()
    assert (ep[0, :-2] == d["edges"][0, :-2]).all() and (d["edges"] >= 0).all()
    assert (ep == P.PAD_BARE).any()                                # the bare node is still somebody's neighbour
    R, t = P.pose()
    ang = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert 0.1 < ang.mean() < 0.6 and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5   # (kornia's θ + 1e-6)
    assert d["R0"].dtype == d["t0"].dtype == d["tpx"].dtype == np.float32
    fx, fy, cx, cy = d["intr"]
    assert np.abs(d["tpx"] - (fx * d["tgt"][:, 0] / d["tgt"][:, 2] + cx)).max() < 2.0


def test_gn_system_defaults_ignore_the_new_arguments():
    """No lambda_flow, no use_edge_weighting: targets and edge weights are not read, the partial losses sum to loss2."""
    d = P.base()
    i = P.inputs("default")
    R, t = P.pose()
    a = fo.gn_system(i[0], i[1], *i[3:], R, t)
    b = fo.gn_system(i[0], i[1], *i[3:], R, t, graph_edges_weights=d["ew_b"], target_px=d["tpx"], target_py=d["tpy"])
    assert a["A"].tobytes() == b["A"].tobytes() and a["b"].tobytes() == b["b"].tobytes() and a["loss2"] == b["loss2"]
    assert a["loss2_data"] + a["loss2_arap"] + a["loss2_motion"] == pytest.approx(a["loss2"], rel=1e-14)
    assert min(a["loss2_data"], a["loss2_arap"], a["loss2_motion"]) > 0


@pytest.mark.parametrize("pad", [False, True], ids=["full", "padded"])
@pytest.mark.parametrize("tag", P.DIRECT_SETS)
def test_gn_system_is_gn_optimizes_linearisation(tag, pad):
    from scipy.linalg import lu_factor, lu_solve
    R, t = P.pose()
    sysd = P.system(tag, pad)
    prm = P.params(tag)
    prm["num_iter"] = 1
    ref = fo.gn_optimize(*P.inputs(tag, pad), prev_rot=R, prev_trans=t, **P.flow_targets(tag), **prm)
    assert ref["valid_solve"] == 1
    R1, t1 = _apply(lu_solve(lu_factor(sysd["A"]), sysd["b"]), R, t)
    assert np.abs(R1 - ref["node_rotations"]).max() <= 1e-12
    assert np.abs(t1 - ref["node_translations"]).max() <= 1e-12
    ci = ref["convergence_info"]
    assert sysd["loss"] == pytest.approx(ci["total"][0], rel=1e-13)
    for k in ("data", "arap", "motion"):
        assert np.sqrt(sysd["loss2_" + k]) == pytest.approx(ci[k][0], rel=1e-13)
    # the shares of a match shard: data rows alone + regularisers alone (which carry the damping) = the whole
    sd, sr = P.system(tag, pad, include_reg=False), P.system(tag, pad, include_data=False)
    lm = _lm(tag, 0)
    scale = np.abs(sysd["A"]).max()
    assert np.abs(sd["A"] + sr["A"] - lm * np.eye(len(sysd["b"])) - sysd["A"]).max() <= 1e-14 * scale
    assert np.abs(sd["b"] + sr["b"] - sysd["b"]).max() <= 1e-14 * max(np.abs(sd["b"]).max(), np.abs(sr["b"]).max())
    assert sd["loss2"] + sr["loss2"] == pytest.approx(sysd["loss2"], rel=1e-14)
    assert (sd["loss2_data"], sd["loss2_arap"], sd["loss2_motion"]) == (sysd["loss2_data"], 0.0, 0.0)
    assert (sr["loss2_data"], sr["loss2_arap"], sr["loss2_motion"]) == (0.0, sysd["loss2_arap"], sysd["loss2_motion"])


def test_gn_system_sets_differ_from_the_default():
    """Every set changes the system it is meant to change (none is a no-op on this problem)."""
    ref = P.system("default")
    for tag in P.DIRECT_SETS[1:]:
        s = P.system(tag)
        assert np.abs(s["A"] - ref["A"]).max() > 1e-3 * np.abs(ref["A"]).max(), tag
    assert np.abs(P.system("default", pad=True)["A"] - ref["A"]).max() > 1e-3 * np.abs(ref["A"]).max()


@pytest.mark.slow
@pytest.mark.parametrize("tag", P.ALL_SETS)
def test_condition_number_of_the_iterative_sets(tag):
    """Condition on the inputs: max cond(A) over the ten GN steps of the f64 oracle <= 1e5 for every set an iterative
    solver is held to (measured: default 4.8e3, ew_mild 7.3e3, ew_builder 2.8e4, flow_1e-4 1.5e4, flow_1e-3 6.7e4,
    mixed 3.9e4, no_motion 2.6e4, depth4 2.4e4)."""
    from scipy.linalg import lu_factor, lu_solve
    i = P.inputs(tag)
    prm = P.params(tag)
    prm.pop("lm_factor", None)
    R, t = P.pose()
    kappa = 0.0
    for it in range(10):
        s = fo.gn_system(i[0], i[1], *i[3:], R, t, lm_factor=_lm(tag, it), graph_edges_weights=i[2],
                         **P.flow_targets(tag), **prm)
        ev = np.linalg.eigvalsh(s["A"])
        assert ev[0] > 0
        kappa = max(kappa, ev[-1] / ev[0])
        R, t = _apply(lu_solve(lu_factor(s["A"]), s["b"]), R, t)
    ref = P.oracle(tag)                       # the loop above is the oracle's own iteration
    assert np.abs(R - ref["node_rotations"]).max() < 1e-9 and np.abs(t - ref["node_translations"]).max() < 1e-9
    print(f"{tag}: max cond(A) over 10 GN steps {kappa:.3g}")
    assert kappa <= KAPPA_MAX, (tag, kappa)


@pytest.mark.slow
@pytest.mark.parametrize("tag", P.DIRECT_SETS)
def test_dense_and_sparse_oracle_agree(tag):
    """Condition on the inputs: the two f64 summation orders land within 1e-9 of each other, so a 1e-5 comparison of
    the device against either is a comparison against the mathematics and not against one rounding sequence."""
    a, b = P.oracle(tag, sparse=False), P.oracle(tag, sparse=True)
    ca, cb = a["convergence_info"], b["convergence_info"]
    assert a["valid_solve"] == b["valid_solve"] == 1 and len(ca["total"]) == len(cb["total"])
    dr = np.abs(a["node_rotations"] - b["node_rotations"]).max()
    dt = np.abs(a["node_translations"] - b["node_translations"]).max()
    print(f"{tag}: dense vs sparse oracle max|dR| {dr:.3g} max|dt| {dt:.3g}, accepted steps {len(ca['total'])}")
    assert dr <= 1e-9 and dt <= 1e-9, (tag, dr, dt)
    np.testing.assert_allclose(ca["total"], cb["total"], rtol=1e-12)


def test_unequal_focal_lengths_problem():
    """The camera with fy = 1.25 fx (every golden one has fx = fy): gn_system is still gn_optimize's linearisation, the
    system differs from the golden camera's in the flow sets and in "default" (the quirk's mfx / mfy terms), and the
    flow_1e-3 solve the GPU test compares with runs its ten steps in both oracles alike."""
    from scipy.linalg import lu_factor, lu_solve
    assert P.ANISO[0] == P.base()["intr"][0] and P.ANISO[1] == 1.25 * P.ANISO[0]
    assert all(float(np.float32(v)) == v for v in P.ANISO)
    R, t = P.pose()
    for tag in ("default", "flow_ref"):
        sysd = P.system(tag, True, intr=P.ANISO)
        assert np.abs(sysd["A"] - P.system(tag, True)["A"]).max() > 1e-3 * np.abs(sysd["A"]).max()
        prm = P.params(tag)
        prm["num_iter"] = 1
        ref = fo.gn_optimize(*P.inputs(tag, True, P.ANISO), prev_rot=R, prev_trans=t, **P.flow_targets(tag), **prm)
        R1, t1 = _apply(lu_solve(lu_factor(sysd["A"]), sysd["b"]), R, t)
        assert np.abs(R1 - ref["node_rotations"]).max() <= 1e-12
        assert np.abs(t1 - ref["node_translations"]).max() <= 1e-12
    a, b = P.oracle("flow_1e-3", True, False, P.ANISO), P.oracle("flow_1e-3", True, True, P.ANISO)
    assert a["valid_solve"] == b["valid_solve"] == 1
    assert len(a["convergence_info"]["total"]) == len(b["convergence_info"]["total"]) == 10
    assert np.abs(a["node_rotations"] - b["node_rotations"]).max() <= 1e-9
    assert np.abs(a["node_translations"] - b["node_translations"]).max() <= 1e-9


def test_oracle_step_counts_of_the_flow_sets():
    """flow_1 under the default stop rule accepts exactly one step (the second step's loss rises by more than
    stop_loss_diff); flow_ref is a one-step solve; every other set runs its ten steps."""
    for tag in P.DIRECT_SETS:
        n = len(P.oracle(tag)["convergence_info"]["total"])
        assert n == (1 if tag in ("flow_1", "flow_ref") else 10), (tag, n)
    prm = P.params("flow_1")
    prm["num_iter"] = 2
    prm["stop_loss_diff"] = 1e9
    R, t = P.pose()
    two = fo.gn_optimize_sparse(*P.inputs("flow_1"), prev_rot=R, prev_trans=t, **P.flow_targets("flow_1"), **prm)
    tot = two["convergence_info"]["total"]
    assert tot[1] - tot[0] > fo.GN_DEFAULTS["stop_loss_diff"]


@pytest.mark.parametrize("pad", [False, True], ids=["full", "padded"])
def test_flow_ref_cholesky_and_lu_updates_agree(pad):
    from scipy.linalg import cho_factor, cho_solve, lu_factor, lu_solve
    s = P.system("flow_ref", pad)
    x_lu = lu_solve(lu_factor(s["A"]), s["b"])
    x_ch = cho_solve(cho_factor(s["A"]), s["b"])
    d = np.abs(x_lu - x_ch).max()
    print(f"flow_ref ({'padded' if pad else 'full'}): max |x_lu - x_chol| = {d:.3g}, max |x| = {np.abs(x_lu).max():.3g}")
    assert d <= 1e-7
