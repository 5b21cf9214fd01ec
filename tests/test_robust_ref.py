"""CPU: the reference of the per-match weights and robust data rows (tests/robust_ref.py) pinned without a device.

* no weights, no kernel: robust_ref.gn_optimize is fo.gn_optimize bit for bit (0.0 difference) from the pose() start;
* duplication identity: weights from {0, 1, 2} equal fo.gn_optimize on the problem with each match repeated w² times
  (transforms within 1e-12 — measured 1.5e-15 when this was written — and loss logs to 1e-12 relative): the weight's
  meaning is tied to the existing oracle and not to the restatement;
* outlier fixture (identity start, 10 % of the targets displaced by N(0, 0.05 m)): under Tukey 0.03 and under Huber 0.005
  the worst node translation error against the clean solve is at most 1/5 of the plain solve's; Tukey rejects some
  matches (s = 0) and down-weights others (0 < s < 1), Huber rejects none;
* the Tukey boundary: s = 0 at u = 1 exactly, > 0 just below, continuous there;
* the fixtures the GPU tests rely on are what they claim (the isolated node's matches are all rejected at every step).
"""
import numpy as np

import gn_params_ref as P
import robust_ref as RR
from oracle import fusion_oracle as fo


def test_without_weights_and_kernel_it_is_the_oracle_bit_for_bit():
    R, t = P.pose()
    for tag, pad in (("default", False), ("mixed", True)):
        a = RR.gn_optimize(*P.inputs(tag, pad), prev_rot=R, prev_trans=t, **P.flow_targets(tag), **P.params(tag))
        b = fo.gn_optimize(*P.inputs(tag, pad), prev_rot=R, prev_trans=t, **P.flow_targets(tag), **P.params(tag))
        assert np.abs(a["node_rotations"] - b["node_rotations"]).max() == 0.0
        assert np.abs(a["node_translations"] - b["node_translations"]).max() == 0.0
        assert a["valid_solve"] == b["valid_solve"] == 1
        for k in ("total", "data", "arap", "motion"):
            assert a["convergence_info"][k] == b["convergence_info"][k]
        assert all((s == 1.0).all() for s in a["scales"])


def test_duplication_identity_ties_the_weight_to_the_oracle():
    w = RR.weights012()
    assert set(np.unique(w).tolist()) == {0.0, 1.0, 2.0} and min(np.bincount(w.astype(int))) > 150
    rows = RR.duplicated(w)
    assert len(rows) == int((w ** 2).sum()) and (np.bincount(rows, minlength=600) == w ** 2).all()
    R, t = P.pose()
    a = RR.solve("w012")
    b = fo.gn_optimize(*RR.with_matches(P.inputs("default"), rows), prev_rot=R, prev_trans=t)
    dr = np.abs(a["node_rotations"] - b["node_rotations"]).max()
    dt = np.abs(a["node_translations"] - b["node_translations"]).max()
    print(f"duplication identity: max|dR| {dr:.3g} max|dt| {dt:.3g}")
    assert a["valid_solve"] == b["valid_solve"] == 1
    assert dr <= 1e-12 and dt <= 1e-12
    ca, cb = a["convergence_info"], b["convergence_info"]
    assert len(ca["total"]) == len(cb["total"]) == 10
    for k in ("total", "data", "arap", "motion"):
        np.testing.assert_allclose(ca[k], cb[k], rtol=1e-12, atol=0)
    plain = P.oracle("default", sparse=False)
    assert RR.max_t_err(a, plain) > 1e-4                        # the weights matter on this problem


def test_outlier_fixture_and_the_two_kernels():
    tgt, mask = RR.outlier_targets()
    d = P.base()
    assert mask.sum() == 60 and (tgt[~mask] == d["tgt"][~mask]).all()
    disp = np.linalg.norm(tgt[mask].astype(np.float64) - d["tgt"][mask], axis=1)
    assert 0.03 < disp.mean() < 0.15
    clean, plain, tukey, huber = (RR.solve(k) for k in ("clean", "plain", "tukey", "huber"))
    assert all(x["valid_solve"] == 1 and len(x["convergence_info"]["total"]) == 10 for x in (clean, plain, tukey, huber))
    e_plain, e_tukey, e_huber = (RR.max_t_err(x, clean) for x in (plain, tukey, huber))
    print(f"worst node translation error vs the clean solve: plain {e_plain:.3g} m, Tukey 0.03 {e_tukey:.3g} m "
          f"(1/{e_plain / e_tukey:.1f}), Huber 0.005 {e_huber:.3g} m (1/{e_plain / e_huber:.1f})")
    assert e_plain > 5e-3
    assert e_tukey <= e_plain / 5 and e_huber <= e_plain / 5
    s_t, s_h = tukey["scales"][-1], huber["scales"][-1]
    assert (s_t == 0.0).any() and ((s_t > 0.0) & (s_t < 1.0)).any()
    assert (s_t[~mask] > 0.0).mean() > 0.95 and (s_t[mask] == 0.0).mean() > 0.5   # it is the outliers that are rejected
    assert (s_h > 0.0).all() and (s_h < 1.0).any() and (s_h <= 1.0).all()
    assert all((s == 1.0).all() for s in plain["scales"])
    # the scale follows the estimate: IRLS, not a weight fixed at the start
    assert not np.array_equal(tukey["scales"][0], tukey["scales"][-1])


def test_tukey_boundary():
    c = 0.03
    c2 = c * c
    assert RR.row_scale(c2, "tukey", c) == 0.0                       # u = 1 exactly
    below = np.nextafter(c2, 0.0)
    s = float(RR.row_scale(below, "tukey", c))
    assert 0.0 < s < 1e-15                                           # just below: positive, and continuous at the boundary
    assert RR.row_scale(2 * c2, "tukey", c) == 0.0 and RR.row_scale(0.0, "tukey", c) == 1.0
    u = np.linspace(0.0, 1.0, 11)
    np.testing.assert_allclose(RR.row_scale(u * c2, "tukey", c) ** 2, (1 - u) ** 2, atol=1e-15)   # the biweight's root
    # Huber: 1 up to delta, then sqrt(delta / e), continuous; never 0
    dl = 0.005
    e = np.array([0.0, dl / 2, dl, np.nextafter(dl, 1.0), 4 * dl, 1.0])
    sh = RR.row_scale(e ** 2, "huber", dl)
    np.testing.assert_allclose(sh, [1, 1, 1, 1, 0.5, np.sqrt(dl)], rtol=1e-12)
    assert (sh > 0).all()
    assert np.isnan(RR.row_scale(np.nan, "huber", dl)) and RR.row_scale(np.nan, "tukey", c) == 0.0


def test_gpu_fixtures_are_what_they_claim():
    d = P.base()
    tgt, mask = RR.isolated_targets()
    assert 0 < mask.sum() < 40 and (d["anchors"][mask] == RR.ISOLATED).any(1).all()
    iso = RR.solve("isolated")
    assert iso["valid_solve"] == 1 and len(iso["convergence_info"]["total"]) == 10
    assert all((s[mask] == 0.0).all() for s in iso["scales"])         # no data row ever touches the node
    assert all((s[~mask] > 0.0).mean() > 0.9 for s in iso["scales"])
    zeros = RR.solve("zeros")
    assert zeros["valid_solve"] == 1 and all(v == 0.0 for v in zeros["convergence_info"]["data"])
    both, tuk = RR.solve("w_tukey"), RR.solve("tukey")
    assert RR.max_t_err(both, tuk) > 1e-4                              # weights and kernel together differ from either
    for name in RR.CASES:
        r = RR.solve(name)
        assert r["valid_solve"] == 1 and len(r["convergence_info"]["total"]) == 10, name
    assert RR.problem("m597")[1][5].shape[0] == 597 and 597 % 64 != 0 and 600 % 64 != 0
    assert RR.DEFAULTS == {"huber": 0.005, "tukey": 0.03}
