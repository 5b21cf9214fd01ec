"""GPU: the one-launch Schwarz iteration's contribution dot over four lanes per inverse row (k_as_iter, k_as_w0).

Each lane of a row's quad runs two of k_as_apply's four accumulation chains over one half of the row, in their order, on
8-byte halves of the slab's words (stored in the 32-bit order 0, 2, 1, 3), and the quad sums them by DPP: the iterates
must stay bitwise those of the two-launch form (k_pcg_iter<.., kAS> + k_as_apply) — here on gn_1k, whose cluster count
is no multiple of 8 (padding workgroups in the XCD-contiguous mapping), and on gn_2k_hole, whose rim subdomains have
short rings (fewer than 24 rows: dot lanes past the subdomain's rows) — and a solve must repeat bit for bit.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("gn_1k.npz", "gn_2k_hole.npz")
_cache = {}


def _load(name):
    if name in _cache:
        return _cache[name]
    g = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    d = {k: g[k] for k in g.files}
    if "frames" not in d:   # (gn_1k: one frame, unprefixed)
        for k in ("src", "tgt", "tpos", "conf", "anchors", "weights"):
            d[f"f0_{k}"] = d[k]
    _cache[name] = d
    return d


def _problem(g, cuda):
    f = {k: torch.from_numpy(np.ascontiguousarray(g[f"f0_{k}"])).to(cuda)
         for k in ("src", "tgt", "tpos", "conf", "anchors", "weights")}
    return dict(graph_nodes=torch.from_numpy(g["nodes"]).to(cuda), graph_edges=torch.from_numpy(g["edges"]).to(cuda),
                graph_edges_weights=torch.from_numpy(g["edge_weights"]).to(cuda), target_node_position=f["tpos"],
                node_confidence=f["conf"], source_points=f["src"], anchors=f["anchors"].int(), weights=f["weights"],
                target_points=f["tgt"])


def _solve(s, g, pb):
    """One solve: (rotations, translations, status, per-step PCG counts), all on the host."""
    out = s.optimize(**pb, intrinsics=tuple(float(v) for v in g["intr"]))
    torch.cuda.synchronize()
    return (out["node_rotations"].cpu().numpy().copy(), out["node_translations"].cpu().numpy().copy(),
            out["_status"].cpu().numpy().copy(), s.stats()[:, 0].copy())


def _same(a, b, what):
    for x, y, n in zip(a, b, ("rotations", "translations", "status", "PCG counts per step")):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, n)


def test_one_launch_is_bitwise_the_two_launch_form_on_short_subdomains(cuda, monkeypatch):
    """gn_1k (a cluster count that is no multiple of 8: padding workgroups in the XCD-contiguous mapping) and gn_2k_hole
    (short rings at the hole's rim): transforms, status and per-step PCG counts equal bit for bit, one launch per
    iteration, and at least one fixture has a subdomain of fewer than 24 rows."""
    from occlusionfusion_amd import GaussNewtonSolver
    monkeypatch.setenv("OFX_PRECOND", "as")
    short = []
    for name in FIXTURES:
        g = _load(name)
        pb = _problem(g, cuda)
        N = g["nodes"].shape[0]
        monkeypatch.setenv("OFX_AS_ONE", "0")
        s2 = GaussNewtonSolver(N, 10000)
        two = _solve(s2, g, pb)
        assert s2.precond_info()["launches_per_iteration"] == 2
        monkeypatch.setenv("OFX_AS_ONE", "1")
        s1 = GaussNewtonSolver(N, 10000)
        one = _solve(s1, g, pb)
        info = s1.precond_info()
        assert info["schwarz"] == 1 and info["launches_per_iteration"] == 1, info
        assert two[2][0] == 1 and two[3].sum() > 0, name   # (a valid solve that iterated)
        _same(two, one, name)
        print(f"{name}: clusters {info['clusters']}, subdomain rows {info['subdomain_rows']}, PCG iterations "
              f"{int(one[3].sum())}")
        short.append(info["subdomain_rows"] < 24 * info["clusters"])
    assert any(short), "no fixture has a subdomain of fewer than 24 rows"


def test_one_launch_solve_repeats_bitwise(cuda, monkeypatch):
    from occlusionfusion_amd import GaussNewtonSolver
    monkeypatch.delenv("OFX_PRECOND", raising=False)
    monkeypatch.setenv("OFX_AS_ONE", "1")
    g = _load("gn_2k_hole.npz")
    pb = _problem(g, cuda)
    s = GaussNewtonSolver(g["nodes"].shape[0], 10000, precond="schwarz")
    a = _solve(s, g, pb)
    b = _solve(s, g, pb)
    assert s.precond_info()["launches_per_iteration"] == 1
    _same(a, b, "gn_2k_hole twice on one handle")
