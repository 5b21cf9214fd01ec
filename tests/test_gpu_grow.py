"""GPU: growing the graph from the sampled model (ofx_grow_nodes, torch.ops.ofx.grow_nodes, NodeGrower,
WarpField.grow_from_volume).

* the kernels equal the numpy restatement (tests/grow_ref.py) bit for bit — nodes, R, T, edge rows, edge weights and
  count — on 5 000 random points of a 0.5 m x 0.5 m plane patch with nodes over one third of it (about 3 000 candidates:
  several 1 024-candidate chunks), with planted rows: an exact duplicate, a pair at exactly the spacing, a pair one ulp
  under it, a NaN point, out-of-range anchors, invalid padding; max_new = 64 falls inside a chunk;
* zero candidates, no rows, refused arguments, operator == C ABI, opcheck, determinism;
* WarpField.grow_from_volume: the sphere scene of tests/test_gpu_surface.py is fully skinned after one round, and a plane
  first seen over its left third is covered by growth where the fixed graph never passes its rim;
* FusionPipeline.track_step(model="volume", grow_every=1) on config 1 — bitwise the loop without growth when nothing is
  uncovered, growing and solving at a quarter of the coverage — and Registration.grow_from_volume.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grow_ref as gr  # noqa: E402
from occlusionfusion_amd import _lib, ops  # noqa: E402,F401  (ops registers torch.ops.ofx.*)
from occlusionfusion_amd._lib import byref, call, ptr, stream_ptr  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
COV = 0.02
K_E = 8
N_PLANTED, N_PLANE, N_PAD = 11, 5000, 100


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene_arrays():
    """Model rows: the planted rows (far off the patch, one metre apart), the plane points, invalid padding. Nodes on a
    coverage grid over the left third, each with its own rotation and translation; skins drawn at random among them."""
    rng = np.random.default_rng(11)
    s = F32(COV)
    under = np.nextafter(s, F32(0))
    planted = np.array([[1, 2, 0.5], [1, 2, 0.5],                    # 0, 1: duplicate
                        [0, 3, 0.5], [s, 3, 0.5],                    # 2, 3: exactly the spacing apart: both kept
                        [0, 4, 0.5], [under, 4, 0.5],                # 4, 5: one ulp under: the second dropped
                        [np.nan, 5, 0.5], [1, 5, 0.5], [1, 6, 0.5],  # 6 NaN, 7 anchor == n_nodes, 8 anchor -1
                        [2, 6, 0.5], [3, 6, 0.5]], F32)              # 9 anchor 2^31 - 1, 10 invalid row
    plane = np.concatenate([rng.uniform(0, 0.5, (N_PLANE, 2)), np.full((N_PLANE, 1), 0.5)], 1).astype(F32)
    pts = np.concatenate([planted, plane, np.zeros((N_PAD, 3), F32)], 0)
    x, y = np.meshgrid(np.arange(0, 0.5 / 3, COV), np.arange(0, 0.5 + 1e-9, COV), indexing="ij")
    nodes = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, 0.5)], 1).astype(F32)
    n = nodes.shape[0]
    M = pts.shape[0]
    a = rng.integers(0, n, (M, 4)).astype(np.int32)
    a[7, 2], a[8, 0], a[9, 3] = n, -1, 2 ** 31 - 1
    w = rng.uniform(0.05, 1, (M, 4)).astype(F32)
    w = (w / (w.sum(1, keepdims=True) + F32(1e-6))).astype(F32)
    valid = np.ones(M, np.uint8)
    valid[10] = 0
    valid[N_PLANTED + N_PLANE:] = 0
    R = np.stack([_rot(rng.normal(size=3), rng.uniform(0, 0.6)) for _ in range(n)]).astype(F32)
    R[0] = _rot((1, 0, 0), 3.1)                                       # the other Shepperd branches
    R[1] = _rot((0, 1, 0), 3.0)
    R[2] = _rot((0, 0, 1), 2.9)
    T = rng.normal(0, 0.01, (n, 3)).astype(F32)
    E = rng.integers(0, n, (n, K_E)).astype(np.int32)
    W = rng.uniform(0, 1, (n, K_E)).astype(F32)
    return dict(pts=pts, a=a, w=w, valid=valid, nodes=nodes, R=R, T=T, E=E, W=W)


@pytest.fixture(scope="module")
def scene(cuda):
    s = scene_arrays()
    s["dev"] = {k: torch.from_numpy(s[k]).to(cuda) for k in ("pts", "a", "w", "valid")}
    s["ref"] = {}
    return s


def _ref(s, max_new):
    """The restatement for a cap, computed once and shared (never modified)."""
    if max_new not in s["ref"]:
        s["ref"][max_new] = gr.grow_nodes(s["pts"], s["a"], s["w"], s["valid"], s["nodes"], s["R"], s["T"], s["E"], s["W"],
                                          COV, 2 * COV, COV, max_new)
    return s["ref"][max_new]


class _Handle:
    def __init__(self, max_points, max_new):
        self.h = _lib.c_void_p()
        call("ofx_grow_create", max_points, max_new, byref(self.h))

    def __del__(self):
        _lib.lib.ofx_grow_destroy(self.h)


def _graph_buffers(s, max_new, dev, k_e=K_E, fill=-3.0):
    """The caller's arrays: n_nodes rows of the scene followed by max_new rows of garbage."""
    n = s["nodes"].shape[0]
    out = []
    for key, shape, dt in (("nodes", (3,), torch.float32), ("R", (3, 3), torch.float32), ("T", (3,), torch.float32),
                           ("E", (k_e,), torch.int32), ("W", (k_e,), torch.float32)):
        t = torch.full((n + max_new,) + shape, fill, dtype=dt, device=dev)
        src = torch.from_numpy(s[key]).to(dev)
        t[:n] = src if key not in ("E", "W") else src[:, :k_e] if k_e <= K_E else torch.nn.functional.pad(src, (0, k_e - K_E))
        out.append(t)
    out.append(torch.full((3,), -7, dtype=torch.int32, device=dev))
    return out


def _direct(handle, s, max_new, dev, n_points=None, min_dist=2 * COV, spacing=COV, status=False, k_e=K_E, n_nodes=None,
            null=None, pts=None):
    """ofx_grow_nodes through ctypes."""
    d = s["dev"]
    g = _graph_buffers(s, max_new, dev, k_e)
    p = d["pts"] if pts is None else pts
    M = p.shape[0] if n_points is None else n_points
    args = [handle.h, ptr(p), ptr(d["a"]), ptr(d["w"]), ptr(d["valid"]), M, ptr(g[0]),
            s["nodes"].shape[0] if n_nodes is None else n_nodes, ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]), k_e, COV,
            float(min_dist), float(spacing), max_new, ptr(g[5]), stream_ptr()]
    if null is not None:
        args[null] = None
    if status:
        return _lib.lib.ofx_grow_nodes(*args)
    call("ofx_grow_nodes", *args)
    return g


def _check(g, ref, s, max_new):
    n = s["nodes"].shape[0]
    count = g[5].cpu().numpy()
    assert list(count) == list(ref["count"])
    k = n + int(count[1])
    for t, key in zip(g[:5], ("nodes", "R", "T", "edges", "edge_weights")):
        x = t.cpu().numpy()
        assert x[:k].tobytes() == np.ascontiguousarray(ref[key]).tobytes(), key     # old rows kept, new rows bit for bit
        assert (x[k:] == -3).all(), key                                             # nothing past the selected rows


@pytest.mark.parametrize("max_new", [1024, 64])
def test_kernel_equals_restatement(scene, cuda, max_new):
    ref = _ref(scene, max_new)
    n_cand, n_sel, capped = (int(v) for v in ref["count"])
    assert 2500 < n_cand < 3500 and n_cand > 2 * 1024                 # several chunks
    if max_new == 64:
        assert (n_sel, capped) == (64, 1) and np.searchsorted(np.nonzero(
            gr.candidates(scene["pts"], scene["a"], scene["valid"], scene["nodes"], 2 * COV))[0], ref["rows"][-1]) < 1024
    else:
        assert capped == 0 and 200 < n_sel < 1024
        assert list(ref["rows"][:4]) == [0, 2, 3, 4]                   # the planted rows: duplicate and one-ulp pair cut
    _check(_direct(_Handle(6000, 1024), scene, max_new, cuda), ref, scene, max_new)


def test_cap_at_the_natural_count(scene, cuda):
    """max_new equal to what the loop selects anyway: nothing is left out, the flag stays 0."""
    n_sel = int(_ref(scene, 1024)["count"][1])
    g = _direct(_Handle(6000, 1024), scene, n_sel, cuda)
    assert g[5].cpu().tolist() == [int(_ref(scene, 1024)["count"][0]), n_sel, 0]
    g = _direct(_Handle(6000, 1024), scene, n_sel - 1, cuda)
    assert g[5].cpu().tolist()[1:] == [n_sel - 1, 1]


def test_empty_inputs(scene, cuda):
    h = _Handle(6000, 64)
    n = scene["nodes"].shape[0]
    M = scene["pts"].shape[0]
    near = torch.from_numpy(scene["nodes"][np.arange(M) % n] + F32(0.001)).to(cuda)   # every row within min_dist of a node
    for kw in (dict(pts=near), dict(n_points=0), dict(max_new=0)):
        g = _direct(h, scene, kw.pop("max_new", 64), cuda, **kw)
        assert g[5].cpu().tolist() == [0, 0, 0]
        assert all((t[n:] == -3).all() for t in g[:5])
    # a huge min_dist: no candidate either; a negative one: every valid row with a good skin is one
    assert _direct(h, scene, 64, cuda, min_dist=10.0)[5].cpu().tolist() == [0, 0, 0]
    c = _direct(h, scene, 64, cuda, min_dist=-1.0)[5].cpu().tolist()
    assert c[0] == N_PLANTED + N_PLANE - 5 and c[1:] == [64, 1]


def test_refused_arguments(scene, cuda):
    h, big = _Handle(6000, 64), _Handle(6000, 4096)
    assert _direct(h, scene, 64, cuda, status=True, k_e=9) == -1
    assert _direct(h, scene, 64, cuda, status=True, k_e=0) == -1
    assert _direct(big, scene, 4096, cuda, status=True, n_nodes=65534 - 4095) == -3
    assert b"65534" in _lib.lib.ofx_last_error()
    assert _direct(h, scene, 64, cuda, status=True, n_points=6001) == -1
    assert _direct(h, scene, 65, cuda, status=True) == -1                       # above the handle's max_new
    assert _direct(h, scene, 64, cuda, status=True, spacing=0.0) == -1
    assert _direct(h, scene, 64, cuda, status=True, spacing=-1.0) == -1
    assert _direct(h, scene, 64, cuda, status=True, min_dist=float("nan")) == -1
    assert _direct(h, scene, 64, cuda, status=True, n_nodes=0) == -1
    for null in (0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 17):
        assert _direct(h, scene, 64, cuda, status=True, null=null) == -1, null
    torch.cuda.synchronize()


def test_k_e_below_eight(scene, cuda):
    """Graphs with fewer edge columns: the same neighbours, cut at K_e, weights renormalised over the row."""
    ref = gr.grow_nodes(scene["pts"], scene["a"], scene["w"], scene["valid"], scene["nodes"], scene["R"], scene["T"],
                        scene["E"][:, :3], scene["W"][:, :3], COV, 2 * COV, COV, 64)
    g = _direct(_Handle(6000, 64), scene, 64, cuda, k_e=3)
    _check(g, ref, scene, 64)
    assert np.array_equal(ref["edges"][-64:], _ref(scene, 64)["edges"][-64:, :3])


def test_op_equals_c_abi_and_opcheck(scene, cuda):
    from occlusionfusion_amd.grow import NodeGrower
    d = scene["dev"]
    n = scene["nodes"].shape[0]
    ref = _direct(_Handle(6000, 1024), scene, 300, cuda)
    grower = NodeGrower(6000, 1024, cuda)
    g = _graph_buffers(scene, 300, cuda)
    count = grower.grow(d["pts"], d["a"], d["w"], d["valid"], g[0], n, g[1], g[2], g[3], g[4], COV, max_new=300, count=g[5])
    assert count is g[5]
    for x, y in zip(g, ref):
        assert x.dtype == y.dtype and torch.equal(x, y)
    with pytest.raises(ValueError, match="room"):
        grower.grow(d["pts"], d["a"], d["w"], d["valid"], g[0], n, g[1], g[2], g[3], g[4], COV, max_new=301)
    g = _graph_buffers(scene, 64, cuda)
    torch.library.opcheck(torch.ops.ofx.grow_nodes.default,
                          (grower._state, grower._h.value, d["pts"], d["a"], d["w"], d["valid"], g[0], n, g[1], g[2], g[3],
                           g[4], COV, 2 * COV, COV, 64, g[5]))


def test_determinism_across_calls_and_handles(scene, cuda):
    h1, h2 = _Handle(6000, 1024), _Handle(65536, 4096)
    a = _direct(h1, scene, 1024, cuda)
    _direct(h1, scene, 7, cuda, min_dist=0.0)                        # other work on the handle in between
    b = _direct(h1, scene, 1024, cuda)
    c = _direct(h2, scene, 1024, cuda)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---------------------------------------------------------------------------------------------- WarpField.grow_from_volume
def _sphere(cuda, coverage=None):
    """tests/test_gpu_surface.py's sphere scene with every weight 1 and moving nodes."""
    import test_gpu_surface as tg
    phi, _, nodes = tg.scene_arrays()
    vol, wf = tg._volume(cuda, phi, np.ones(tg.DIMS, F32), nodes, tg.COVERAGE if coverage is None else coverage)
    rng = np.random.default_rng(3)
    n = nodes.shape[0]
    R = np.stack([_rot(rng.normal(size=3), rng.uniform(0, 0.4)) for _ in range(n)]).astype(F32)
    wf.skin_tsdf_cache()
    wf.set_node_transforms(R, rng.normal(0, 0.005, (n, 3)).astype(F32))
    return tg, vol, wf


def test_grow_from_volume_on_the_sphere(cuda):
    """One round: the new rows are the restatement's on the sampled model, the graph, the transforms and the skin cache
    follow, and no surface voxel is left without a skin."""
    from occlusionfusion_amd import WarpField
    tg, vol, wf = _sphere(cuda)
    g = wf.graph
    n0 = wf.num_nodes
    before = wf.surface_points(1024, with_codes=True)
    m = {k: v.cpu().numpy().copy() for k, v in wf.surface_points(1024, sync=False).items() if k != "code"}
    R0, T0 = wf.R_t.cpu().numpy(), wf.T_t.cpu().numpy()
    ref = gr.grow_nodes(m["points"], m["anchors"], m["weights"], m["valid"], g.nodes, R0, T0, g.edges, g.edges_weights,
                        tg.COVERAGE, 2 * tg.COVERAGE, tg.COVERAGE, 256)
    n_list0 = wf._cache.n_list
    before_list = wf._cache.brick_list[:n_list0].cpu().numpy()
    res = wf.grow_from_volume(max_points=1024, incremental=True)
    assert before["histogram"][7] > 0 and res["added"] == int(ref["count"][1]) > 0
    assert (res["candidates"], res["capped"]) == (int(ref["count"][0]), 0)
    blist0 = before_list
    re, ap = gr.skin_grow_plan(tg.DIMS, tg.ORIGIN, tg.H_VOX, ref["nodes"], n0, tg.COVERAGE, 4, blist0)
    assert res["appended"] == wf._cache.n_list - n_list0 == len(ap) > 0 and res["reskinned"] == len(re) <= n_list0
    assert np.array_equal(wf._cache.brick_list.cpu().numpy(), np.concatenate([blist0, ap]))   # no longer ascending
    n = n0 + res["added"]
    assert wf.num_nodes == g.num_nodes == n and g.clusters.shape == (n, 1) and g.edges_distances.shape == (n, 8)
    assert wf.deformed_nodes.shape == (n, 3) and wf.packed_nodes().shape == (n, 16)
    for got, key in ((g.nodes, "nodes"), (wf.R_t.cpu().numpy(), "R"), (wf.T_t.cpu().numpy(), "T"), (g.edges, "edges"),
                     (g.edges_weights, "edge_weights"), (wf.nodes_t.cpu().numpy(), "nodes")):
        assert got.tobytes() == np.ascontiguousarray(ref[key]).tobytes(), key
    after = wf.surface_points(1024, with_codes=True)
    assert after["histogram"][7] == 0 and after["accepted"] > before["accepted"]
    # the cache is the one a fresh warp field builds on the grown graph
    fresh = WarpField(g, vol)
    vol.warpfield = wf
    for x, y in zip(wf.skin_tsdf(), fresh.skin_tsdf()):
        assert np.array_equal(x, y)
    # a fixed point within four rounds: no candidate is left
    for _ in range(3):
        res = wf.grow_from_volume(max_points=1024, incremental=True)
        if res["added"] == 0:
            break
    assert res == dict(added=0, candidates=0, capped=0, reskinned=0, appended=0)
    # the cap, and a full graph
    _, vol2, wf2 = _sphere(cuda)
    res = wf2.grow_from_volume(max_new=5, max_points=1024)
    assert (res["added"], res["capped"]) == (5, 1) and wf2.num_nodes == n0 + 5
    assert np.array_equal(wf2.graph.nodes, ref["nodes"][:n0 + 5])


SKIN_COVERAGE = 0.006   # the sphere scene at 0.02 touches every listed brick; at 0.006 one round re-skins 3 of 4 listed
#                          bricks and appends 1 (tests/grow_ref.py on the CPU, asserted below)


def _cache_by_brick(c):
    """brick id -> (anchors, weights, pal_n, pal_ids[:min(pal_n, 64)], local) of its slot, as bytes."""
    P = _lib.PALETTE
    bl = c.brick_list[:c.n_list].cpu().numpy()
    a, w = c.anchors.cpu().numpy().reshape(-1, 2048), c.weights.cpu().numpy().reshape(-1, 2048)
    pn, pi, lo = c.pal_n.cpu().numpy(), c.pal_ids.cpu().numpy().reshape(-1, P), c.local.cpu().numpy().reshape(-1, 2048)
    return {int(b): (a[s].tobytes(), w[s].tobytes(), int(pn[s]), pi[s, :min(int(pn[s]), P)].tobytes(), lo[s].tobytes())
            for s, b in enumerate(bl)}


def test_incremental_skin_update_equals_full_rebuild(cuda):
    """One growth round with the in-place update against a fresh warp field on the grown graph with a full build: the
    dense skin, and per brick the anchors, weights, palette ids, palette counts and local ranks at that brick's slot, bit
    for bit; fewer bricks skinned than listed, some appended; one warped integrate leaves bitwise equal volumes. And the
    same against incremental=False."""
    from occlusionfusion_amd import WarpField
    tg, vol, wf = _sphere(cuda, SKIN_COVERAGE)
    n0, c0 = wf.num_nodes, wf._cache
    n_list0 = c0.n_list
    blist0 = c0.brick_list[:n_list0].cpu().numpy()
    assert np.array_equal(blist0, gr.listed_bricks(tg.DIMS, tg.ORIGIN, tg.H_VOX, wf.graph.nodes, SKIN_COVERAGE, 4))
    res = wf.grow_from_volume(max_points=1024, incremental=True)
    re, ap = gr.skin_grow_plan(tg.DIMS, tg.ORIGIN, tg.H_VOX, wf.graph.nodes, n0, SKIN_COVERAGE, 4, blist0)
    print("skin update:", res, "of", n_list0, "listed bricks")
    assert res["added"] > 0 and res["appended"] == len(ap) > 0 and res["reskinned"] == len(re) < n_list0
    c = wf._cache
    assert c.n_list == n_list0 + len(ap)
    assert np.array_equal(c.brick_list.cpu().numpy(), np.concatenate([blist0, ap]))
    _, vol_f, wf_f = _sphere(cuda, SKIN_COVERAGE)
    fresh = WarpField(wf.graph, vol_f)
    fresh.set_node_transforms(wf.R_t.clone(), wf.T_t.clone())
    cf = fresh.skin_tsdf_cache()
    assert sorted(cf.brick_list[:cf.n_list].cpu().tolist()) == sorted(c.brick_list.cpu().tolist())
    for x, y in zip(wf.skin_tsdf(), fresh.skin_tsdf()):
        assert np.array_equal(x, y)
    assert _cache_by_brick(c) == _cache_by_brick(cf)
    _, vol_n, wf_n = _sphere(cuda, SKIN_COVERAGE)
    res_n = wf_n.grow_from_volume(max_points=1024, incremental=False)
    assert res_n["added"] == res["added"] and res_n["reskinned"] == wf_n._cache.n_list == c.n_list
    assert res_n["appended"] == res["appended"] and _cache_by_brick(wf_n._cache) == _cache_by_brick(c)
    # one warped integrate through each cache
    im = torch.zeros((6, 160, 200), device=cuda)
    im[-1] = 0.08
    for v, w_ in ((vol, wf), (vol_f, fresh)):
        w_.frame_id = 1
        v.with_color = False
        v.integrate({"im": im, "id": 1})
    bits = lambda t: t.view(torch.int32)                            # (the scene plants NaN voxels: compare the bytes)
    assert torch.equal(bits(vol.tsdf_b), bits(vol_f.tsdf_b)) and torch.equal(bits(vol.weight_b), bits(vol_f.weight_b))
    assert not torch.equal(bits(vol.weight_b), bits(vol_n.weight_b))   # the integrate did update voxels


def test_grow_from_volume_refusals(cuda):
    from types import SimpleNamespace
    from occlusionfusion_amd import TSDFVolume, WarpField
    tg, vol, wf = _sphere(cuda)
    with pytest.raises(RuntimeError, match="skin cache"):
        WarpField(wf.graph, vol).grow_from_volume()
    slab = TSDFVolume.from_grid(tg.ORIGIN, tg.H_VOX, tg.DIMS, (100.0, 100.0, 20.0, 16.0),
                                SimpleNamespace(source_frame=0, skip_rate=1), device=cuda, shard=(0, 2))
    ws = WarpField(wf.graph, slab)
    ws.skin_tsdf_cache()
    with pytest.raises(ValueError, match="sharded"):
        ws.grow_from_volume()


PL_DIMS, PL_H, PL_COV, PL_Z0 = (40, 24, 16), 0.01, 0.02, 0.5837
PL_ORIGIN = np.array([-0.195, -0.115, 0.5], F32)
PL_INTR, PL_HW = (200.0, 200.0, 80.0, 60.0), (120, 160)


def _plane_run(cuda, grow):
    """A static fronto-parallel plane under identity transforms: frame 0 shows its left third, where the nodes are;
    frames 1-6 show all of it. -> (warp field, the model sampled after the last integrate, the initial frontier)."""
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd.synthetic import euclidean_edges
    H, W = PL_HW
    x_third = float(PL_ORIGIN[0]) + PL_DIMS[0] * PL_H / 3
    u = np.arange(W, dtype=np.float64)
    full = np.zeros((6, H, W), F32)
    full[-1] = PL_Z0
    left = full.copy()
    left[-1][:, (u - PL_INTR[2]) * PL_Z0 / PL_INTR[0] >= x_third] = 0
    gx, gy = np.meshgrid(np.arange(float(PL_ORIGIN[0]) + 0.01, x_third - 1e-9, PL_COV),
                         np.arange(float(PL_ORIGIN[1]) + 0.01, float(PL_ORIGIN[1]) + PL_DIMS[1] * PL_H, PL_COV), indexing="ij")
    nodes = np.stack([gx.reshape(-1), gy.reshape(-1), np.full(gx.size, PL_Z0)], 1).astype(F32)
    vol = TSDFVolume.from_grid(PL_ORIGIN, PL_H, PL_DIMS, PL_INTR, SimpleNamespace(source_frame=0, skip_rate=1), device=cuda)
    vol.with_color = False
    e, ew = euclidean_edges(nodes, 8)
    wf = WarpField(EDGraph(nodes, e, ew, node_coverage=PL_COV), vol)
    vol.integrate({"im": torch.from_numpy(left).to(cuda), "id": 0})
    wf.skin_tsdf_cache()
    im = torch.from_numpy(full).to(cuda)
    added = []
    for t in range(1, 7):
        wf.frame_id = t
        vol.integrate({"im": im, "id": t})
        if grow:
            added.append(wf.grow_from_volume(max_points=4096)["added"])
    return wf, wf.surface_points(4096), float(nodes[:, 0].max()), added


def test_growth_covers_a_plane_the_fixed_graph_cannot(cuda):
    interior = (PL_DIMS[0] - 2) * (PL_DIMS[1] - 2)
    wf, m, frontier, _ = _plane_run(cuda, grow=False)
    x = m["points"][:, 0].cpu().numpy()
    i, j, _ = np.unravel_index(m["voxel"].cpu().numpy(), PL_DIMS)
    fixed_cols = len(set(zip(i.tolist(), j.tolist())))
    assert m["emitted"] == m["accepted"] > 0 and x.max() <= frontier + 4 * PL_COV      # never past the initial rim
    wf, m, _, added = _plane_run(cuda, grow=True)
    i, j, _ = np.unravel_index(m["voxel"].cpu().numpy(), PL_DIMS)
    cols = len(set(zip(i.tolist(), j.tolist())))
    print(f"plane: {fixed_cols} of {interior} interior columns with the fixed graph, {cols} with growth; added {added}, "
          f"{wf.num_nodes} nodes")
    assert m["emitted"] == m["accepted"] and cols >= 0.95 * interior
    assert added[0] > 0 and wf.num_nodes == wf.graph.nodes.shape[0] == wf.R_t.shape[0]
    assert torch.equal(wf.R_t, torch.eye(3, device=cuda).expand(wf.num_nodes, 3, 3))    # identity blends to identity
    # the skin's weights sum to s / (s + 1e-6): a point under identity transforms moves by |p|·1e-6 / (s + 1e-6), and so
    # does the voxel the integrate warps; s >= exp(-8) (an anchor lies within 4 sigma) and |p| < 0.7 m here
    assert float(wf.T_t.abs().max()) < 0.7 * 1e-6 / np.exp(-8.0)


# ---------------------------------------------------------------------------------------------- the tracking loop
def _pipeline(cuda, seq):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"))
    pipe.integrate_source(pipe.prepare(0))
    return pipe


def test_track_step_with_growth(cuda):
    """Config 1: 4 sigma = 0.4 m covers the whole sphere, so grow_every=1 adds nothing and the loop's outputs and volume
    are bitwise those of grow_every=0. With the coverage cut to a quarter (a Euclidean graph on the same nodes) a grown
    frame solves, N rises, and every array the solver and the integrate see has N rows."""
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.synthetic import euclidean_edges
    seq = S.config_sequence(1, device=cuda)
    a, b = _pipeline(cuda, seq), _pipeline(cuda, seq)
    for t in (1, 2, 3):
        oa = a.track_step(a.prepare(t), t, model="volume", max_model_points=16384)
        ob = b.track_step(b.prepare(t), t, model="volume", max_model_points=16384, grow_every=1)
        assert ob["grow"]["added"] == 0 and "grow" not in oa
        assert torch.equal(oa["node_rotations"], ob["node_rotations"])
        assert torch.equal(oa["node_translations"], ob["node_translations"])
    assert torch.equal(a.vol.tsdf_b, b.vol.tsdf_b) and torch.equal(a.vol.weight_b, b.vol.weight_b)
    with pytest.raises(ValueError, match="volume"):
        b.track_step(b.prepare(4), 4, grow_every=1)
    del a, b
    seq = S.config_sequence(1, device=cuda)
    seq.node_coverage = seq.node_coverage / 4
    seq.edges, seq.edge_weights = euclidean_edges(seq.nodes, 8)
    p = _pipeline(cuda, seq)
    n0 = p.nodes_t.shape[0]
    o1 = p.track_step(p.prepare(1), 1, model="volume", max_model_points=16384, grow_every=1, grow=dict(max_new=512))
    N = p.wf.num_nodes
    print("growth at a quarter of the coverage:", o1["grow"], "nodes", n0, "->", N)
    assert o1["valid_solve"] == 1 and o1["grow"]["added"] == N - n0 > 0
    assert p.solver.max_nodes >= N and p.solver.params["precond"] == "direct"
    for x in (p.nodes_t, p.edges_t, p.ew_t, p.prev_rot, p.prev_trans, p.wf.R_t, p.wf.T_t, p.wf.packed_nodes()):
        assert x.shape[0] == N
    fi = p.prepare(2)
    assert fi.tpos.shape[0] == n0                                   # the sequence knows the source frame's nodes only
    o2 = p.track_step(fi, 2, model="volume", max_model_points=16384, grow_every=1, grow=dict(max_new=512))
    assert o2["valid_solve"] == 1 and o2["node_rotations"].shape[0] == N and o2["node_translations"].shape[0] == N
    assert p.wf.num_nodes == N + o2["grow"]["added"]


def test_registration_grow_from_volume(cuda):
    """Registration follows the growth: previous transforms, solver capacity and the model from the volume."""
    from occlusionfusion_amd import Registration
    tg, vol, wf = _sphere(cuda)
    K = np.array([[100.0, 0, 20.0], [0, 100.0, 16.0], [0, 0, 1]])
    reg = Registration(wf.graph.nodes, wf.graph, wf, K, max_matches=2000, precond="direct")
    n0 = wf.num_nodes
    res = reg.grow_from_volume(max_points=1024)
    N = wf.num_nodes
    assert res["added"] == N - n0 > 0 and reg.graph is wf.graph and reg.graph.nodes.shape[0] == N
    assert reg.solver.max_nodes >= N and reg.solver.params["precond"] == "direct"
    assert reg.prev_rot.shape == (N, 3, 3) and reg.prev_trans.shape == (N, 3)
    assert torch.equal(reg.prev_rot, wf.R_t) and torch.equal(reg.prev_trans, wf.T_t)
    assert reg.source_pcd.shape[0] == reg.source_normals.shape[0] > 0 and int(reg.point_anchors.max()) >= n0
