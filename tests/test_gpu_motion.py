"""GPU: the motion completion network and its runner on the device (csrc/motion.hip, occlusionfusion_amd/motion.py)
against the f64 restatement tests/motion_ref.py, on the fixtures under tests/golden only.

* network parity on demo frames 1, 5, 16, 17, 20 (T = 1, first occlusion, the history cap, the first drop, N = 254), on a
  hand-made graph with every edge case (T = 1 and 16) and on a random 8-NN graph of 2,500 nodes: (mu, sigma) within 1e-5;
* two runs bitwise equal, at most 34 launches per forward;
* the preprocessing alone within 2 f32 ulp of the restatement's f32-cast arrays (frames 2, 6, 18), the degenerate case;
* the completer chained over frames 1-20 with its state on the device: node motion within 1e-6 m, confidence within 1e-5;
* each operator bit-identical to the direct C-ABI call, and torch.library.opcheck.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as mr  # noqa: E402
from motion_ref import frame_pyd, load_demo, load_weights  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-5          # the project's parity bar on (mu, sigma)
FRAMES = range(1, 21)


@pytest.fixture(scope="module")
def sd():
    return load_weights()


@pytest.fixture(scope="module")
def demo():
    return load_demo()


@pytest.fixture(scope="module")
def chain(sd, demo):
    """The restatement chained over frames 1-20, computed once: per frame its f32 network inputs and f64 outputs."""
    run, out = mr.Runner(sd, 2.0), {}
    for f in FRAMES:
        node = demo[f"node_{f}"]
        pos, mo, vis = node[:, :3].astype(np.float64), node[:, 3:6].astype(np.float64), node[:, 6] > 0.5
        nm, conf, raw = run(pos, pos + mo, vis, frame_pyd(demo, f))
        out[f] = dict(src=pos, dst=pos + mo, vis=vis, inputs=[a.copy() for a in run.inputs], raw=raw, motion=nm, conf=conf)
    return out


@pytest.fixture(scope="module")
def net(sd, cuda):
    from occlusionfusion_amd.motion import MotionCompleter
    return MotionCompleter(sd, device=cuda)


def hand_graph():
    """N = 70 (one wave plus 6), K = 8: -1 padding, node 69 that no list names, hub 3 named by every row (in-degree 70,
    more than one wave of edges), a duplicated neighbour in row 5, a self-loop in row 6; levels of 9, 3 and 1 nodes, the
    last with all -1 edges."""
    rng = np.random.default_rng(5)
    nn0 = rng.integers(0, 69, (70, 8))
    nn0[:, 0] = 3
    nn0[5, 1] = nn0[5, 2] = 11
    nn0[6, 1] = 6
    nn0[8, 5:] = -1
    nn0[69, 1:] = -1
    nn1 = rng.integers(0, 9, (9, 6))
    nn1[2, 3:] = -1
    nn2 = np.array([[1, 2], [0, -1], [0, 0]])
    nn3 = np.full((1, 3), -1)
    pyd = {"nn_index_l0": nn0, "nn_index_l1": nn1, "nn_index_l2": nn2, "nn_index_l3": nn3,
           "down_sample_idx1": rng.choice(70, 9, replace=False), "down_sample_idx2": np.array([7, 0, 4]),
           "down_sample_idx3": np.array([2]), "up_sample_idx1": rng.integers(0, 9, 70),
           "up_sample_idx2": rng.integers(0, 3, 9), "up_sample_idx3": np.zeros(3, np.int64)}
    assert not (nn0 == 69).any() and (nn0 == 3).sum() >= 65
    return pyd


def knn_graph(n=2500, seed=6):
    """A random 8-NN graph of n points and three levels of every 4th point (6, 4, 3 neighbours)."""
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 0.4, (n, 3))
    pyd, idx = {}, np.arange(n)
    for l, k in enumerate((8, 6, 4, 3)):
        p = pts[idx]
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d, np.inf)
        pyd[f"nn_index_l{l}"] = np.argsort(d, axis=1)[:, :k]
        if l < 3:
            keep = np.arange(0, len(idx), 4)
            pyd[f"down_sample_idx{l + 1}"] = keep
            pyd[f"up_sample_idx{l + 1}"] = np.minimum(np.arange(len(idx)) // 4, len(keep) - 1)
            idx = idx[keep]
    return pts, pyd


def random_inputs(n, T, seed, pos=None):
    rng = np.random.default_rng(seed)
    pos = rng.normal(0, 0.3, (n, 3)) if pos is None else pos - pos.mean(axis=0)
    cm = rng.normal(0, 1.0, (n, 4))
    cm[:, 3] = rng.random(n) > 0.3
    cm[cm[:, 3] == 0, :3] = 0
    hist = rng.normal(0, 1.0, (T, n, 4))
    return [a.astype(np.float32) for a in (pos, cm, hist)]


def check_forward(net, sd, pyd, inputs, what):
    net.set_graph(pyd)
    got = net.forward(*inputs).cpu().numpy().astype(np.float64)
    want = mr.forward(sd, *inputs, *mr.pyramid_arrays(pyd))
    err = float(np.abs(got - want).max())
    print(f"{what}: max |(mu, sigma) - f64 restatement| = {err:.3e} (outputs up to {np.abs(want).max():.2f})")
    assert np.isfinite(got).all() and err < BAR, (what, err)
    return err


@pytest.mark.parametrize("f", [1, 5, 16, 17, 20])
def test_network_parity_on_demo_frames(net, sd, demo, chain, f):
    c = chain[f]
    assert c["inputs"][2].shape[0] == min(f, 16) and c["inputs"][0].shape[0] == (254 if f == 20 else len(c["vis"]))
    net.set_graph(frame_pyd(demo, f))
    got = net.forward(*c["inputs"]).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - c["raw"]).max())
    print(f"frame {f}: N = {len(got)}, T = {min(f, 16)}, max |(mu, sigma) - f64 restatement| = {err:.3e}")
    assert err < BAR


@pytest.mark.parametrize("T", [1, 16])
def test_graph_edge_cases(net, sd, T):
    check_forward(net, sd, hand_graph(), random_inputs(70, T, 10 + T), f"hand-made graph, T = {T}")


def test_grid_sizing_2500_nodes(net, sd):
    pts, pyd = knn_graph()
    check_forward(net, sd, pyd, random_inputs(2500, 3, 20, pos=pts), "random 8-NN graph, N = 2500")


def test_repeatable_and_launch_count(net, demo, chain):
    net.set_graph(frame_pyd(demo, 20))
    a = net.forward(*chain[20]["inputs"])
    b = net.forward(*chain[20]["inputs"])
    assert torch.equal(a, b)
    net.set_graph(frame_pyd(demo, 20))      # the edge lists are rebuilt in the same order
    assert torch.equal(a, net.forward(*chain[20]["inputs"]))
    assert 1 <= net.info()["launches"] <= 34
    assert net.info()["levels"] == [254, 60, 18, 11]


@pytest.fixture(scope="module")
def chained(sd, demo, chain, cuda):
    """The completer chained over frames 1-20, its state on the device; per frame its outputs on the host."""
    from occlusionfusion_amd.motion import MotionCompleter
    mc, out = MotionCompleter(sd, device=cuda), {}
    for f in FRAMES:
        c = chain[f]
        mc.set_graph(frame_pyd(demo, f))
        nm, conf = mc(c["src"], c["dst"], c["vis"])
        out[f] = dict(motion=nm.cpu().numpy(), conf=conf.cpu().numpy(), status=int(mc.last["status"].item()),
                      pos=mc.last["pos"].cpu().numpy(), cm=mc.last["curr_motion"].cpu().numpy(),
                      hist=mc.last["hist"].cpu().numpy(), raw=mc.last["raw"].cpu().numpy())
    return out


def ulps(got, want):
    """|got - want| in units of want's f32 spacing, elementwise maximum."""
    sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp).max())


@pytest.mark.parametrize("f", [2, 6, 18])
def test_preprocessing_alone(chained, chain, f):
    pos, cm, hist = chain[f]["inputs"]
    g = chained[f]
    assert g["status"] == 0 and g["hist"].shape == hist.shape
    u = [ulps(g["pos"], pos), ulps(g["cm"], cm), ulps(g["hist"], hist)]
    print(f"frame {f}: centred positions / curr_motion / history differ by at most {u} f32 ulp")
    assert max(u) <= 2.0


def test_end_to_end_over_20_frames(chained, chain):
    em = ec = 0.0
    for f in FRAMES:
        assert chained[f]["motion"].shape == chain[f]["motion"].shape and chained[f]["status"] == 0
        em = max(em, float(np.abs(chained[f]["motion"] - chain[f]["motion"]).max()))
        ec = max(ec, float(np.abs(chained[f]["conf"] - chain[f]["conf"]).max()))
    print(f"frames 1-20 chained, N 227 -> 254: max node motion error {em:.3e} m, max confidence error {ec:.3e}")
    assert len(chained[1]["conf"]) == 227 and len(chained[20]["conf"]) == 254
    assert em < 1e-6 and ec < 1e-5


def test_degenerate_fit_gives_zeros_and_advances_the_history(sd, demo, chain, cuda):
    from occlusionfusion_amd.motion import MotionCompleter
    mc = MotionCompleter(sd, device=cuda)
    mc.set_graph(frame_pyd(demo, 1))
    c = chain[1]
    mc(c["src"], c["dst"], c["vis"])
    vis = np.zeros(len(c["vis"]), bool)
    vis[[3, 40]] = True
    nm, conf = mc(c["src"], c["dst"], vis)
    assert int(mc.last["status"].item()) & 1
    assert not nm.any().item() and not conf.any().item()
    assert mc.info()["hist_rows"] == 2 and tuple(mc.last["hist"].shape) == (2, 227, 4)
    ref = mr.Runner(sd, 2.0)
    ref.preprocess(c["src"], c["dst"] - c["src"], c["vis"])
    pos, cm, hist, status = ref.preprocess(c["src"], c["dst"] - c["src"], vis)
    assert status == 1
    assert np.abs(mc.last["hist"].cpu().numpy() - hist).max() < 1e-6
    assert np.abs(mc.last["curr_motion"].cpu().numpy() - cm).max() < 1e-5
    mc.reset()
    nm, conf = mc(c["src"], c["dst"], c["vis"])
    assert int(mc.last["status"].item()) == 0 and mc.info()["hist_rows"] == 1
    assert np.abs(nm.cpu().numpy() - c["motion"]).max() < 1e-6


def _direct_handle(sd, max_hist):
    from occlusionfusion_amd import _lib
    from occlusionfusion_amd.motion import pack_weights
    blob = pack_weights(sd)
    h = ctypes.c_void_p()
    _lib.call("ofx_motion_create", blob.ctypes.data_as(ctypes.c_void_p), blob.size, 512, max_hist, ctypes.byref(h))
    return h


def test_ops_equal_c_abi_and_opcheck(sd, demo, chain, cuda):
    from occlusionfusion_amd import _lib
    from occlusionfusion_amd._lib import ptr, stream_ptr
    from occlusionfusion_amd.motion import MotionCompleter
    mc = MotionCompleter(sd, max_nodes=512, max_hist=1, device=cuda)
    pyd = frame_pyd(demo, 5)
    mc.set_graph(pyd)
    c = chain[5]
    pos, cm, hist = (torch.from_numpy(a).to(cuda) for a in c["inputs"])
    out = torch.ops.ofx.motion_forward(mc.state, mc.handle, pos, cm, hist)
    direct = torch.empty_like(out)
    _lib.call("ofx_motion_forward", ctypes.c_void_p(mc.handle), ptr(pos), ptr(cm), ptr(hist), hist.shape[0], pos.shape[0],
              ptr(direct), stream_ptr())
    assert torch.equal(out, direct)
    torch.library.opcheck(torch.ops.ofx.motion_forward.default, (mc.state, mc.handle, pos, cm, hist))
    # motion_complete: a second handle driven through the C ABI sees the same two calls
    src, dst = torch.from_numpy(c["src"]).to(cuda), torch.from_numpy(c["dst"]).to(cuda)
    vis = torch.from_numpy(c["vis"]).to(cuda)
    h = _direct_handle(sd, 1)
    other = MotionCompleter.__new__(MotionCompleter)   # (set_graph's marshalling for the bare handle)
    other._h, other.device = h, cuda
    try:
        MotionCompleter.set_graph(other, pyd)
        N = src.shape[0]
        for _ in range(2):
            got = torch.ops.ofx.motion_complete(mc.state, mc.handle, src, dst, vis, 2.0, 1)
            want = (torch.empty(N, 3, dtype=torch.float64, device=cuda), torch.empty(N, dtype=torch.float64, device=cuda),
                    torch.empty(1, dtype=torch.int32, device=cuda), torch.empty(N, 3, device=cuda),
                    torch.empty(N, 4, device=cuda), torch.zeros(1, N, 4, device=cuda), torch.empty(N, 4, device=cuda))
            _lib.call("ofx_motion_complete", h, ptr(src), ptr(dst), ptr(vis.to(torch.uint8)), N, 2.0,
                      *[ptr(t) for t in want], stream_ptr())
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        other._h = None
        torch.cuda.synchronize()
        _lib.call("ofx_motion_destroy", h)
    # from the second call on a max_hist = 1 handle fed the same frame is in a steady state: opcheck's repeated calls agree
    torch.library.opcheck(torch.ops.ofx.motion_complete.default, (mc.state, mc.handle, src, dst, vis, 2.0, 1))
    with pytest.raises(ValueError):
        torch.ops.ofx.motion_complete(mc.state, mc.handle, src, dst, vis, 2.0, 16)


def test_refused_arguments(sd, demo, chain, cuda):
    from occlusionfusion_amd import _lib
    from occlusionfusion_amd.motion import MotionCompleter
    mc = MotionCompleter(sd, max_nodes=256, device=cuda)
    pos, cm, hist = chain[1]["inputs"]
    with pytest.raises(_lib.OfxError):        # no graph yet
        mc.forward(pos, cm, hist)
    mc.set_graph(frame_pyd(demo, 1))
    with pytest.raises(_lib.OfxError):        # not the graph's node count
        mc.forward(pos[:200], cm[:200], hist[:, :200])
    pyd = knn_graph(300)[1]
    with pytest.raises(_lib.OfxError):        # above max_nodes
        mc.set_graph(pyd)
