"""CPU: the numpy restatement of the motion completion network (tests/motion_ref.py) is pinned where something can pin
it — its LSTM, Linear, LayerNorm and softplus to torch's own modules loaded with the fixture weights (f64, 1e-12), its
TransformerConv to an independent dense form (1e-12), its outputs on the demo frames to the values stored with the
fixture — and its f32 run stays within 5e-6 of its f64 run (4 x the 1.2e-6 measured when the fixture was made). The graph
layers stay unpinned against the reference itself (torch_geometric is not available)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as mr  # noqa: E402

from motion_ref import frame_pyd, load_demo, load_weights  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return load_weights()


@pytest.fixture(scope="module")
def demo():
    return load_demo()


def test_fixture_is_the_whole_state_dict(sd):
    assert len(sd) == 164 and sum(v.size for v in sd.values()) == 294152
    assert all(v.dtype == np.float32 for v in sd.values())


def test_lstm_equals_torch(sd):
    rng = np.random.default_rng(0)
    seq = rng.normal(0, 1.0, (16, 9, 4))
    m = torch.nn.LSTM(input_size=4, hidden_size=32, num_layers=2).double()
    m.load_state_dict({k[len("seq_encoder."):]: torch.from_numpy(v).double() for k, v in sd.items()
                       if k.startswith("seq_encoder.")})
    with torch.no_grad():
        want, _ = m(torch.from_numpy(seq))
    got = mr.lstm(seq, mr.cast_sd(sd, np.float64))
    assert np.abs(got - want.numpy()).max() < 1e-12


def test_linear_layernorm_softplus_equal_torch(sd):
    rng = np.random.default_rng(1)
    sd64 = mr.cast_sd(sd, np.float64)
    x = rng.normal(0, 2.0, (7, 128))
    lin = torch.nn.Linear(128, 4).double()
    lin.load_state_dict({"weight": torch.from_numpy(sd64["lin.weight"]), "bias": torch.from_numpy(sd64["lin.bias"])})
    ln = torch.nn.LayerNorm(128).double()
    ln.load_state_dict({"weight": torch.from_numpy(sd64["norm_out.weight"]), "bias": torch.from_numpy(sd64["norm_out.bias"])})
    with torch.no_grad():
        assert np.abs(mr.linear(x, sd64["lin.weight"], sd64["lin.bias"]) - lin(torch.from_numpy(x)).numpy()).max() < 1e-12
        assert np.abs(mr.layernorm(x, sd64["norm_out.weight"], sd64["norm_out.bias"])
                      - ln(torch.from_numpy(x)).numpy()).max() < 1e-12
    s = np.array([-30.0, -3.0, 0.0, 0.5, 19.9, 20.0, 20.1, 45.0])
    assert np.abs(mr.softplus(s) - F.softplus(torch.from_numpy(s)).numpy()).max() < 1e-12


def test_transformer_conv_equals_the_dense_form(sd):
    """A graph with a node nobody names, a hub, a duplicated neighbour, a self-loop and -1 padding."""
    rng = np.random.default_rng(2)
    N = 12
    nn = rng.integers(0, N - 1, (N, 4))          # node N-1 is never named
    nn[:, 0] = 3                                  # a hub
    nn[5, 1] = nn[5, 2] = 7                       # a duplicate
    nn[6, 1] = 6                                  # a self-loop
    nn[8, 2:] = -1
    E = mr.edge_list(nn)
    assert E.shape[1] == N * 4 - 2 and not (E[1] == N - 1).any()
    sd64 = mr.cast_sd(sd, np.float64)
    for prefix, C in (("conv0.", 32), ("layer61.conv.", 96)):
        x = rng.normal(0, 1.0, (N, C))
        got, want = mr.transformer_conv(x, E, sd64, prefix), mr.transformer_conv_dense(x, E, sd64, prefix)
        assert np.abs(got - want).max() < 1e-12
        skip = x @ sd64[prefix + "lin_skip.weight"].T + sd64[prefix + "lin_skip.bias"]
        assert np.abs(got[N - 1] - skip[N - 1]).max() < 1e-13     # no incoming edge: the skip term only


def test_kabsch_is_the_polar_factor_whatever_the_svd_signs():
    rng = np.random.default_rng(3)
    p0 = rng.normal(0, 0.3, (40, 3))
    ax = np.array([0.2, -0.1, 0.3])
    th = np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]]) / th
    R0 = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    p1 = p0 @ R0.T + np.array([0.01, -0.02, 0.03])
    R, t = mr.kabsch(p0, p1)
    assert np.abs(R - R0).max() < 1e-12 and np.abs(t - [0.01, -0.02, 0.03]).max() < 1e-12
    assert mr.kabsch(p0[:2], p1[:2]) is None and mr.kabsch(p0 * [1, 1, 0], p1 * [1, 1, 0]) is None


def test_stored_outputs_and_f32_run(sd, demo):
    """The chained runner reproduces the fixture's stored f64 outputs, and its f32 run stays within 5e-6 of them."""
    r64, r32 = mr.Runner(sd, 2.0), mr.Runner(sd, 2.0, dtype=np.float32)
    sizes, first_occluded, worst = [], None, 0.0
    for f in range(1, 21):
        node, pyd = demo[f"node_{f}"], frame_pyd(demo, f)
        pos, mo, vis = node[:, :3].astype(np.float64), node[:, 3:6].astype(np.float64), node[:, 6] > 0.5
        nm, conf, raw = r64(pos, pos + mo, vis, pyd)
        assert np.abs(raw - demo[f"raw_{f}"]).max() < 1e-9
        assert np.abs(nm - demo[f"motion_{f}"]).max() < 1e-11 and np.abs(conf - demo[f"conf_{f}"]).max() < 1e-9
        _, _, raw32 = r32(pos, pos + mo, vis, pyd)
        assert raw32.dtype == np.float32
        worst = max(worst, float(np.abs(raw32 - raw).max()))
        sizes.append((len(node), r64.hist.shape[0]))
        if first_occluded is None and not vis.all():
            first_occluded = f
    print("f32 vs f64 restatement, max over frames 1-20:", worst)
    assert worst < 5e-6
    assert sizes[0] == (227, 1) and sizes[-1] == (254, 16) and sizes[15][1] == 16 and sizes[14][1] == 15
    assert first_occluded == 5
    assert [demo[f"nn_index_l{l}_1"].shape[0] for l in range(4)] == [227, 55, 17, 6]
