"""numpy restatement of the motion completion network (OcclusionFusion motion_model.py:7-98) and of its runner's pre- and
post-processing (fusion_with_occlusion/run_motion_model.py:45-196, demo.py:28-156): the yardstick of
occlusionfusion_amd/csrc/motion.hip. Run in f64 on the f32 weights (dtype=np.float32 runs every operation in f32).

The LSTM, Linear, LayerNorm and softplus here are pinned to torch's own modules (tests/test_motion_ref.py). The graph
layers are restated from their published definition — torch_geometric's TransformerConv (1 head, root weight, no beta, no
edge features) and DeepGCNLayer block 'res+' in eval mode — and are unpinned against the reference: torch_geometric is
not available to run it.
"""
import os

import numpy as np

LAYERS = ("layer11", "layer12", "layer21", "layer22", "layer31", "layer32", "layer41", "layer42", "layer51", "layer52",
          "layer61", "layer62", "layer71", "layer72")
MAX_HIST = 16
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_weights():
    sd = {}
    for n in ("motion_net.npz", "motion_net_l7.npz"):
        with np.load(os.path.join(GOLD, n), allow_pickle=False) as z:
            sd.update({k: z[k] for k in z.files})
    return sd


def load_demo():
    with np.load(os.path.join(GOLD, "motion_demo.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def frame_pyd(demo, f):
    keys = [f"nn_index_l{l}" for l in range(4)] + [f"{d}_sample_idx{l}" for d in ("down", "up") for l in (1, 2, 3)]
    return {k: demo[f"{k}_{f}"] for k in keys}


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def softplus(x):
    """F.softplus, beta 1, threshold 20."""
    x = np.asarray(x)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0)))).astype(x.dtype)


def linear(x, w, b):
    return x @ w.T + b


def layernorm(x, w, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)      # biased
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * w + b


def lstm(seq, sd, prefix="seq_encoder", layers=2, hidden=32):
    """seq (T,N,4) -> the top layer's outputs (T,N,hidden). Gate order i, f, g, o; zero initial state."""
    x = seq
    for l in range(layers):
        wi, wh = sd[f"{prefix}.weight_ih_l{l}"], sd[f"{prefix}.weight_hh_l{l}"]
        bi, bh = sd[f"{prefix}.bias_ih_l{l}"], sd[f"{prefix}.bias_hh_l{l}"]
        h = np.zeros((x.shape[1], hidden), x.dtype)
        c = np.zeros_like(h)
        out = []
        for t in range(x.shape[0]):
            g = (x[t] @ wi.T + bi) + (h @ wh.T + bh)
            i, f, gg, o = (g[:, k * hidden:(k + 1) * hidden] for k in range(4))
            c = sigmoid(f) * c + sigmoid(i) * np.tanh(gg)
            h = sigmoid(o) * np.tanh(c)
            out.append(h)
        x = np.stack(out)
    return x


def edge_list(nn_index):
    """run_motion_model.py:134-148: (2,E) [s = the row's node, d = its listed neighbour], -1 entries dropped, in row-major
    order."""
    nn = np.asarray(nn_index).astype(np.int64)
    rows = np.repeat(np.arange(nn.shape[0], dtype=np.int64), nn.shape[1]).reshape(nn.shape)
    keep = nn >= 0
    return np.stack([rows[keep], nn[keep]])


def transformer_conv(x, edges, sd, prefix):
    """out_d = Σ_e α_e v_s + lin_skip(x_d), α = softmax over the edges sharing the target d of q_d·k_s / sqrt(C) (maximum
    subtracted, +1e-16 in the denominator), accumulated in edge-list order. A node with no incoming edge: skip only."""
    C = x.shape[1]
    q = linear(x, sd[prefix + "lin_query.weight"], sd[prefix + "lin_query.bias"])
    k = linear(x, sd[prefix + "lin_key.weight"], sd[prefix + "lin_key.bias"])
    v = linear(x, sd[prefix + "lin_value.weight"], sd[prefix + "lin_value.bias"])
    out = linear(x, sd[prefix + "lin_skip.weight"], sd[prefix + "lin_skip.bias"])
    s, d = edges
    a = (q[d] * k[s]).sum(axis=1) / x.dtype.type(np.sqrt(C))
    amax = np.full(x.shape[0], -np.inf, x.dtype)
    np.maximum.at(amax, d, a)
    e = np.exp(a - amax[d])
    den = np.zeros(x.shape[0], x.dtype)
    np.add.at(den, d, e)
    alpha = e / (den[d] + x.dtype.type(1e-16))
    agg = np.zeros_like(out)
    np.add.at(agg, d, alpha[:, None] * v[s])
    return agg + out


def transformer_conv_dense(x, edges, sd, prefix):
    """The same layer in an independent dense form: an N x N score matrix with edge multiplicities."""
    N, C = x.shape
    q = x @ sd[prefix + "lin_query.weight"].T + sd[prefix + "lin_query.bias"]
    k = x @ sd[prefix + "lin_key.weight"].T + sd[prefix + "lin_key.bias"]
    v = x @ sd[prefix + "lin_value.weight"].T + sd[prefix + "lin_value.bias"]
    mult = np.zeros((N, N), x.dtype)                       # mult[d, s] = how many times edge s -> d is listed
    for s, d in zip(*edges):
        mult[d, s] += 1
    score = (q @ k.T) / np.sqrt(C)                         # [d, s]
    out = x @ sd[prefix + "lin_skip.weight"].T + sd[prefix + "lin_skip.bias"]
    for d in range(N):
        if mult[d].sum() == 0:
            continue
        m = score[d][mult[d] > 0].max()
        wgt = mult[d] * np.exp(np.where(mult[d] > 0, score[d] - m, 0.0))
        out[d] += (wgt / (wgt.sum() + 1e-16)) @ v
    return out


def res_plus(x, edges, sd, name):
    """DeepGCNLayer block 'res+', eval mode: x + conv(relu(layernorm(x)))."""
    h = np.maximum(layernorm(x, sd[name + ".norm.weight"], sd[name + ".norm.bias"]), 0)
    return x + transformer_conv(h, edges, sd, name + ".conv.")


def cast_sd(sd, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in sd.items()}


def forward(sd, pos, curr_motion, hist, nn_index, down, up, dtype=np.float64):
    """motion_model.py:52-98. pos (N,3), curr_motion (N,4), hist (T,N,4), nn_index: the four (N_l,K_l) lists, down / up:
    the three sample maps each -> (N,4) = (mu, sigma)."""
    sd = cast_sd(sd, dtype)
    pos, curr_motion, hist = (np.asarray(a).astype(dtype) for a in (pos, curr_motion, hist))
    E = [edge_list(nn) for nn in nn_index]
    down = [np.asarray(d).astype(np.int64) for d in down]
    up = [np.asarray(u).astype(np.int64) for u in up]
    seq = lstm(hist, sd)[-1]
    seq_pred = linear(seq, sd["seq_linear.weight"], sd["seq_linear.bias"])
    x = linear(np.concatenate([pos, seq_pred, curr_motion], axis=1), sd["node_encoder.weight"], sd["node_encoder.bias"])
    f0 = transformer_conv(x, E[0], sd, "conv0.")
    f1 = res_plus(res_plus(f0, E[0], sd, "layer11"), E[0], sd, "layer12")
    f2 = res_plus(res_plus(f1[down[0]], E[1], sd, "layer21"), E[1], sd, "layer22")
    f3 = res_plus(res_plus(f2[down[1]], E[2], sd, "layer31"), E[2], sd, "layer32")
    f4 = res_plus(res_plus(f3[down[2]], E[3], sd, "layer41"), E[3], sd, "layer42")
    f5 = np.concatenate([f4[up[2]], f3], axis=1)
    f5 = res_plus(res_plus(f5, E[2], sd, "layer51"), E[2], sd, "layer52")
    f6 = np.concatenate([f5[up[1]], f2], axis=1)
    f6 = res_plus(res_plus(f6, E[1], sd, "layer61"), E[1], sd, "layer62")
    f7 = np.concatenate([f6[up[0]], f1], axis=1)
    f7 = res_plus(res_plus(f7, E[0], sd, "layer71"), E[0], sd, "layer72")
    out = np.maximum(layernorm(f7, sd["norm_out.weight"], sd["norm_out.bias"]), 0)
    pred = linear(out, sd["lin.weight"], sd["lin.bias"])
    pred[:, 3] = softplus(pred[:, 3])
    return pred


def pyramid_arrays(pyd):
    """The (nn_index, down, up) lists of a pyramid dict (EDGraph.get_graph_pyramid() / a demo graph .npz)."""
    return ([np.asarray(pyd[f"nn_index_l{l}"]) for l in range(4)],
            [np.asarray(pyd[f"down_sample_idx{l}"]) for l in (1, 2, 3)],
            [np.asarray(pyd[f"up_sample_idx{l}"]) for l in (1, 2, 3)])


def kabsch(p0, p1):
    """rigid_icp: R = V Uᵀ of H = Σ (p0 - c0)ᵀ (p1 - c1), no reflection fix; t = c1 - R c0. None where fewer than 3 rows
    or H numerically singular (|det H| <= 1e-12 |H|_F³)."""
    if len(p0) < 3:
        return None
    c0, c1 = p0.mean(axis=0), p1.mean(axis=0)
    H = (p0 - c0).T @ (p1 - c1)
    nf = np.linalg.norm(H)
    if not (nf > 0 and np.isfinite(nf) and abs(np.linalg.det(H)) > 1e-12 * nf ** 3):
        return None
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    return R, c1 - R @ c0


class Runner:
    """MotionCompleteNet_Runner / Demo without files: keeps the history, std_prev and the previous call's source positions
    and visible mask. conf_scale: 2 in the fusion runner (0.5 * 4), 4 in demo.py."""

    def __init__(self, sd, conf_scale=2.0, dtype=np.float64, max_hist=MAX_HIST):
        self.sd, self.c, self.dtype, self.max_hist = sd, conf_scale, dtype, max_hist
        self.reset()

    def reset(self):
        self.hist = None
        self.std_prev = None
        self.pos_prev = None
        self.vis_prev = None

    def preprocess(self, node_pos, node_motion, visible):
        """-> pos_c (N,3), curr_motion (N,4), hist (T,N,4), all f64, and status (bit 0 / bit 1: the current / the
        previous-frame fit was degenerate)."""
        node_pos, node_motion = np.asarray(node_pos, np.float64), np.asarray(node_motion, np.float64)
        visible = np.asarray(visible).astype(bool)
        N = node_pos.shape[0]
        status = 0
        fit = kabsch(node_pos[visible], node_pos[visible] + node_motion[visible])
        if fit is None:
            status |= 1
            self.rigid = np.zeros((N, 3))
        else:
            self.rigid = node_pos @ fit[0].T + fit[1] - node_pos
        nonrigid = node_motion - self.rigid
        curr = np.zeros((N, 4))
        curr[visible, :3] = nonrigid[visible] * 100.0
        self.std = (np.mean(np.std(curr[visible, :3], axis=0)) if visible.any() else 0.0) + 0.1
        curr[visible, :3] = curr[visible, :3] / self.std
        curr[:, 3] = visible
        prev = np.zeros((N, 4))
        prev[:, 3] = 1.0
        if self.hist is None:
            self.hist = np.zeros((1, N, 4))
        else:
            n_prev = self.pos_prev.shape[0]
            motion_prev = node_pos[:n_prev] - self.pos_prev
            fitp = kabsch(self.pos_prev[self.vis_prev], self.pos_prev[self.vis_prev] + motion_prev[self.vis_prev])
            if fitp is None:
                status |= 2
            else:
                rigid_prev = self.pos_prev @ fitp[0].T + fitp[1] - self.pos_prev
                prev[:n_prev, :3] = (motion_prev - rigid_prev) * 100.0
            T = self.hist.shape[0]
            drop = int(T == self.max_hist)
            T = min(T + 1, self.max_hist)
            temp = np.zeros((T, N, 4))
            temp[:-1, :n_prev] = self.hist[drop:] * self.std_prev / self.std
            temp[-1, :n_prev] = prev[:n_prev] / self.std
            self.hist = temp
        self.std_prev = self.std
        self.pos_prev, self.vis_prev = node_pos.copy(), visible.copy()
        self.status = status
        return node_pos - node_pos.mean(axis=0), curr, self.hist, status

    def postprocess(self, raw):
        raw = np.asarray(raw, np.float64)
        if self.status & 1:
            return np.zeros((raw.shape[0], 3)), np.zeros(raw.shape[0])
        mu, sigma = raw[:, :3], raw[:, 3]
        scale = np.sqrt(np.sum(np.square(mu), axis=1))
        conf = np.exp(-self.c * np.square(sigma / (scale + 1.0)))
        return mu * self.std / 100.0 + self.rigid, conf

    def __call__(self, source_pos, deformed_pos, visible, pyd):
        """-> node_motion (N,3), confidence (N), raw (N,4). The network sees the f32 cast of the preprocessed arrays, as
        the reference's does."""
        src, dst = np.asarray(source_pos, np.float64), np.asarray(deformed_pos, np.float64)
        pos, curr, hist, _ = self.preprocess(src, dst - src, visible)
        nn, down, up = pyramid_arrays(pyd)
        f32 = [a.astype(np.float32) for a in (pos, curr, hist)]
        self.inputs = f32
        raw = forward(self.sd, *f32, nn, down, up, dtype=self.dtype)
        return (*self.postprocess(raw), raw)
