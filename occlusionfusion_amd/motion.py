"""Motion completion: OcclusionFusion's MotionCompleteNet (motion_model.py:7-98) and its runner
(fusion_with_occlusion/run_motion_model.py:45-196) as an inference-only device path (csrc/motion.hip).

MotionCompleter is the twin of MotionCompleteNet_Runner: it keeps the motion history, std_prev and the previous call's
node positions on the device, and fills the Gauss-Newton solve's motion term (target_node_pos, node_conf) for the nodes
the camera cannot see. The LSTM / Linear / LayerNorm parts are pinned to torch's modules by the tests; the graph layers
(TransformerConv, DeepGCNLayer) are restated from their definition and unpinned against the reference.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import byref, call, ptr, stream_ptr

TAG = 0x4D4F5431   # 'MOT1': the blob layout of csrc/motion.hip
MAX_HIST = 16
# the 15 TransformerConv layers in forward order: (state-dict prefix of the conv, of the norm (None: conv0), width)
CONVS = (("conv0.", None, 32),) + tuple(
    (f"{n}.conv.", f"{n}.norm.", c) for n, c in (
        ("layer11", 32), ("layer12", 32), ("layer21", 32), ("layer22", 32), ("layer31", 32), ("layer32", 32),
        ("layer41", 32), ("layer42", 32), ("layer51", 64), ("layer52", 64), ("layer61", 96), ("layer62", 96),
        ("layer71", 128), ("layer72", 128)))


def _expected_shapes():
    sh = {"node_encoder.weight": (32, 11), "node_encoder.bias": (32,), "seq_linear.weight": (4, 32),
          "seq_linear.bias": (4,), "norm_out.weight": (128,), "norm_out.bias": (128,), "lin.weight": (4, 128),
          "lin.bias": (4,)}
    for l, cin in ((0, 4), (1, 32)):
        sh[f"seq_encoder.weight_ih_l{l}"] = (128, cin)
        sh[f"seq_encoder.weight_hh_l{l}"] = (128, 32)
        sh[f"seq_encoder.bias_ih_l{l}"] = sh[f"seq_encoder.bias_hh_l{l}"] = (128,)
    for conv, norm, c in CONVS:
        for lin in ("query", "key", "value", "skip"):
            sh[f"{conv}lin_{lin}.weight"], sh[f"{conv}lin_{lin}.bias"] = (c, c), (c,)
        if norm:
            sh[norm + "weight"] = sh[norm + "bias"] = (c,)
    return sh


SHAPES = _expected_shapes()


def blob_floats():
    return 2 + sum(int(np.prod(s)) for s in SHAPES.values()) + 2 * 32   # (conv0 carries an identity norm)


def pack_weights(state_dict):
    """The model_state_dict (tensors or arrays, the reference's 164 keys) -> the packed f32 blob ofx_motion_create takes:
    word 0 the layout tag, word 1 the length (uint32 bit patterns), then the LSTM / seq_linear / node_encoder weights,
    the 15 conv layers (Wᵀ (C,4C) with columns q | k | v | skip, bias (4C), norm weight, norm bias) and the head; every
    matrix transposed, so that consecutive threads read consecutive words. A missing key or a wrong shape is refused."""
    sd = {}
    for k, shape in SHAPES.items():
        if k not in state_dict:
            raise KeyError(f"pack_weights: the state dict has no {k!r}")
        v = state_dict[k]
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if tuple(v.shape) != shape:
            raise ValueError(f"pack_weights: {k} has shape {tuple(v.shape)}, the network's is {shape}")
        sd[k] = np.ascontiguousarray(v, np.float32)
    unknown = set(state_dict) - set(SHAPES)
    if unknown:
        raise ValueError(f"pack_weights: keys the network does not have: {sorted(unknown)[:4]}")
    parts = []
    for l in (0, 1):
        parts += [sd[f"seq_encoder.weight_ih_l{l}"].T, sd[f"seq_encoder.weight_hh_l{l}"].T,
                  sd[f"seq_encoder.bias_ih_l{l}"], sd[f"seq_encoder.bias_hh_l{l}"]]
    parts += [sd["seq_linear.weight"].T, sd["seq_linear.bias"], sd["node_encoder.weight"].T, sd["node_encoder.bias"]]
    for conv, norm, c in CONVS:
        names = [f"{conv}lin_{lin}" for lin in ("query", "key", "value", "skip")]
        parts.append(np.concatenate([sd[n + ".weight"].T for n in names], axis=1))       # (C, 4C)
        parts.append(np.concatenate([sd[n + ".bias"] for n in names]))
        parts += [sd[norm + "weight"], sd[norm + "bias"]] if norm else [np.ones(c, np.float32), np.zeros(c, np.float32)]
    parts += [sd["norm_out.weight"], sd["norm_out.bias"], sd["lin.weight"].T, sd["lin.bias"]]
    body = np.concatenate([np.ascontiguousarray(p, np.float32).reshape(-1) for p in parts])
    head = np.array([TAG, body.size + 2], np.uint32).view(np.float32)
    blob = np.concatenate([head, body])
    assert blob.size == blob_floats()
    return blob


def unpack_weights(blob):
    """pack_weights backwards (the identity norm of conv0 is dropped): -> {key: f32 array}."""
    blob = np.asarray(blob, np.float32)
    head = blob[:2].view(np.uint32)
    if blob.size != blob_floats() or int(head[0]) != TAG or int(head[1]) != blob.size:
        raise ValueError("unpack_weights: not a motion weight blob of this layout")
    pos, sd = [2], {}

    def take(*shape):
        n = int(np.prod(shape))
        out = blob[pos[0]:pos[0] + n].reshape(shape)
        pos[0] += n
        return out

    for l, cin in ((0, 4), (1, 32)):
        sd[f"seq_encoder.weight_ih_l{l}"] = take(cin, 128).T
        sd[f"seq_encoder.weight_hh_l{l}"] = take(32, 128).T
        sd[f"seq_encoder.bias_ih_l{l}"], sd[f"seq_encoder.bias_hh_l{l}"] = take(128), take(128)
    sd["seq_linear.weight"], sd["seq_linear.bias"] = take(32, 4).T, take(4)
    sd["node_encoder.weight"], sd["node_encoder.bias"] = take(11, 32).T, take(32)
    for conv, norm, c in CONVS:
        W, b = take(c, 4 * c), take(4 * c)
        for i, lin in enumerate(("query", "key", "value", "skip")):
            sd[f"{conv}lin_{lin}.weight"], sd[f"{conv}lin_{lin}.bias"] = W[:, i * c:(i + 1) * c].T, b[i * c:(i + 1) * c]
        nw, nb = take(c), take(c)
        if norm:
            sd[norm + "weight"], sd[norm + "bias"] = nw, nb
    sd["norm_out.weight"], sd["norm_out.bias"] = take(128), take(128)
    sd["lin.weight"], sd["lin.bias"] = take(128, 4).T, take(4)
    return {k: np.ascontiguousarray(v) for k, v in sd.items()}


def load_state_dict(path):
    """A torch checkpoint holding `model_state_dict` (checkpoints/model_noise_all.tar), or an .npz with the same keys."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    ck = torch.load(path, map_location="cpu", weights_only=False)
    return dict(ck["model_state_dict"] if "model_state_dict" in ck else ck)


def motion_term(motion_net, nodes, prev_trans, trans, visible):
    """The solver's motion term from a completer, as fusion.py:142-151 forms it: the nodes deformed at the source
    (nodes + prev_trans; prev_trans None = not moved yet) and at the tracked estimate (nodes + trans) go through
    motion_net with the source frame's visible mask. -> ((target_node_pos f32 (N,3) = deformed_at_source + node_motion,
    node_conf f32 (N)), {"node_motion", "confidence", "visible", "status"}), device tensors; the sum is taken in f64."""
    dev = motion_net.device
    nodes = torch.as_tensor(nodes, device=dev).to(torch.float64)
    src = nodes if prev_trans is None else nodes + torch.as_tensor(prev_trans, device=dev).to(torch.float64)
    dst = nodes + torch.as_tensor(trans, device=dev).to(torch.float64)
    vis = torch.as_tensor(np.ascontiguousarray(visible) if isinstance(visible, np.ndarray) else visible, device=dev)
    vis = (vis != 0).reshape(-1)
    nm, conf = motion_net(src, dst, vis)
    info = {"node_motion": nm, "confidence": conf, "visible": vis, "status": motion_net.last["status"]}
    return ((src + nm).to(torch.float32), conf.to(torch.float32)), info


class MotionCompleter:
    """MotionCompleteNet_Runner on the device. conf_scale: 2 as the fusion runner (0.5 * 4); demo.py uses 4."""

    def __init__(self, state_dict, max_nodes=4096, max_hist=MAX_HIST, conf_scale=2.0, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("MotionCompleter needs a HIP device (there is no CPU path)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_nodes, self.max_hist, self.conf_scale = int(max_nodes), int(max_hist), float(conf_scale)
        blob = pack_weights(state_dict)
        h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            call("ofx_motion_create", blob.ctypes.data_as(_lib.c_void_p), blob.size, self.max_nodes, self.max_hist, byref(h))
        self._h = h
        self.state = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.calls = 0
        self.last = None

    @classmethod
    def from_checkpoint(cls, path, **kw):
        return cls(load_state_dict(path), **kw)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                _lib.lib.ofx_motion_destroy(h)
            except Exception:   # (interpreter shutdown: the library may be gone already)
                pass

    @property
    def handle(self):
        return self._h.value

    def _i32(self, a):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32)))
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def set_graph(self, pyd):
        """pyd: what EDGraph.get_graph_pyramid() returns (or the demo's graph arrays): nn_index_l0..3 (N_l, K_l) with -1
        padding, down_sample_idx1..3, up_sample_idx1..3. Stream-ordered; the device builds the incoming-edge lists."""
        nn = [self._i32(pyd[f"nn_index_l{l}"]) for l in range(4)]
        down = [self._i32(pyd[f"down_sample_idx{l}"]).reshape(-1) for l in (1, 2, 3)]
        up = [self._i32(pyd[f"up_sample_idx{l}"]).reshape(-1) for l in (1, 2, 3)]
        for l in range(4):
            if nn[l].dim() != 2:
                raise ValueError(f"set_graph: nn_index_l{l} must be (N, K)")
        for l in range(3):
            if down[l].numel() != nn[l + 1].shape[0] or up[l].numel() != nn[l].shape[0]:
                raise ValueError(f"set_graph: the sample maps of level {l + 1} do not fit the level sizes "
                                 f"{[int(t.shape[0]) for t in nn]}")
        g = _lib.MotionGraph()
        for l in range(4):
            g.nn_index[l], g.n[l], g.k[l] = nn[l].data_ptr(), nn[l].shape[0], nn[l].shape[1]
        for l in range(3):
            g.down[l], g.up[l] = down[l].data_ptr(), up[l].data_ptr()
        with torch.cuda.device(self.device):
            call("ofx_motion_set_graph", self._h, byref(g), stream_ptr(torch.cuda.current_stream(self.device)))
        self._graph_keep = (nn, down, up)   # alive until the copies have run
        self.n_nodes = int(nn[0].shape[0])

    def info(self):
        a = (_lib.c_int64 * 10)()
        call("ofx_motion_info", self._h, a)
        return dict(launches=a[0], hist_rows=a[1], n_prev=a[2], max_nodes=a[3], levels=list(a[4:8]), max_hist=a[8])

    def _f(self, a, dtype):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def forward(self, pos, curr_motion, hist):
        """The network alone (torch.ops.ofx.motion_forward) -> f32 (N,4) = (mu, sigma)."""
        return ops.motion_forward(self.state, self.handle, self._f(pos, torch.float32),
                                  self._f(curr_motion, torch.float32), self._f(hist, torch.float32))

    def __call__(self, source_node_positions, deformed_node_positions, visible_mask):
        """-> device tensors (node_motion f64 (N,3), confidence f64 (N)). The node count may have grown since the last
        call (set_graph first). self.last holds status (i32 (1), device) and the network's inputs and raw output."""
        vis = visible_mask if isinstance(visible_mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(visible_mask))
        vis = (vis.to(self.device) != 0).reshape(-1)
        nm, conf, status, pos, cm, hist, raw = ops.motion_complete(
            self.state, self.handle, self._f(source_node_positions, torch.float64),
            self._f(deformed_node_positions, torch.float64), vis, self.conf_scale, self.max_hist)
        self.calls += 1
        self.last = dict(status=status, pos=pos, curr_motion=cm, hist=hist[:min(self.calls, self.max_hist)], raw=raw)
        return nm, conf

    def reset(self):
        call("ofx_motion_reset", self._h)
        self.calls = 0
        self.last = None
