"""Writes the motion completion fixtures from an OcclusionFusion checkout (data only):

    python tests/golden/make_motion_golden.py /path/to/OcclusionFusion

* motion_net.npz + motion_net_l7.npz: the 164 tensors of checkpoints/model_noise_all.tar's model_state_dict as f32 under
  their own key names. Two files (layer71 / layer72 in the second) so that each stays below 1 MiB.
* motion_demo.npz: frames 1-20 of data/input/node and data/input/graph, and per frame the f64 outputs of
  tests/motion_ref.py (raw network output, node motion, confidence; conf_scale 2), which regression-pin the restatement.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import motion_ref as mr  # noqa: E402

FRAMES = range(1, 21)


def main(ref):
    ck = torch.load(os.path.join(ref, "checkpoints", "model_noise_all.tar"), map_location="cpu", weights_only=False)
    sd = {k: v.numpy().astype(np.float32) for k, v in ck["model_state_dict"].items()}
    assert len(sd) == 164 and sum(v.size for v in sd.values()) == 294152
    last = {k: v for k, v in sd.items() if k.startswith(("layer71.", "layer72."))}
    np.savez_compressed(os.path.join(HERE, "motion_net.npz"), **{k: v for k, v in sd.items() if k not in last})
    np.savez_compressed(os.path.join(HERE, "motion_net_l7.npz"), **last)
    out = {}
    run = mr.Runner(sd, conf_scale=2.0)
    for f in FRAMES:
        node = np.load(os.path.join(ref, "data", "input", "node", f"{f:04d}.npy"))
        pyd = np.load(os.path.join(ref, "data", "input", "graph", f"{f:04d}.npz"))
        out[f"node_{f}"] = node.astype(np.float32)
        for k in pyd.files:
            out[f"{k}_{f}"] = pyd[k].astype(np.int16)
        pos, motion = node[:, :3].astype(np.float64), node[:, 3:6].astype(np.float64)
        nm, conf, raw = run(pos, pos + motion, node[:, 6] > 0.5, pyd)
        out[f"raw_{f}"], out[f"motion_{f}"], out[f"conf_{f}"] = raw, nm, conf
    np.savez_compressed(os.path.join(HERE, "motion_demo.npz"), **out)
    for n in ("motion_net.npz", "motion_net_l7.npz", "motion_demo.npz"):
        print(n, os.path.getsize(os.path.join(HERE, n)))


if __name__ == "__main__":
    main(sys.argv[1])
