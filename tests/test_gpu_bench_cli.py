"""bench.py's command line: a plain run times exactly --steps frames and reports ms_per_step without the legs that
sit behind --full; --dump-outputs writes the last timed step's outputs (solve transforms, fused volume) as .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_parse(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "0", "--full",
                                      "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(cuda, tmp_path):
    """Config 1 (128^3, 199 nodes: the smallest preset), 3 timed frames after 1 warmup one."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=240,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["breakdown_ms"]["valid_solves"] == 3                      # three timed solves, all valid
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32/f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6   # one GPU: frames/s = 1 / step
    assert "cpu_baseline" not in d and "roofline_integrate" not in d   # behind --full
    files = {f: np.load(out / f, allow_pickle=False) for f in sorted(os.listdir(out))}
    assert set(files) == {f"{n}.npy" for n in ("node_rotations", "node_translations", "solve_status", "tsdf_sample",
                                              "color_sample", "weight_sample")}
    assert all(x.dtype in (np.float32, np.float64) for x in files.values())
    assert sum(x.nbytes for x in files.values()) <= 64 * 10 ** 6
    N = d["config"]["nodes"]
    R, T = files["node_rotations.npy"], files["node_translations.npy"]
    assert R.shape == (N, 3, 3) and T.shape == (N, 3)
    # the file holds proper rotations, not their accuracy (test_config1_gn_matches_dense_oracle pins that): the solver
    # composes 4 solves x 10 GN updates in f32 as the reference does, without re-orthonormalising, so R Rᵀ drifts from I
    # by some 1e-5; anything that is not a rotation (translations, a wrong reshape, garbage) misses 1e-3 by far
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), R.shape), atol=1e-3)
    np.testing.assert_allclose(np.linalg.det(R.astype(np.float64)), 1.0, atol=1e-3)
    assert np.abs(T).max() > 0                                         # the scene moves: the solve returned a motion
    V = d["config"]["dims"] ** 3                                       # 2 Mi voxels: no more than the sample, so whole
    tsdf, w = files["tsdf_sample.npy"], files["weight_sample.npy"]
    assert tsdf.shape == w.shape == files["color_sample.npy"].shape == (V,)
    assert np.isfinite(tsdf).all() and np.abs(tsdf).max() <= 1.0
    assert w.max() >= 2 and (tsdf[w > 0] < 1).any()                    # source frame + warped frames were fused
