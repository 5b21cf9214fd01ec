"""CPU: closed-form known answers for the numpy restatement of ofx_surface_points (tests/surface_ref.py): a
fronto-parallel plane, an analytic sphere, the thinning rule with its padding rows — and the condition the GPU tracking
test relies on: the share of the volume model that the identity association accepts on config 1's frame 20."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
import surface_ref as sr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
H_VOX, TRUNC = 0.01, 0.04
ORIGIN = np.zeros(3, F32)
SPHERE_DIMS, SPHERE_C, SPHERE_R = (20, 18, 22), np.array([0.095, 0.085, 0.105]), 0.06


def _all_bricks(dims):
    return np.arange(np.prod([(d + 7) // 8 for d in dims]), dtype=np.int32)


def _one_node_skin(dims):
    V = int(np.prod(dims))
    return np.zeros((V, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (V, 1))


def _centres(dims):
    return fo.world_points(ORIGIN, dims, H_VOX).reshape(tuple(dims) + (3,)).astype(np.float64)


def sphere_tsdf(dims=SPHERE_DIMS):
    d = np.linalg.norm(_centres(dims) - SPHERE_C, axis=-1) - SPHERE_R
    return np.clip(d / TRUNC, -1, 1).astype(F32)


def test_fronto_parallel_plane():
    dims, z0 = (12, 10, 16), 0.0837
    c = _centres(dims)
    phi = np.clip((z0 - c[..., 2]) / TRUNC, -1, 1).astype(F32)
    a, w = _one_node_skin(dims)
    V = int(np.prod(dims))
    out = sr.surface_points(phi, np.ones(dims, F32), ORIGIN, H_VOX, _all_bricks(dims), a, w, 1.0, V)
    n_acc, n_emit = out["count"].tolist()
    inner_columns = (dims[0] - 2) * (dims[1] - 2)
    assert n_acc == n_emit == inner_columns                       # exactly one voxel per interior (i, j) column
    vox = out["voxel"][:n_emit]
    i, j, k = np.unravel_index(vox, dims)
    assert len(set(zip(i.tolist(), j.tolist()))) == inner_columns
    assert np.all(k == 8)                                         # z = 0.08: the last voxel in front of z0 = 0.0837
    assert np.array_equal(out["normals"][:n_emit], np.tile(np.array([0, 0, -1], F32), (n_emit, 1)))
    p = out["points"][:n_emit]
    cf = c.astype(F32)
    assert np.array_equal(p[:, 0], cf[i, j, k, 0]) and np.array_equal(p[:, 1], cf[i, j, k, 1])
    ulp = float(np.spacing(F32(z0)))
    err = np.abs(p[:, 2].astype(np.float64) - z0).max()
    print(f"plane: |p_z - z0| max = {err / ulp:.2f} ulp of z0")
    assert err <= 4 * ulp
    hist = np.bincount(out["code"], minlength=8)
    assert hist[0] == inner_columns and hist[6] == 0 and hist[7] == 0 and hist[4] == 0


def test_analytic_sphere():
    phi = sphere_tsdf()
    a, w = _one_node_skin(SPHERE_DIMS)
    V = int(np.prod(SPHERE_DIMS))
    out = sr.surface_points(phi, np.ones(SPHERE_DIMS, F32), ORIGIN, H_VOX, _all_bricks(SPHERE_DIMS), a, w, 1.0, V)
    n = int(out["count"][1])
    hist = np.bincount(out["code"], minlength=8)
    p = out["points"][:n].astype(np.float64) - SPHERE_C
    r = np.linalg.norm(p, axis=1)
    err = np.abs(r - SPHERE_R).max()
    cos = (out["normals"][:n].astype(np.float64) * (p / r[:, None])).sum(1)
    print(f"sphere: {n} accepted, codes {hist.tolist()}, max |r - R| = {err / H_VOX:.4f} h, min cos = {cos.min():.6f}")
    assert out["count"].tolist() == [n, n] and n > 300 and hist[6] == 0
    assert err <= H_VOX / 20
    assert cos.min() >= 0.9999
    assert np.abs(np.linalg.norm(out["normals"][:n].astype(np.float64), axis=1) - 1).max() < 1e-6
    # every accepted voxel lies outside the sphere, within a voxel diagonal of it, and is listed in (slot, l) order
    i, j, k = np.unravel_index(out["voxel"][:n], SPHERE_DIMS)
    d = np.linalg.norm(_centres(SPHERE_DIMS)[i, j, k] - SPHERE_C, axis=1) - SPHERE_R
    assert d.min() >= 0 and d.max() < H_VOX * np.sqrt(3)
    key = ((i // 8 * 3 + j // 8) * 3 + k // 8) * 512 + ((i % 8) * 8 + j % 8) * 8 + k % 8
    assert np.all(np.diff(key) > 0)


@pytest.mark.parametrize("which", ["below", "exact", "above", "zero"])
def test_thinning_and_padding_rows(which):
    phi = sphere_tsdf()
    a, w = _one_node_skin(SPHERE_DIMS)
    args = (phi, np.ones(SPHERE_DIMS, F32), ORIGIN, H_VOX, _all_bricks(SPHERE_DIMS), a, w, 1.0)
    full = sr.surface_points(*args, int(np.prod(SPHERE_DIMS)))
    n = int(full["count"][0])
    M = {"below": 100, "exact": n, "above": n + 9, "zero": 0}[which]
    out = sr.surface_points(*args, M)
    E = min(n, M)
    assert out["count"].tolist() == [n, E]
    keep = [r for r in range(n) if n <= M or ((r + 1) * M) // n > (r * M) // n]   # the rule, in Python integers
    assert len(keep) == E
    for key in ("points", "normals", "anchors", "weights", "voxel"):
        assert out[key].shape[0] == M
        assert np.array_equal(out[key][:E], full[key][:n][keep])
        assert np.all(out[key][E:] == (-1 if key == "voxel" else 0))             # the padding rows are defined
    assert np.all(out["valid"][:E] == 1) and np.all(out["valid"][E:] == 0)
    assert np.array_equal(out["code"], full["code"])                             # thinning never changes a code


def test_listed_bricks_fix_the_order_and_padding_is_code_1():
    phi = sphere_tsdf()
    a, w = _one_node_skin(SPHERE_DIMS)
    blist = np.array([13, 4, 26, 22], np.int32)                   # any order, a subset: rows follow the list
    out = sr.surface_points(phi, np.ones(SPHERE_DIMS, F32), ORIGIN, H_VOX, blist, a, w, 1.0, 4096)
    n = int(out["count"][1])
    i, j, k = np.unravel_index(out["voxel"][:n], SPHERE_DIMS)
    brick = (i // 8 * 3 + j // 8) * 3 + k // 8
    slot = np.array([blist.tolist().index(b) for b in brick])
    assert n > 0 and np.all(np.diff(slot) >= 0) and set(brick.tolist()) <= set(blist.tolist())
    code = out["code"].reshape(4, 8, 8, 8)
    assert np.all(code[2, 4:, :, :] == 1) and np.all(code[2, :, 2:, :] == 1) and np.all(code[2, :, :, 6:] == 1)


@pytest.mark.slow
def test_identity_association_accepts_the_volume_model_on_frame_20():
    """The condition behind test_gpu_surface's tracking test (>= 0.8 of the emitted model points accepted by every
    association), checked where it is weakest, under the identity: config 1's source frame integrated by the oracle,
    the model sampled by surface_ref, associated with frame 20 by assoc_ref with the tracking defaults (plane mode,
    dist_max 0.05, cos_min 0.5, edge_max 0.03, normals given). The skin does not enter: on config 1 the 4σ = 0.4 m
    cut-off covers the whole sphere, so one identity node stands in for it (the warp is then exact)."""
    from occlusionfusion_amd import synthetic as S
    c = S.BASELINE_CONFIGS[1]
    scene, seed = S.config_scene(1)
    cam = S.bench_camera(c["cam_scale"])
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    D = (c["dims"],) * 3
    V = int(np.prod(D))
    origin = np.asarray(c["origin"], F32)
    tsdf, weight, color = np.ones(V, F32), np.zeros(V, F32), np.zeros(V, F32)
    d0 = S.frame_depth(scene, cam, seed, 0)
    fo.integrate(tsdf, weight, color, fo.world_points(origin, D, c["voxel"]), np.ones(V, bool), d0, None, intr,
                 with_color=False)
    a, w = np.zeros((V, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (V, 1))
    m = sr.surface_points(tsdf.reshape(D), weight.reshape(D), origin, c["voxel"], _all_bricks(D), a, w, 1.0, V)
    n = int(m["count"][1])
    assert n > 5000
    shares = {}
    for t in (5, 10, 20):
        vm = fo.backproject_depth(S.frame_depth(scene, cam, seed, t), *intr)
        code, _, _ = ar.gate(m["points"][:n], m["normals"][:n], m["anchors"][:n], m["weights"][:n], None,
                             np.tile(np.eye(3, dtype=F32), (4, 1, 1)), np.zeros((4, 3), F32), np.zeros((4, 3), F32),
                             intr, vm, dist_max=0.05, cos_min=0.5, edge_max=0.03, mode=ar.PLANE)
        shares[t] = float((code == 0).mean())
        print(f"frame {t}: {n} model points, identity association codes {np.bincount(code, minlength=7).tolist()}, "
              f"share {shares[t]:.4f}")
    assert shares[20] >= 0.8, shares
