"""CPU: closed-form known answers for the numpy restatement of ofx_associate (tests/assoc_ref.py): a fronto-parallel
plane, one constructed point per rejection code, and the even subsample rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_ref as ar  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
H, W = 32, 40
INTR = (30.0, 30.0, 19.5, 15.5)
# identity warp that is exact in f32: one node at the origin carries the whole weight, (x - 0) + 0 + 0 = x
NODES = np.zeros((4, 3), F32)
R_ID = np.tile(np.eye(3, dtype=F32), (4, 1, 1))
T_0 = np.zeros((4, 3), F32)


def _skin(P):
    return np.zeros((P, 4), np.int32), np.tile(np.array([1, 0, 0, 0], F32), (P, 1))


def _at(u, v, z):
    """The point of depth z on the ray of pixel (u, v)."""
    fx, fy, cx, cy = INTR
    return [(u - cx) * z / fx, (v - cy) * z / fy, z]


def _run(points, depth, normals=None, valid=None, **kw):
    pts = np.asarray(points, F32).reshape(-1, 3)
    a, w = _skin(pts.shape[0])
    vm = fo.backproject_depth(np.asarray(depth, F32), *INTR)
    return ar.associate(pts, normals, a, w, valid, R_ID, T_0, NODES, INTR, vm, **kw), vm


def test_plane_known_answers():
    depth = np.ones((H, W), F32)
    uv = [(u, v) for v in range(H) for u in range(W)]
    pts = np.array([_at(u, v, 1.02) for u, v in uv], F32)
    interior = np.array([0 < u < W - 1 and 0 < v < H - 1 for u, v in uv])
    for mode in (ar.PLANE, ar.POINT):
        out, vm = _run(pts, depth, mode=mode, max_matches=H * W)
        assert np.array_equal(out["warped"], pts)                       # the identity warp is exact
        assert np.array_equal(out["code"] == 0, interior)               # every interior point is accepted
        assert np.all(out["code"][~interior] == 4)                      # the border has no normal
        assert out["count"].tolist() == [int(interior.sum())] * 2
        assert np.array_equal(out["match_idx"], np.nonzero(interior)[0])
        t = out["tgt"][interior]
        if mode == ar.PLANE:   # the foot of x' on the plane z = 1: (x, y, 1) exactly
            assert np.array_equal(t, np.stack([pts[interior, 0], pts[interior, 1], np.ones(len(t), F32)], 1))
        else:                  # the pixel's vertex
            q = np.stack([vm[:, v, u] for (u, v), i in zip(uv, interior) if i])
            assert np.array_equal(t, q)
        assert np.all(out["tgt"][~interior] == 0)
    # n_q = (0, 0, -1) exactly: a normal of (0, 0, -1) has cosine 1 and passes cos_min = 1, its opposite fails any
    n = np.tile(np.array([0, 0, -1], F32), (len(pts), 1))
    out, _ = _run(pts, depth, normals=n, cos_min=1.0)
    assert np.array_equal(out["code"] == 0, interior)
    out, _ = _run(pts, depth, normals=-n, cos_min=-0.999)
    assert np.all(out["code"][interior] == 6)


def test_each_rejection_code():
    depth = np.ones((H, W), F32)
    depth[10, 10] = 0.0          # a hole
    depth[:, 30:] = 1.05         # a 5 cm depth step between columns 29 and 30
    cases = [
        (_at(5, 5, 1.02), [0, 0, -1], 1, 0),       # accepted
        (_at(5, 5, 1.02), [0, 0, -1], 0, 1),       # valid == 0
        (_at(5, 5, -1.0), [0, 0, -1], 1, 2),       # behind the camera
        ([5.0, 0.0, 1.0], [0, 0, -1], 1, 2),       # off the image
        ([np.nan, 0.0, 1.0], [0, 0, -1], 1, 2),    # non-finite
        (_at(10, 10, 1.02), [0, 0, -1], 1, 3),     # the hole pixel
        (_at(11, 10, 1.02), [0, 0, -1], 1, 4),     # a 4-neighbour is the hole
        (_at(0, 7, 1.02), [0, 0, -1], 1, 4),       # the image border
        (_at(29, 20, 1.02), [0, 0, -1], 1, 4),     # the 5 cm step against edge_max = 3 cm, from the near side
        (_at(30, 20, 1.04), [0, 0, -1], 1, 4),     # and from the far side
        (_at(18, 14, 1.06), [0, 0, -1], 1, 5),     # 6 cm off against dist_max = 5 cm
        (_at(5, 5, 1.02), [0, 0, 1], 1, 6),        # a back-facing normal
        (_at(33, 20, 1.04), [0, 0, -1], 1, 0),     # accepted on the far plane
    ]
    pts = np.array([c[0] for c in cases], F32)
    nrm = np.array([c[1] for c in cases], F32)
    valid = np.array([c[2] for c in cases], np.uint8)
    want = np.array([c[3] for c in cases], np.uint8)
    out, _ = _run(pts, depth, normals=nrm, valid=valid, dist_max=0.05, cos_min=0.5, edge_max=0.03, mode=ar.PLANE)
    assert out["code"].tolist() == want.tolist()
    assert set(want.tolist()) == set(range(7))
    assert np.all(out["tgt"][want != 0] == 0)
    assert out["match_idx"].tolist() == [0, len(cases) - 1] and out["count"].tolist() == [2, 2]
    assert np.array_equal(out["tgt_out"][:, 2], np.array([1.0, 1.05], F32))
    assert np.array_equal(out["warped"][1], pts[1])                      # an invalid point keeps its position
    # without normals the back-facing point passes; a 6 cm depth tolerance lets the far point through
    out, _ = _run(pts, depth, normals=None, valid=valid, dist_max=0.07)
    assert out["code"].tolist() == [0 if c in (5, 6) else c for c in want.tolist()]


def test_an_anchor_outside_the_graph_is_invalid_skin():
    depth = np.ones((H, W), F32)
    pts = np.array([_at(5, 5, 1.02)] * 3, F32)
    a, w = _skin(3)
    a[1, 3], a[2, 0] = -1, 4
    vm = fo.backproject_depth(depth, *INTR)
    out = ar.associate(pts, None, a, w, None, R_ID, T_0, NODES, INTR, vm)
    assert out["code"].tolist() == [0, 1, 1] and np.array_equal(out["warped"], pts)


@pytest.mark.parametrize("m", [1, 7, 1000])
def test_subsample_rule(m):
    for n in (0, 1, m - 1, m):
        assert np.array_equal(ar.emitted_ranks(n, m), np.arange(max(n, 0)))    # n <= max_matches: everything
    for n in (m + 1, 2 * m - 1, 7 * m + 3):
        if n <= m:
            continue
        r = ar.emitted_ranks(n, m)
        assert len(r) == m and np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] == n - 1
        # even: any two gaps between neighbours differ by at most one rank
        gaps = np.diff(np.concatenate([[-1], r]))
        assert gaps.max() - gaps.min() <= 1
        # the rule itself, one rank at a time in Python integers
        assert r.tolist() == [k for k in range(n) if ((k + 1) * m) // n > (k * m) // n]
    assert len(ar.emitted_ranks(5, 0)) == 0
