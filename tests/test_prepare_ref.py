"""CPU: the numpy restatement of ofx_prepare_depth (tests/prepare_ref.py) — known answers, the edge rule (a skipped tap
is a hole, so nothing bleeds across a depth edge), the denoising it buys on config 1's frame 20 against the noise-free
render, and holes preserved on that frame and on the reference's own real pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prepare_ref as pr  # noqa: E402
from oracle import fusion_oracle as fo  # noqa: E402

F32 = np.float32
INTR = (30.0, 30.0, 19.5, 15.5)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def test_plane_with_holes_is_exact():
    d = np.ones((32, 40), F32)
    d[12:17, 8:13] = 0.0
    for r in (1, 3, 4):
        out = pr.prepare(d, INTR, radius=r)
        assert np.array_equal(_bits(out["depth"]), _bits(d))           # exactly 1.0 at valid pixels, exactly 0 at holes
        n = out["normals"]
        hole = d == 0
        near = np.zeros_like(hole)                                     # a hole, a 4-neighbour of one, or the border
        near[1:-1, 1:-1] = hole[1:-1, 1:-1] | hole[:-2, 1:-1] | hole[2:, 1:-1] | hole[1:-1, :-2] | hole[1:-1, 2:]
        near[0, :] = near[-1, :] = near[:, 0] = near[:, -1] = True
        assert np.all(n[:, near] == 0)
        assert np.all(n[0][~near] == 0) and np.all(n[1][~near] == 0) and np.all(n[2][~near] == -1)
        assert (~near).sum() > 900


def test_radius_0_is_the_input_and_the_oracle_vertex_map():
    rng = np.random.default_rng(3)
    d = (1.0 + 0.3 * rng.random((17, 33))).astype(F32)
    d[rng.random(d.shape) < 0.1] = 0.0
    d[2, 3], d[5, 7], d[9, 9] = np.nan, -1.0, 1e-41                     # NaN and negative: holes; a subnormal: valid
    out = pr.prepare(d, INTR, radius=0)
    want = np.where(d > 0, d, F32(0))
    assert np.array_equal(_bits(out["depth"]), _bits(want))
    assert np.array_equal(_bits(out["point_image"]), _bits(fo.backproject_depth(d, *INTR)))
    mm = (1000.0 * want).astype(np.uint16)
    out = pr.prepare(mm, INTR, radius=0)
    assert np.array_equal(_bits(out["depth"]), _bits(mm.astype(F32) / F32(1000.0)))
    assert np.array_equal(_bits(out["point_image"]), _bits(fo.backproject_depth(mm, *INTR)))


def test_nothing_bleeds_across_a_depth_edge():
    """A 5 cm step and range_cut 3 cm: the image filters bit for bit as its two halves filtered separately with the
    other half zeroed, because a skipped tap behaves exactly like a hole."""
    rng = np.random.default_rng(11)
    u, v = np.meshgrid(np.arange(40.0), np.arange(32.0))
    d = (1.0 + 0.002 * (u - 19.5) + 0.004 * np.sin(0.3 * v) + rng.normal(0, 0.001, u.shape)).astype(F32)
    d[:, 22:] += F32(0.05)
    d[5:8, 4:7] = 0.0
    left, right = d.copy(), d.copy()
    left[:, 22:] = 0.0
    right[:, :22] = 0.0
    for r in (1, 3, 4):
        kw = dict(radius=r, sigma_s=2.0, sigma_r=0.01, range_cut=0.03)
        whole = pr.bilateral(d, **kw)
        halves = pr.bilateral(left, **kw) + pr.bilateral(right, **kw)   # disjoint supports: the sum joins them
        assert np.array_equal(_bits(whole), _bits(halves))
        assert not np.array_equal(_bits(whole), _bits(d))               # and it did filter
        wide = pr.bilateral(d, radius=r, sigma_s=2.0, sigma_r=0.05, range_cut=0.2)
        assert not np.array_equal(_bits(wide), _bits(halves))           # a cut above the step does bleed


@pytest.fixture(scope="module")
def frame20():
    intr, noisy, clean = pr.config1_frame(20)
    return intr, noisy, pr.clean_reference(clean, intr)


def test_denoising_on_config_1_frame_20(frame20):
    intr, noisy, ref = frame20
    raw = pr.prepare(noisy, intr, radius=0)
    filt = pr.prepare(noisy, intr, radius=3, sigma_s=2.0, sigma_r=0.01)
    assert ref["points"].shape[0] == 8640
    pr.check_denoising(pr.measures(raw["depth"], raw["point_image"], raw["normals"], ref, intr),
                       pr.measures(filt["depth"], filt["point_image"], filt["normals"], ref, intr))


def test_holes_are_preserved(frame20, golden_dir):
    intr, noisy, _ = frame20
    assert np.array_equal(pr.bilateral(noisy) > 0, noisy > 0) and (noisy == 0).any()
    g = np.load(os.path.join(golden_dir, "moose.npz"), allow_pickle=False)
    for k in ("src_mm", "tgt_mm"):
        mm = g[k]
        assert (mm == 0).any() and (mm > 0).any()
        assert np.array_equal(pr.bilateral(mm) > 0, mm > 0)
