"""GPU: the motion completion network in the tracking loop (FusionPipeline.track_step / Registration.track,
motion_net=), on config 1's camera, volume and graph with the occluder in the scene.

* motion_net=None is the loop as it is: bitwise the transforms of a call without the keyword;
* with a completer the result's "motion" equals the pieces called by hand, bitwise, and the final solve's motion term is
  exactly deformed_at_source + node_motion and confidence, the solves before it have none;
* after a frame tracked with the completer the default loop gives what it gives from that state without one.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_ref import load_weights  # noqa: E402

pytestmark = pytest.mark.gpu


def pyramid_from_nodes(nodes, edges):
    """A 4-level pyramid over the graph's own lists: every 4th node per level, 6 / 4 / 3 nearest neighbours."""
    pyd, idx = {"nn_index_l0": np.asarray(edges)}, np.arange(len(nodes))
    for l, k in ((1, 6), (2, 4), (3, 3)):
        keep = np.arange(0, len(idx), 4)
        pyd[f"down_sample_idx{l}"] = keep
        pyd[f"up_sample_idx{l}"] = np.minimum(np.arange(len(idx)) // 4, len(keep) - 1)
        idx = idx[keep]
        p = np.asarray(nodes, np.float64)[idx]
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d, np.inf)
        pyd[f"nn_index_l{l}"] = np.argsort(d, axis=1)[:, :min(k, len(idx) - 1)]
    return pyd


@pytest.fixture(scope="module")
def scene(cuda):
    from occlusionfusion_amd import synthetic as S
    c = S.BASELINE_CONFIGS[1]
    seq = S.SyntheticSequence.build(c["nodes"], cam=S.bench_camera(c["cam_scale"]), seed=c["seed"],
                                    scene=S.SphereScene(motion="nonrigid", occluder=True),
                                    coverage=S.config_coverage(1), graph="geodesic", device=cuda)
    return seq, pyramid_from_nodes(seq.nodes, seq.edges), load_weights()


def _pipeline(cuda, seq):
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.pipeline import FusionPipeline
    c = S.BASELINE_CONFIGS[1]
    pipe = FusionPipeline(seq, c["origin"], c["voxel"], (c["dims"],) * 3, n_matches=10000, device=cuda,
                          gn_params=dict(precond="direct"))
    pipe.integrate_source(pipe.prepare(0))
    return pipe


def _completer(cuda, scene):
    from occlusionfusion_amd.motion import MotionCompleter
    mc = MotionCompleter(scene[2], max_nodes=512, device=cuda)
    mc.set_graph(scene[1])
    return mc


def test_motion_net_none_is_the_loop_as_it_is(scene, cuda):
    seq = scene[0]
    a, b = _pipeline(cuda, seq), _pipeline(cuda, seq)
    oa = a.track_step(a.prepare(1), 1)
    ob = b.track_step(b.prepare(1), 1, motion_net=None)
    assert oa["valid_solve"] == ob["valid_solve"] == 1 and "motion" not in oa and "motion" not in ob
    assert oa["assoc"] == ob["assoc"]
    assert torch.equal(oa["node_rotations"], ob["node_rotations"])
    assert torch.equal(oa["node_translations"], ob["node_translations"])


def test_track_step_with_the_completer_equals_the_pieces(scene, cuda):
    seq = scene[0]
    pipe, mc = _pipeline(cuda, seq), _completer(cuda, scene)
    calls, optimize = [], pipe.solver.optimize

    def recording(*args, **kw):
        calls.append((args[3], args[4]))          # (target_node_pos, node_conf) of GaussNewtonSolver.optimize
        return optimize(*args, **kw)

    pipe.solver.optimize = recording
    out = pipe.track_step(pipe.prepare(1), 1, motion_net=mc)
    pipe.solver.optimize = optimize
    m = out["motion"]
    assert out["valid_solve"] == 1 and len(out["assoc"]) == 4 and len(calls) == 4
    assert set(m) == {"node_motion", "confidence", "visible", "status"} and int(m["status"].item()) == 0
    N = len(seq.nodes)
    assert m["node_motion"].shape == (N, 3) and m["confidence"].shape == (N,) and m["node_motion"].is_cuda
    assert bool((m["confidence"] > 0).all()) and bool((m["confidence"] <= 1).all())
    # by hand: the loop without a motion term, the previous frame's visible nodes, a fresh completer
    hand, fresh = _pipeline(cuda, seq), _pipeline(cuda, seq)
    visible = fresh.vol.check_visibility(torch.from_numpy(seq.nodes).to(cuda))[0]
    assert int(visible.sum()) >= 3        # (the graph was sampled from the source frame: that frame sees its nodes)
    first = hand.track_step(hand.prepare(1), 1, motion=False)
    nodes = torch.from_numpy(seq.nodes).to(cuda).double()
    mc2 = _completer(cuda, scene)
    nm, conf = mc2(nodes, nodes + first["node_translations"].double(), visible)
    assert torch.equal(m["visible"].cpu(), torch.from_numpy(visible))
    assert torch.equal(m["node_motion"], nm) and torch.equal(m["confidence"], conf)
    # the solves: three without a motion term, then one on deformed_at_source + node_motion / confidence
    assert all(c == (None, None) for c in calls[:3])
    assert torch.equal(calls[3][0], (nodes + nm).float()) and torch.equal(calls[3][1], conf.float())
    assert calls[3][0].dtype == torch.float32 and calls[3][1].dtype == torch.float32
    assert not torch.equal(out["node_translations"], first["node_translations"])
    # the default loop from this state is what a pipeline that never saw a completer gives from it
    rot, trans = pipe.prev_rot.clone(), pipe.prev_trans.clone()
    a = pipe.track_step(pipe.prepare(2), 2)
    other = _pipeline(cuda, seq)
    other.prev_rot, other.prev_trans, other.vol.frame_id = rot, trans, 1
    b = other.track_step(other.prepare(2), 2)
    assert a["valid_solve"] == b["valid_solve"] == 1 and "motion" not in a
    assert torch.equal(a["node_rotations"], b["node_rotations"])
    assert torch.equal(a["node_translations"], b["node_translations"])
    with pytest.raises(ValueError):
        pipe.track_step(pipe.prepare(3), 3, model="volume", motion_net=mc)


def test_registration_track_with_the_completer(scene, cuda):
    from types import SimpleNamespace
    from occlusionfusion_amd import EDGraph, TSDFVolume, WarpField
    from occlusionfusion_amd import synthetic as S
    from occlusionfusion_amd.registration import Registration
    seq = scene[0]
    c = S.BASELINE_CONFIGS[1]
    cam = seq.cam
    intr = (cam.fx, cam.fy, cam.cx, cam.cy)
    K = np.eye(3)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intr
    cp = seq.canonical_points
    pts = cp[np.sort(np.random.default_rng(5).choice(cp.shape[0], 8229, replace=False))]

    def make():
        vol = TSDFVolume.from_grid(c["origin"], c["voxel"], (c["dims"],) * 3, intr,
                                   SimpleNamespace(source_frame=0, skip_rate=1), device=cuda)
        graph = EDGraph(seq.nodes, seq.edges, seq.edge_weights, node_coverage=seq.node_coverage)
        wf = WarpField(graph, vol)
        vol.integrate({"im": seq.frame(0), "id": 0})
        return Registration(pts, graph, wf, K, precond="direct"), vol

    frame = {"im": seq.frame(3), "id": 3}
    (ra, _), (rb, _), (rc, vol) = make(), make(), make()
    a, b = ra.track(frame), rb.track(frame, motion_net=None)
    assert "motion" not in a and "motion" not in b
    assert np.array_equal(a["node_rotations"], b["node_rotations"])
    assert torch.equal(a["node_translations"], b["node_translations"])
    mc = _completer(cuda, scene)
    o = rc.track(frame, motion_net=mc)
    assert o["valid_solve"] == 1 and len(o["assoc"]) == 4 and int(o["motion"]["status"].item()) == 0
    assert torch.equal(o["motion"]["visible"].cpu(), torch.from_numpy(vol.get_visible_nodes()))
    nodes = torch.from_numpy(seq.nodes).to(cuda).double()
    nm, conf = _completer(cuda, scene)(nodes, nodes + a["node_translations"].to(cuda).double(), o["motion"]["visible"])
    assert torch.equal(o["motion"]["node_motion"], nm) and torch.equal(o["motion"]["confidence"], conf)
