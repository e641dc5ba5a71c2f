"""deepim.core.tracker.Tracker with TEST.TRACK_OCCLUSION on the device: P = 2 objects of one small mesh through 8 frames of
lib.dataset.synthetic_sequences, the pose head zeroed as in tests/test_gpu_tracker.py, so that the tracked pose is the prediction.

  the scene        an untracked occluder hides object 0 in frames 3 to 5 (its preconditions are asserted on the scene itself)
  control          without occlusion reasoning, and with the ZNCC score on, object 0 is LOST in those frames
  "depth"          it is OCCLUDED instead, coasts on the exact motion model, and is back at frame 6 with its velocity and its ring
  the budget       TRACK_MAX_OCCLUDED 2: frame 5 is OCCLUDED | LOST, with an offered pose also REINIT
  "tracks"         one track teleported onto the other: counts against numpy on the read-back render, the score over the visible
                   pixels against tests/hyp_reference.py
  plumbing         eager and graph-replayed runs agree bit for bit; "none" launches neither new op; "depth" needs depth frames"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hyp_reference as hr  # noqa: E402
import track_occ_reference as O  # noqa: E402
from ops_trace import OpsTrace  # noqa: E402
from test_gpu_tracker import MODEL_SEED, P, _cfg, _host, _observed, _tracker  # noqa: E402

DEV = "cuda:0"
FRAMES = 8
HIDDEN = (3, 4, 5)
# object 0 (0.73 m away, 0.21 m across), from frame 3 up to frame 6: the same mesh 0.35 m nearer (2.7 times as large in the image, its
# nearest point still behind ZNEAR = 0.25), centred on the object
OCCLUDER = ("occluder", 3, 6, 0, 0.35, 0.0, 0)
SEED = 8
STATE = ("hist", "age", "ring", "ring_n", "ring_pos", "occ_age", "occluder_ok")


def _occ_cfg(**track):
    return _cfg(test_iter=2, motion="velocity", damping=1.0, score="rgb", **track)


def _sequence(cfg, frames, seed, events=()):
    from lib.dataset.synthetic_sequences import SyntheticSequence

    return SyntheticSequence(cfg, frames, P, seed, device=DEV, events=events, subdiv=3, model_seed=MODEL_SEED)


def _render(seq, poses):
    rm = seq.render_machine
    dep = torch.empty((P, 1, rm.height, rm.width), device=DEV)
    rm.render_batch(torch.from_numpy(seq.class_index).to(DEV), torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(DEV), depth=dep)
    return dep


@pytest.fixture(scope="module")
def occluder_scene(hip_lib):
    """the video with the occluder, and the checks of the scene itself, from dim_track_visibility at the true poses against each
    frame's depth: at most 5 % of object 0 visible in frames 3 to 5, all of it outside them, all of object 1 throughout"""
    from lib.hip import ops

    cfg = _occ_cfg()
    seq = _sequence(cfg, FRAMES, SEED, events=[OCCLUDER])
    frames = [seq.frame(t) for t in range(FRAMES)]
    assert (seq.pose_gt[:, 0, 2, 3] - OCCLUDER[4] - 0.11 > float(cfg.dataset.ZNEAR)).all()
    counts = []
    for t in range(FRAMES):
        depth_frame = frames[t]["depth_raw"].view(torch.int16).to(torch.float32) / float(cfg.dataset.DEPTH_FACTOR)
        counts.append(_host(ops.track_visibility(_render(seq, seq.pose_gt[t]), "depth", cfg.TEST.TRACK_OCC_DELTA, depth_frame=depth_frame)[1]))
    counts = np.stack(counts)
    print("set-up counts of object 0:", counts[:, 0].tolist())
    assert (counts[:, :, 0] > 5000).all() and not counts[:, :, 2].any(), counts
    for t in range(FRAMES):
        if t in HIDDEN:
            assert counts[t, 0, 1] <= 0.05 * counts[t, 0, 0], ("set-up: the occluder leaves too much of object 0 visible", t, counts[t])
        else:
            assert counts[t, 0, 1] == counts[t, 0, 0], ("set-up: object 0 is hidden outside the occluder's frames", t, counts[t])
        assert counts[t, 1, 1] == counts[t, 1, 0], ("set-up: object 1 is hidden", t, counts[t])
    return seq, frames, counts


def _run(seq, frames, graph, offer=None, **track):
    """-> (per-frame outputs on the host, per-frame state on the host, tracker)"""
    cfg = _occ_cfg(**track)   # (the configuration is one global object: set again for every tracker)
    tr, _ = _tracker(cfg, "zero", seq, graph)
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    outs, states = [], []
    for t, fr in enumerate(frames):
        kw = {}
        if offer is not None:
            kw = dict(reinit_pose=fr["pose_gt"], reinit_valid=None if offer else torch.zeros(P, dtype=torch.int32))
        out = tr.step(fr["frame_bgr"], depth_raw=fr["depth_raw"] if tr.needs_depth else None, **kw)
        outs.append({k: (None if v is None else _host(v)) for k, v in out.items()})
        states.append({k: _host(getattr(tr, k)) for k in STATE})
    return outs, states, tr


def _flags(outs):
    return np.stack([o["flags"] for o in outs])


def test_control_without_occlusion_reasoning_the_hidden_object_is_lost(occluder_scene):
    from lib.hip import ops

    seq, frames, _ = occluder_scene
    outs, states, tr = _run(seq, frames, True)
    flags = _flags(outs)
    print("flags:", flags.tolist(), "scores of object 0:", [float(o["score"][0]) for o in outs])
    assert tr.cfg.TEST.TRACK_OCCLUSION == "none" and all(o["visible"] is None and o["counts"] is None and o["pose_track"] is None for o in outs)
    assert not flags[:3].any() and not flags[:, 1].any(), flags
    assert (flags[3:6, 0] & ops.STATUS_TRACK_LOST).all() and not (flags & ops.STATUS_TRACK_OCCLUDED).any(), flags
    assert all(outs[t]["score"][0] < tr.cfg.TEST.TRACK_MIN_SCORE for t in HIDDEN)
    assert states[5]["age"][0] == 1 and not states[5]["occ_age"].any() and states[5]["occluder_ok"].tolist() == [1, 1]   # untouched state


def test_depth_occlusion_coasts_through_the_hidden_frames(occluder_scene):
    from lib.hip import ops

    seq, frames, scene_counts = occluder_scene
    outs, states, tr = _run(seq, frames, True, occlusion="depth")
    flags = _flags(outs)
    LOST, OCC = ops.STATUS_TRACK_LOST, ops.STATUS_TRACK_OCCLUDED
    print("flags:", flags.tolist(), "visible:", [o["visible"].tolist() for o in outs], "scores:", [o["score"].tolist() for o in outs])
    assert not flags[:, 1].any() and not flags[:3].any() and not flags[6:].any(), flags          # object 1 never, object 0 only when hidden
    for t in HIDDEN:
        assert flags[t, 0] & OCC and not flags[t, 0] & (LOST | ops.STATUS_TRACK_REINIT), (t, flags)
        assert states[t]["ring_n"][0] == states[2]["ring_n"][0] == 3 and states[t]["ring_pos"][0] == states[2]["ring_pos"][0], t
        assert states[t]["ring"][0].tobytes() == states[2]["ring"][0].tobytes(), t
        assert states[t]["occ_age"][0] == t - 2 and states[t]["age"][0] == 2 and outs[t]["visible"][0] <= 0.05
        assert states[t]["hist"][0, 1].tobytes() == outs[t]["pose_track"][0].tobytes()
    # the tracked pose is the true one to 1e-5, so the tracker's own counts show the scene's preconditions too (a silhouette pixel may differ)
    counts = np.stack([o["counts"] for o in outs])
    assert np.abs(counts[:, :, 0] - scene_counts[:, :, 0]).max() <= 20, (counts[:, :, 0], scene_counts[:, :, 0])
    assert (counts[3:6, 0, 1] <= 0.05 * counts[3:6, 0, 0]).all() and np.array_equal(counts[:3, :, 1], counts[:3, :, 0])
    assert np.array_equal(counts[6:, :, 1], counts[6:, :, 0]) and np.array_equal(counts[:, 1, 1], counts[:, 1, 0]) and not counts[:, :, 2].any()
    err = np.stack([np.abs(o["pose_track"].astype(np.float64) - seq.pose_gt[t]).max(axis=(1, 2)) for t, o in enumerate(outs)])
    print("max |pose_track - ground truth| per frame and object:", err.tolist())
    assert err.max() <= 1e-5, err
    # frame 6: back, with its velocity, a fresh budget and a score over the whole render again
    assert flags[6, 0] == 0 and states[6]["age"][0] == 2 and states[6]["occ_age"][0] == 0
    assert outs[6]["score"][0] >= tr.cfg.TEST.TRACK_MIN_SCORE and outs[6]["visible"][0] == 1.0
    assert states[6]["ring_n"][0] == 4 and states[6]["ring_pos"][0] == (states[2]["ring_pos"][0] + 1) % tr.settings["window"]
    assert all(s["occluder_ok"].tolist() == [1, 1] for s in states)
    assert all(o["visible"][1] == 1.0 for o in outs)


@pytest.mark.parametrize("offer", [True, False], ids=["reinit", "no-reinit"])
def test_the_occlusion_budget_runs_out(occluder_scene, offer):
    from lib.hip import ops

    seq, frames, _ = occluder_scene
    outs, states, tr = _run(seq, frames, True, offer=offer, occlusion="depth", max_occluded=2)
    flags = _flags(outs)
    LOST, REINIT, OCC = ops.STATUS_TRACK_LOST, ops.STATUS_TRACK_REINIT, ops.STATUS_TRACK_OCCLUDED
    print("flags:", flags.tolist())
    assert not flags[:, 1].any() and not flags[:3].any()
    track_bits = flags[:, 0] & (OCC | LOST | REINIT)   # (a score over too few visible pixels may add DIM_STATUS_HYP_NO_SCORE)
    assert track_bits[3] == track_bits[4] == OCC and states[4]["occ_age"][0] == 2
    assert track_bits[5] == (OCC | LOST | REINIT if offer else OCC | LOST), flags
    assert states[5]["occ_age"][0] == 0
    if offer:
        assert states[5]["hist"][0, 1].tobytes() == seq.pose_gt[5, 0].tobytes() == outs[5]["pose_track"][0].tobytes()
        assert states[5]["age"][0] == 1 and states[5]["ring_n"][0] == 0 and states[5]["occluder_ok"].tolist() == [1, 1]
    else:
        assert states[5]["hist"][0].tobytes() == states[4]["hist"][0].tobytes() and states[5]["age"][0] == 1
        assert states[5]["occluder_ok"].tolist() == [0, 1]


def test_tracks_hide_each_other(hip_lib):
    """object 1 teleported onto object 0 from two frames before the video on: one constant-velocity trajectory on top of another.
    Object 1 is 0.24 m farther away, so it is the hidden one"""
    seed, event = 5, ("teleport", -2, 1, -183.0, -51.0)
    seq = _sequence(_occ_cfg(), 3, seed, events=[event])
    assert seq.pose_gt[0, 1, 2, 3] - seq.pose_gt[0, 0, 2, 3] > 0.2
    frames = [seq.frame(t) for t in range(3)]
    cfg = _occ_cfg(occlusion="tracks")
    tr, _ = _tracker(cfg, "zero", seq, False)
    assert not tr.needs_depth
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    for t, fr in enumerate(frames):
        out = tr.step(fr["frame_bgr"])
        depth_sc, counts, score = _host(tr.depth_sc), _host(out["counts"]), _host(out["score"])
        want_vis, want_counts = O.visibility(depth_sc, None, None, "tracks", cfg.TEST.TRACK_OCC_DELTA)
        assert np.array_equal(counts, want_counts), (t, counts, want_counts)
        assert _host(tr.depth_visible).tobytes() == want_vis.tobytes(), t
        assert counts[1, 2] > 1000 and counts[0, 2] == 0 and not counts[:, 3].any(), counts
        assert np.abs(_host(out["pose_track"]).astype(np.float64) - seq.pose_gt[t]).max() <= 1e-5
        obs, img, bbox = _host(_observed(cfg, fr)), _host(tr.image_sc), _host(tr.bbox_sc)
        for p in range(P):
            want = hr.score_one("rgb", obs[p], img[p], want_vis[p, 0], bbox[p])
            whole = hr.score_one("rgb", obs[p], img[p], depth_sc[p, 0], bbox[p])
            print("frame {} object {}: score {:.6f}, reference over the visible pixels {:.6f}, over the whole render {:.6f}".format(
                t, p, score[p], want, whole))
            assert abs(score[p] - want) <= 1e-5, (t, p, score[p], want)
        assert whole < want - 0.1, "set-up: the hidden part does not change object 1's score: the masked score guards nothing"
        assert _host(out["visible"]).tobytes() == (counts[:, 1].astype(np.float64) / counts[:, 0]).astype(np.float32).tobytes()


def test_eager_and_graph_runs_agree_bit_for_bit(occluder_scene):
    seq, frames, _ = occluder_scene
    eager = _run(seq, frames, False, offer=True, occlusion="both", max_occluded=2)
    graph = _run(seq, frames, True, offer=True, occlusion="both", max_occluded=2)
    assert eager[2].graph is None and graph[2].graph is not None
    for t in range(FRAMES):
        for k, v in eager[0][t].items():
            assert v.tobytes() == graph[0][t][k].tobytes(), (t, k)
        for k, v in eager[1][t].items():
            assert v.tobytes() == graph[1][t][k].tobytes(), (t, k)
    assert _flags(eager[0])[5, 0] & 16384    # the run went through the occluded state


def test_the_chain_with_and_without_occlusion(occluder_scene):
    seq, frames, _ = occluder_scene
    new_ops = ("track_visibility", "track_update_occ")
    tr, _ = _tracker(_occ_cfg(), "zero", seq, False)
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    with OpsTrace() as trace:
        tr.step(frames[0]["frame_bgr"])
    names = [c[0] for c in trace.calls]
    assert not any(n in new_ops or n.startswith("track_visibility") for n in names) and names[-2:] == ["pose_score", "track_update"], names
    tr, _ = _tracker(_occ_cfg(occlusion="depth"), "zero", seq, False)
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    with OpsTrace() as trace:
        tr.step(frames[0]["frame_bgr"], depth_raw=frames[0]["depth_raw"])
    names = [c[0] for c in trace.calls]
    assert names[-3:] == ["track_visibility", "pose_score", "track_update_occ"] and "track_update" not in names, names
    # without a score the render of the tracked pose is still made
    tr, _ = _tracker(_cfg(test_iter=2, score="none", occlusion="tracks"), "zero", seq, False)
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    with OpsTrace() as trace:
        out = tr.step(frames[0]["frame_bgr"])
    names = [c[0] for c in trace.calls]
    assert names[-2:] == ["track_visibility", "track_update_occ"] and "pose_score" not in names and out["score"] is None, names
    assert (_host(out["counts"])[:, 0] > 5000).all()


@pytest.mark.parametrize("mode", ["depth", "both"])
def test_depth_occlusion_needs_depth_frames(occluder_scene, mode):
    seq, frames, _ = occluder_scene
    tr, _ = _tracker(_occ_cfg(occlusion=mode), "zero", seq, False)
    assert tr.needs_depth
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    with pytest.raises(ValueError, match="depth_raw"):
        tr.step(frames[0]["frame_bgr"])
