"""No GPU: the numpy restatement of the tracker's occlusion kernels checks itself (tests/track_occ_reference.py) -- the O(P^2)
definition of "hidden by a track" against the two-minimum form the kernel computes, the scripted table of the occluded state, and
its equality with tests/track_reference.py when nothing can be occluded --, the TEST.TRACK_OCC* settings name what they refuse, the
synthetic video's occluder event, and the two C entry points return DIM_ERR_ARG before anything is enqueued."""
import ctypes

import numpy as np
import pytest

import track_occ_reference as O
import track_reference as R


# ---------------------------------------------------------------- visibility
@pytest.mark.parametrize("mode", ["tracks", "depth", "both"])
@pytest.mark.parametrize("P,H,W", [(1, 4, 8), (2, 6, 9), (3, 16, 16), (5, 16, 16), (17, 8, 8)])
def test_definition_equals_the_two_minimum_form(P, H, W, mode):
    rng = np.random.RandomState(100 * P + W)
    for delta in (0.0, 0.015, 0.015625, 0.25):   # (the last two are exact next to the base depths: "exactly delta apart" occurs)
        depth, frame = O.boundary_planes(rng, P, H, W, delta)
        for ok in (None, (rng.rand(P) < 0.6).astype(np.int32)):
            a_vis, a_cnt = O.visibility(depth, frame, ok, mode, delta)
            b_vis, b_cnt = O.visibility_two_min(depth, frame, ok, mode, delta)
            assert a_vis.tobytes() == b_vis.tobytes() and np.array_equal(a_cnt, b_cnt), (delta, ok)
            assert np.array_equal(a_cnt[:, 0], a_cnt[:, 1:].sum(1))
            assert np.array_equal(a_cnt[:, 0], O.drawn(depth).sum((1, 2, 3)))
            keep = a_vis != 0
            assert a_vis[keep].tobytes() == depth[keep].tobytes() and not np.signbit(a_vis[~keep]).any()   # d's bits, or +0.0
            if mode == "tracks":
                assert not a_cnt[:, 3].any()
            if mode == "depth":
                assert not a_cnt[:, 2].any()
            if P == 1:
                assert not a_cnt[:, 2].any()   # a lone track is never hidden by tracks


def test_boundary_planes_hold_the_boundaries():
    """ties, exactly delta apart, one float32 step either side, and everything that is not drawn"""
    delta = np.float32(0.015625)
    depth, frame = O.boundary_planes(np.random.RandomState(0), 3, 32, 32, delta)
    d = depth[:, 0]
    diff = (d[0] - d[1]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        both = O.drawn(d[0]) & O.drawn(d[1])
        assert (both & (diff == 0)).any() and (both & (diff == delta)).any()
        assert (both & (diff > delta) & (diff < delta * np.float32(1.0001))).any()
        assert (both & (diff < delta) & (diff > delta * np.float32(0.9999))).any()
    assert np.isnan(depth).any() and np.isinf(depth).any() and (depth == 0).any() and (depth < 0).any()
    assert np.isnan(frame).any() and (frame == 0).any()


def test_visibility_rules_on_a_hand_made_pixel_row():
    delta = np.float32(0.015625)   # 0.5 + delta is exact, and so are the differences below
    up, down = np.nextafter(np.float32(0.5) + delta, np.float32(1)), np.nextafter(np.float32(0.5) + delta, np.float32(0))
    #                 tie    = delta          1 ulp more  1 ulp less  q not drawn  p not drawn
    near = np.array([0.5, 0.5, 0.5, 0.5, np.nan, 0.5], np.float32)
    far = np.array([0.5, np.float32(0.5) + delta, up, down, 0.9, -1.0], np.float32)
    depth = np.stack([near, far]).reshape(2, 1, 1, 6)
    vis, cnt = O.visibility(depth, None, None, "tracks", delta)
    assert (vis[1, 0, 0] != 0).tolist() == [True, True, False, True, True, False]
    assert (vis[0, 0, 0] != 0).tolist() == [True, True, True, True, False, True]
    assert cnt.tolist() == [[5, 5, 0, 0], [5, 4, 1, 0]]
    # a track whose occluder_ok is 0 hides nobody, and can still be hidden
    vis, cnt = O.visibility(depth, None, np.array([0, 1], np.int32), "tracks", delta)
    assert cnt.tolist() == [[5, 5, 0, 0], [5, 5, 0, 0]]
    vis, cnt = O.visibility(depth[::-1], None, np.array([0, 1], np.int32), "tracks", delta)
    assert cnt.tolist() == [[5, 4, 1, 0], [5, 5, 0, 0]]
    # the frame's depth: a pixel without a reading hides nothing; hidden by both counts as hidden by a track
    frame = np.array([0.4, 0.0, np.nan, 0.4, 0.4, 0.4], np.float32).reshape(1, 6)
    vis, cnt = O.visibility(depth, frame, None, "both", delta)
    assert cnt.tolist() == [[5, 2, 0, 3], [5, 1, 1, 3]]


# ---------------------------------------------------------------- the state machine
def test_the_occlusion_table_reaches_every_branch():
    T = O.OCC_TABLE
    frames = O.occ_table()
    assert len(frames) == T["frames"] == 12 and frames[0]["pose_new"].shape == (7, 3, 4)
    assert np.float64(np.float32(T["min_visible"])) == 0.25
    rows = O.run_table(frames)
    P = T["tracks"]
    for bit, want in ((O.OCCLUDED, O.EXPECT_OCCLUDED), (O.LOST, O.EXPECT_LOST), (O.REINIT, O.EXPECT_REINIT)):
        got = {p: [f for f, r in enumerate(rows) if r[0]["flags"][p] & bit] for p in range(P)}
        assert got == want, (bit, got)
    st = lambda f: rows[f][1]      # noqa: E731
    out = lambda f: rows[f][0]     # noqa: E731
    # track 0: exactly min_visible of it is not occluded; visible is the fraction
    assert out(6)["flags"][0] == 0 and out(6)["visible"][0] == np.float32(0.25) and out(0)["visible"][0] == 1
    # track 1: coasting at age 1 and at age 2 -- the history takes pose_pred bit for bit, the ring does not move
    assert st(0)["age"][1] == 2 and st(0)["occ_age"][1] == 1 and st(0)["ring_n"][1] == 0 and st(0)["ring_pos"][1] == 0
    assert st(0)["hist"][1, 1].tobytes() == frames[0]["pose_pred"][1].tobytes()
    assert st(0)["hist"][1, 0].tobytes() == frames[0]["pose_before"][1].tobytes()      # what the fresh state held
    assert st(1)["age"][1] == 2 and st(1)["occ_age"][1] == 2
    assert st(1)["hist"][1, 0].tobytes() == frames[0]["pose_pred"][1].tobytes() and st(1)["hist"][1, 1].tobytes() == frames[1]["pose_pred"][1].tobytes()
    assert np.array_equal(out(1)["mean"][1], [0, 0]) and out(1)["step"][1, 0] > 0.5     # nothing stored: mean 0; the step is still reported
    # ... the budget is spent without an offer: rule 6 (history kept, no velocity), the estimate stays the last coasted pose
    assert out(2)["flags"][1] == O.OCCLUDED | O.LOST and st(2)["age"][1] == 1 and st(2)["occ_age"][1] == 0
    assert st(2)["hist"][1].tobytes() == st(1)["hist"][1].tobytes() and out(2)["occluder_ok"][1] == 0
    assert out(2)["pose_track"][1].tobytes() == frames[1]["pose_pred"][1].tobytes()
    assert st(3)["occ_age"][1] == 1 and out(3)["occluder_ok"][1] == 1
    assert out(4)["flags"][1] == 0 and st(4)["occ_age"][1] == 0 and st(4)["ring_n"][1] == 1   # recovered: the first step enters the ring
    # track 2: a coasting track does not look at its score; the budget is spent with an offer: rule 5
    assert out(3)["flags"][2] == out(4)["flags"][2] == O.OCCLUDED and st(4)["ring_n"][2] == 3
    assert out(5)["flags"][2] == O.OCCLUDED | O.LOST | O.REINIT and out(5)["occluder_ok"][2] == 1
    assert st(5)["hist"][2, 1].tobytes() == frames[5]["reinit_pose"][2].tobytes() == out(5)["pose_track"][2].tobytes()
    assert st(5)["age"][2] == 1 and st(5)["ring_n"][2] == 0 and not st(5)["ring"][2].any() and st(5)["occ_age"][2] == 0
    # track 3: fatal wins while hidden
    assert out(4)["flags"][3] == R.REN_BOX_EMPTY | O.LOST and st(4)["occ_age"][3] == 0 and st(4)["ring_pos"][3] == (st(3)["ring_pos"][3] + 1) % 3
    # track 4: a bad prediction while hidden is lost at once, budget or not
    assert out(2)["flags"][4] == out(7)["flags"][4] == O.OCCLUDED | O.LOST and st(2)["occ_age"][4] == 0
    assert st(2)["hist"][4].tobytes() == st(1)["hist"][4].tobytes()
    assert out(8)["flags"][4] == O.OCCLUDED and st(8)["occ_age"][4] == 1
    # track 5: nothing drawn is not occluded; the gap of frames 6-7 leaves the ring where it was, the recovery resets occ_age
    assert out(3)["flags"][5] == 0 and out(3)["visible"][5] == 0 and st(3)["ring_n"][5] == 3
    assert st(7)["ring_pos"][5] == st(5)["ring_pos"][5] and st(7)["ring"][5].tobytes() == st(5)["ring"][5].tobytes() and st(7)["occ_age"][5] == 2
    assert out(7)["mean"][5].tobytes() == out(5)["mean"][5].tobytes()                    # the mean of what is stored
    assert out(8)["flags"][5] == 0 and st(8)["occ_age"][5] == 0 and st(8)["age"][5] == 2
    assert st(8)["ring_pos"][5] == (st(5)["ring_pos"][5] + 1) % 3
    assert st(8)["hist"][5, 0].tobytes() == frames[7]["pose_pred"][5].tobytes() and st(8)["hist"][5, 1].tobytes() == frames[8]["pose_new"][5].tobytes()
    # track 6: the hidden frames do not fill the ring: the window rule bites at frame 4, not at frame 2
    assert [int(st(f)["ring_n"][6]) for f in range(5)] == [1, 1, 1, 2, 3]
    # the negative control: a reference whose coasting tracks push their step changes the flags somewhere
    other = O.run_table(frames, coast_pushes_ring=True)
    assert any(not np.array_equal(a[0]["flags"], b[0]["flags"]) for a, b in zip(rows, other))


@pytest.mark.parametrize("counts", ["visible", "hidden"])
def test_min_visible_zero_is_the_plain_update(counts):
    """track_reference's own table through the new update: nothing can be occluded with min_visible = 0 (whatever the counts say) or
    with everything visible (whatever min_visible says), and every shared tensor is the plain update's exactly"""
    frames = R.scripted_table()
    if counts == "hidden":
        frames = [dict(fr, counts=np.tile(np.array([50, 0, 50, 0], np.int32), (6, 1))) for fr in frames]
    T = dict(R.TABLE, max_occluded=3)
    rows = O.run_table(frames, T, min_visible=0.0 if counts == "hidden" else 1.0)
    want = R.run_table(R.scripted_table())
    for f, ((o, st), (w_flags, w_step, w_mean, w_st)) in enumerate(zip(rows, want)):
        assert np.array_equal(o["flags"], w_flags), f
        assert o["step"].tobytes() == w_step.tobytes() and o["mean"].tobytes() == w_mean.tobytes(), f
        for k, v in w_st.items():
            assert st[k].tobytes() == v.tobytes(), (f, k)
        assert not st["occ_age"].any()
        assert o["pose_track"].tobytes() == w_st["hist"][:, 1].tobytes()
        lost_for_good = ((w_flags & R.LOST) != 0) & ((w_flags & R.REINIT) == 0)
        assert np.array_equal(o["occluder_ok"], 1 - lost_for_good.astype(np.int32))


# ---------------------------------------------------------------- settings
@pytest.fixture
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    yield config
    reset_config()


def test_occlusion_defaults(cfg):
    from deepim.core.tracker import occlusion_settings

    assert occlusion_settings(cfg) == dict(mode="none", delta=0.015, min_visible=0.3, max_occluded=30)
    assert cfg.TEST.TRACK_OCC_DELTA == cfg.TEST.VSD_DELTA


@pytest.mark.parametrize("key,bad", [("TRACK_OCCLUSION", "hands"), ("TRACK_OCCLUSION", None), ("TRACK_OCC_DELTA", -0.001),
                                     ("TRACK_OCC_DELTA", float("inf")), ("TRACK_OCC_DELTA", float("nan")), ("TRACK_MIN_VISIBLE", -0.1),
                                     ("TRACK_MIN_VISIBLE", 1.5), ("TRACK_MIN_VISIBLE", float("nan")), ("TRACK_MIN_VISIBLE", True),
                                     ("TRACK_MAX_OCCLUDED", -1), ("TRACK_MAX_OCCLUDED", 2.5), ("TRACK_MAX_OCCLUDED", True)])
def test_occlusion_settings_name_the_bad_key(cfg, key, bad):
    from deepim.core.tracker import Tracker, occlusion_settings, track_settings

    cfg.TEST[key] = bad
    for check in (occlusion_settings, track_settings):
        with pytest.raises(ValueError, match="TEST." + key):
            check(cfg)
    cfg.TEST.INIT_MASK = "box_rendered"
    with pytest.raises(ValueError, match="TEST." + key):   # ... and the constructor, before any device work
        Tracker(cfg, None, object(), 2)


@pytest.mark.parametrize("mode", ["tracks", "depth", "both"])
def test_occlusion_modes_are_accepted(cfg, mode):
    from deepim.core.tracker import occlusion_settings

    cfg.TEST.TRACK_OCCLUSION, cfg.TEST.TRACK_MIN_VISIBLE, cfg.TEST.TRACK_MAX_OCCLUDED = mode, 0, 0
    assert occlusion_settings(cfg) == dict(mode=mode, delta=0.015, min_visible=0.0, max_occluded=0)


# ---------------------------------------------------------------- the synthetic video's occluder event (host part)
def test_occluder_event_changes_no_trajectory_and_sits_where_it_says():
    from lib.dataset.synthetic_sequences import LEAD, occluder_layers, sequence_poses

    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
    ev = [("occluder", 2, 4, 1, 0.3, 25.0, 0), ("occluder", 3, 5, 0, 0.2, 0.0, 0)]
    cls, a = sequence_poses(6, 3, seed=11)
    cls2, b = sequence_poses(6, 3, seed=11, events=ev)
    assert a.tobytes() == b.tobytes() and cls.tobytes() == cls2.tobytes()
    gt = a[LEAD:]
    assert [len(occluder_layers(ev, t, gt[t], K)[0]) for t in range(6)] == [0, 0, 1, 2, 1, 0]
    oc, op = occluder_layers(ev, 3, gt[3], K, seed=11)
    assert oc.tolist() == [0, 0] and op.dtype == np.float32 and op.shape == (2, 3, 4)
    obj = gt[3, 1].astype(np.float64)
    assert abs(op[0, 2, 3] - (obj[2, 3] - 0.3)) < 1e-6
    du = (op[0, 0, 3] / op[0, 2, 3] - obj[0, 3] / obj[2, 3]) * K[0, 0]
    dv = (op[0, 1, 3] / op[0, 2, 3] - obj[1, 3] / obj[2, 3]) * K[1, 1]
    assert abs(du - 25.0) < 1e-3 and abs(dv) < 1e-3
    assert np.abs(op[0, :, :3] @ op[0, :, :3].T - np.eye(3)).max() < 1e-6
    # the rotation is fixed over the event's frames
    assert np.array_equal(occluder_layers(ev, 2, gt[2], K, seed=11)[1][0, :, :3], op[0, :, :3])


def test_too_many_layers_are_refused():
    from deepim.config.config import config, reset_config
    from lib.dataset.synthetic_sequences import SyntheticSequence

    reset_config()
    try:
        config.dataset.class_name = ["ape"]
        ev = [("occluder", 1, 3, 0, 0.3, 0.0, 0), ("occluder", 2, 4, 1, 0.3, 0.0, 0)]
        SyntheticSequence(config, 4, 14, 3, device="cpu", events=ev)            # 14 + 2 = 16 layers in frame 2: the most there is
        with pytest.raises(ValueError, match="16 layers"):
            SyntheticSequence(config, 4, 15, 3, device="cpu", events=ev)
        with pytest.raises(ValueError, match="occluder event"):
            SyntheticSequence(config, 4, 2, 3, device="cpu", events=[("occluder", 0, 1, 2, 0.3, 0.0, 0)])
    finally:
        reset_config()


# ---------------------------------------------------------------- argument errors of the C entry points (nothing is launched)
def test_entry_points_refuse_bad_arguments_without_a_device(hip_lib):
    one = ctypes.c_void_p(256)   # a non-null, aligned "pointer": an argument error returns before anything could read it
    err = lambda: hip_lib.dim_last_error().decode()  # noqa: E731
    assert hip_lib.dim_track_visibility_workspace_bytes(16, 480, 640) == 1200 * 4 * 16 * 4
    assert hip_lib.dim_track_visibility_workspace_bytes(3, 5, 13) == 4 * 3 * 4 and hip_lib.dim_track_visibility_workspace_bytes(0, 5, 13) == 0

    # visibility: (depth_rendered, depth_frame, occluder_ok, P, H, W, mode, delta, workspace, depth_visible, counts, stream)
    def vis(P=2, H=4, W=8, mode=3, delta=0.015, frame=one, ptrs=(one, one, one, one)):
        return hip_lib.dim_track_visibility(ptrs[0], frame, None, P, H, W, mode, delta, ptrs[1], ptrs[2], ptrs[3], None)

    for bad in (dict(P=0), dict(H=0), dict(W=-1)):
        assert vis(**bad) == -1 and "track_visibility: P" in err(), bad
    for mode in (0, 4, 7, -1):
        assert vis(mode=mode) == -1 and "mode" in err(), mode
    for mode in (2, 3):
        assert vis(mode=mode, frame=None) == -1 and "depth_frame" in err()
    for delta in (-0.001, float("inf"), float("nan")):
        assert vis(delta=delta) == -1 and "delta" in err(), delta
    for k in range(4):
        assert vis(mode=1, frame=None, ptrs=tuple(None if j == k else one for j in range(4))) == -1 and "null pointer" in err(), k

    # update_occ: dim_track_update's arguments, then (counts, min_visible, max_occluded, pose_pred) in front of the state
    def update(Wn=3, P=1, n_rows=1, status=one, min_visible=0.3, max_occluded=5, reinit=(one, one), ptrs=(one,) * 16):
        return hip_lib.dim_track_update_occ(ptrs[0], ptrs[1], status, n_rows, 2, None, 0.5, reinit[0], reinit[1], 5.0, 0.05, Wn, 0.25, 6.0, P,
                                            ptrs[2], min_visible, max_occluded, *ptrs[3:], None)

    for Wn in (0, 65):
        assert update(Wn=Wn) == -1 and "Wn" in err()
    assert update(P=0) == -1 and "P = 0" in err()
    assert update(status=None) == -1 and "status_rows" in err()
    assert update(reinit=(one, None)) == -1 and "reinit" in err()
    for bad in (-0.1, 1.5, float("nan")):
        assert update(min_visible=bad) == -1 and "min_visible" in err(), bad
    assert update(max_occluded=-1) == -1 and "max_occluded" in err()
    for k in range(16):
        assert update(ptrs=tuple(None if j == k else one for j in range(16))) == -1 and "null pointer" in err(), k
