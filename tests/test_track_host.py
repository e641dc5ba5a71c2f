"""No GPU: the float64 restatement of the tracker kernels checks itself (tests/track_reference.py), the TEST.TRACK_* settings and the
Tracker constructor name what they refuse, the synthetic video's pose tables are deterministic, and the three C entry points
return DIM_ERR_ARG with a message for bad arguments before anything is enqueued."""
import ctypes

import numpy as np
import pytest

import track_reference as R


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("angle", [0.0, 1e-7, np.radians(1.0), np.radians(90.0), np.radians(179.95)])
def test_exp_of_log_is_the_rotation(angle):
    rng = np.random.RandomState(3)
    for _ in range(5):
        a = rng.randn(3)
        a /= np.linalg.norm(a)
        D = R.so3_exp(angle * a)
        w = R.so3_log(D)
        assert np.abs(R.so3_exp(w) - D).max() <= 1e-12
        assert abs(np.linalg.norm(w) - angle) <= 1e-12
        if angle > 0:
            assert np.abs(w - angle * a).max() <= 1e-9   # the axis itself, sign included


def test_log_at_exactly_pi_is_a_half_turn():
    D = np.diag([1.0, -1.0, -1.0])
    w = R.so3_log(D)
    assert abs(np.linalg.norm(w) - np.pi) <= 1e-15 and np.abs(R.so3_exp(w) - D).max() <= 1e-12


def _hist(n=4, seed=0):
    rng = np.random.RandomState(seed)
    hist = np.zeros((n, 2, 3, 4), np.float32)
    for p in range(n):
        tr = R.constant_velocity_poses(2, R.so3_exp(rng.randn(3)), 0.05 * rng.randn(3), 0.1 * rng.randn(2), 0.01 * rng.randn(2),
                                       rng.uniform(0.6, 1.2), 1.0 + 0.01 * rng.randn())
        hist[p] = tr.astype(np.float32)
    return hist


def test_alpha_zero_equals_hold():
    hist = _hist()
    age = np.full(4, 2, np.int32)
    moved, hold = R.predict(hist, age, "velocity", 0.0)
    held, hold0 = R.predict(hist, age, "hold", 0.0)
    assert not hold.any() and hold0.all()
    assert np.abs(moved - held).max() <= 1e-15
    assert np.array_equal(held, hist[:, 1].astype(np.float64))


def test_alpha_one_reproduces_the_next_pose_of_a_constant_velocity_trajectory():
    rng = np.random.RandomState(7)
    for _ in range(6):
        tr = R.constant_velocity_poses(3, R.so3_exp(rng.randn(3)), 0.2 * rng.randn(3), 0.1 * rng.randn(2), 0.02 * rng.randn(2),
                                       rng.uniform(0.6, 1.2), 1.0 + 0.02 * rng.randn())
        pred, hold = R.predict(tr[None, :2], np.array([2]), "velocity", 1.0)   # float64 history: no rounding in the way
        assert not hold[0] and np.abs(pred[0] - tr[2]).max() <= 1e-12


def test_predict_holds_on_a_short_or_bad_history():
    hist = _hist(6)
    age = np.array([0, 1, 2, 2, 2, 2], np.int32)
    hist[3, 0, 2, 3] = 0.0        # z_prev <= 0
    hist[4, 1, 2, 3] = -1.0       # z_last <= 0
    hist[5, 0, 1, 1] = np.nan
    out, hold = R.predict(hist, age, "velocity", 1.0)
    assert hold.tolist() == [True, True, False, True, True, True]
    assert np.array_equal(out[hold], hist[hold, 1].astype(np.float64), equal_nan=True)


def test_the_scripted_table_reaches_every_update_branch():
    frames = R.scripted_table()
    assert len(frames) == R.TABLE["frames"] == 14 and frames[0]["pose_new"].shape == (6, 3, 4)
    rows = R.run_table(frames)
    lost = {p: [f for f, r in enumerate(rows) if r[0][p] & R.LOST] for p in range(6)}
    reinit = {p: [f for f, r in enumerate(rows) if r[0][p] & R.REINIT] for p in range(6)}
    assert lost == R.EXPECT_LOST and reinit == R.EXPECT_REINIT
    # rule 4 on track 0: the history is the last two poses, bit for bit, the ring wrapped more than once
    st = rows[-1][3]
    assert np.array_equal(st["hist"][0, 1], frames[-1]["pose_new"][0]) and np.array_equal(st["hist"][0, 0], frames[-2]["pose_new"][0])
    assert st["age"][0] == 2 and st["ring_n"][0] == 3 and st["ring_pos"][0] == 14 % 3
    assert all(r[0][0] == 32 for r in rows)                       # the non-fatal bit passes through, nothing is added
    # rule 5: the offered pose bit for bit, age 1, an empty ring (track 3 at frame 2)
    st = rows[2][3]
    assert np.array_equal(st["hist"][3, 1], frames[2]["reinit_pose"][3]) and st["age"][3] == 1
    assert st["ring_n"][3] == 0 and st["ring_pos"][3] == 0 and not st["ring"][3].any()
    # rule 6: history and ring kept, no velocity (track 1 at frame 2)
    before, st = rows[1][3], rows[2][3]
    assert np.array_equal(st["hist"][1], before["hist"][1]) and st["age"][1] == 1 and st["ring_n"][1] == 3
    # the +inf step of track 4 (frame 3)
    assert rows[3][1][4, 1] == np.inf and np.isfinite(rows[3][1][4, 0]) and rows[3][2][4, 1] == np.inf
    # both negative-control variants change the flags somewhere
    for variant in (dict(swap_5_6=True), dict(window_on_part_full=True)):
        other = R.run_table(frames, **variant)
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(rows, other)), variant


# ---------------------------------------------------------------- settings and refusals
@pytest.fixture
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    yield config
    reset_config()


def test_track_defaults(cfg):
    from deepim.core.tracker import track_settings

    assert track_settings(cfg) == dict(motion="velocity", damping=1.0, window=10, lost_rot_deg=10.0, lost_trans=0.01, score="none",
                                       min_score=0.5, depth_tau=0.02, pose="loop")


@pytest.mark.parametrize("key,bad", [("TRACK_MOTION", "accel"), ("TRACK_DAMPING", 1.5), ("TRACK_DAMPING", -0.1), ("TRACK_DAMPING", float("nan")),
                                     ("TRACK_WINDOW", 0), ("TRACK_WINDOW", 65), ("TRACK_WINDOW", 2.5), ("TRACK_LOST_ROT_DEG", 0.0),
                                     ("TRACK_LOST_TRANS", float("inf")), ("TRACK_SCORE", "zncc"), ("TRACK_MIN_SCORE", float("nan")),
                                     ("TRACK_DEPTH_TAU", 0.0), ("TRACK_POSE", "sil"), ("TRACK_POSE", "icp"), ("TRACK_POSE", "photo")])
def test_track_settings_name_the_bad_key(cfg, key, bad):
    from deepim.core.tracker import track_settings

    cfg.TEST[key] = bad
    with pytest.raises(ValueError, match="TEST." + key):
        track_settings(cfg)


def test_track_pose_of_a_stage_that_is_on(cfg):
    from deepim.core.tracker import track_settings

    cfg.TEST.TRACK_POSE, cfg.TEST.PHOTO_ITER = "photo", 2
    assert track_settings(cfg)["pose"] == "photo"


class _Lit(object):
    normals = ()


@pytest.mark.parametrize("change,name", [(dict(HYP_NUM=2), "TEST.HYP_NUM"), (dict(COARSE_VIEWS=4), "TEST.COARSE_VIEWS"),
                                         (dict(SIL_ITER=2), "TEST.SIL_ITER"), (dict(FLOW_PNP_ITER=2), "TEST.FLOW_PNP_ITER"),
                                         (dict(INIT_MASK="mask_gt"), "TEST.INIT_MASK"), (dict(TRACK_WINDOW=0), "TEST.TRACK_WINDOW"),
                                         ("lit", "lit ModelNet renderer")])
def test_tracker_constructor_refuses_by_name_before_any_device_work(cfg, change, name):
    """predictor None and a render machine without a device: a constructor that touched either before its checks would fail otherwise"""
    from deepim.core.tracker import Tracker

    cfg.TEST.INIT_MASK = "box_rendered"
    rm = object()
    if change == "lit":
        rm = _Lit()
    else:
        cfg.TEST.update(change)
    with pytest.raises(ValueError, match=name):
        Tracker(cfg, None, rm, 2)


# ---------------------------------------------------------------- the synthetic video's host part
def test_sequence_pose_tables_are_deterministic_and_smooth():
    from lib.dataset.synthetic_sequences import LEAD, sequence_poses

    cls, a = sequence_poses(6, 3, seed=11)
    cls2, b = sequence_poses(6, 3, seed=11)
    assert a.dtype == np.float32 and a.shape == (LEAD + 6, 3, 3, 4) and a.tobytes() == b.tobytes() and cls.tobytes() == cls2.tobytes()
    assert sequence_poses(6, 3, seed=12)[1].tobytes() != a.tobytes()
    # the velocity model with damping 1 extrapolates every frame from the two before it, up to the float32 rounding of the table
    for k in range(2, a.shape[0]):
        pred, hold = R.predict(np.stack([a[k - 2], a[k - 1]], axis=1), np.full(3, 2), "velocity", 1.0)
        assert not hold.any() and np.abs(pred - a[k]).max() <= 2e-6
    # events: a teleport moves one object from its frame on, and nothing else; a leaving object projects outside the image
    _, tele = sequence_poses(6, 3, seed=11, events=[("teleport", 3, 0, 150.0, -20.0)])
    assert np.array_equal(tele[:LEAD + 3], a[:LEAD + 3]) and np.array_equal(tele[:, 1:], a[:, 1:])
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
    du = (tele[LEAD + 3:, 0, 0, 3] / tele[LEAD + 3:, 0, 2, 3] - a[LEAD + 3:, 0, 0, 3] / a[LEAD + 3:, 0, 2, 3]) * K[0, 0]
    assert np.abs(du - 150.0).max() < 1e-3
    _, gone = sequence_poses(6, 3, seed=11, events=[("leave", 2, 1)])
    u = gone[LEAD + 2:, 1, 0, 3] / gone[LEAD + 2:, 1, 2, 3] * K[0, 0] + K[0, 2]
    assert (u > 640 + 300).all() and np.array_equal(gone[:LEAD + 2], a[:LEAD + 2])
    with pytest.raises(ValueError, match="unknown event"):
        sequence_poses(2, 1, seed=0, events=[("explode", 0, 0)])


# ---------------------------------------------------------------- argument errors of the C entry points (nothing is launched)
def test_entry_points_refuse_bad_arguments_without_a_device(hip_lib):
    one = ctypes.c_void_p(256)   # a non-null, aligned "pointer": an argument error returns before anything could read it
    means = (ctypes.c_float * 3)(1.0, 2.0, 3.0)
    err = lambda: hip_lib.dim_last_error().decode()  # noqa: E731
    # ingest: (frame, depth_raw, P, H, W, depth_factor, means, image_observed, depth_observed, stream)
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 6, 1000.0, means, one, None, None) == -1 and "multiple of 4" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 0, 8, 1000.0, means, one, None, None) == -1 and "track_ingest" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 8, 0.0, means, one, None, None) == -1 and "depth_factor" in err()
    assert hip_lib.dim_track_ingest(None, None, 1, 4, 8, 1000.0, means, one, None, None) == -1 and "null pointer" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 8, 1000.0, None, one, None, None) == -1 and "null pointer" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 8, 1000.0, means, None, None, None) == -1 and "null pointer" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 8, 1000.0, means, one, one, None) == -1 and "depth_raw" in err()
    assert hip_lib.dim_track_ingest(one, None, 1, 4, 8, 1000.0, means, ctypes.c_void_p(260), None, None) == -1 and "alignment" in err()
    # predict: (hist, age, P, mode, alpha, pose_out, stream)
    assert hip_lib.dim_track_predict(one, one, 1, 1, 1.5, one, None) == -1 and "alpha" in err()
    assert hip_lib.dim_track_predict(one, one, 1, 1, -0.01, one, None) == -1 and "alpha" in err()
    assert hip_lib.dim_track_predict(one, one, 1, 1, float("nan"), one, None) == -1 and "alpha" in err()
    assert hip_lib.dim_track_predict(one, one, 1, 2, 0.5, one, None) == -1 and "mode" in err()
    assert hip_lib.dim_track_predict(one, one, 0, 1, 0.5, one, None) == -1 and "P = 0" in err()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert hip_lib.dim_track_predict(args[0], args[1], 1, 1, 0.5, args[2], None) == -1 and "null pointer" in err()

    # update: (before, new, status_rows, n_rows, fatal, score, min_score, reinit_pose, reinit_valid, rot, trans, Wn, znear, zfar, P,
    #          hist, age, ring, ring_n, ring_pos, flags, step, mean, stream)
    def update(Wn=3, P=1, n_rows=1, status=one, ptrs=(one,) * 10, reinit=(one, one)):
        return hip_lib.dim_track_update(ptrs[0], ptrs[1], status, n_rows, 2, None, 0.5, reinit[0], reinit[1], 5.0, 0.05, Wn, 0.25, 6.0, P,
                                        *ptrs[2:], None)

    for Wn in (0, 65, -1):
        assert update(Wn=Wn) == -1 and "Wn" in err()
    assert update(P=0) == -1 and "P = 0" in err()
    assert update(status=None) == -1 and "status_rows" in err()
    assert update(reinit=(one, None)) == -1 and "reinit" in err()
    for k in range(10):
        ptrs = tuple(None if j == k else one for j in range(10))
        assert update(ptrs=ptrs) == -1 and "null pointer" in err(), k
