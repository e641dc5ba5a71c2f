"""csrc/track.hip on the device, each entry through its lib.hip.ops wrapper:
  dim_track_ingest    bit-equal to numpy and to ops.pair_blobs_from_raw on the same bytes, outputs between guard words
  dim_track_predict   hold cases bit-equal to hist[1], computed cases within 1e-6 of tests/track_reference.py
  dim_track_update    the scripted 14-frame table of tests/track_reference.py frame by frame, carrying the device's own state"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_reference as R  # noqa: E402
from guard_arena import SENTINEL_WORD, GuardArena  # noqa: E402

DEV = "cuda:0"
PIXEL_MEANS_BGR = np.array([102.9801, 115.9465, 122.7717], np.float32)
DEPTH_FACTOR = 1000.0


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ ingest
@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 4), (3, 8), (5, 12), (480, 640)])
def test_ingest_matches_numpy_and_pair_blobs(ops, H, W, P, with_depth):
    rng = np.random.RandomState(H * 1000 + W + P)
    frame = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    depth = rng.randint(0, 65536, size=(H, W)).astype(np.uint16)
    depth[0, :2] = (0, 65535)
    img = GuardArena(P * 3 * H * W, fill=SENTINEL_WORD)
    dep = GuardArena(P * H * W, fill=SENTINEL_WORD)
    d_frame, d_depth = dev(frame), dev(depth)
    ops.track_ingest(d_frame, DEPTH_FACTOR, PIXEL_MEANS_BGR, img.view((P, 3, H, W)), depth_raw=d_depth if with_depth else None,
                     depth_observed=dep.view((P, 1, H, W)) if with_depth else None)
    img.check("ingest image {}x{} P {}".format(H, W, P))
    dep.check("ingest depth {}x{} P {}".format(H, W, P))
    got_img, got_dep = host(img.view((P, 3, H, W))), host(dep.view((P, 1, H, W)))
    # numpy: planar RGB with the mean subtracted; a true float32 division for the depth
    want_img = np.stack([frame[:, :, 2 - c].astype(np.float32) - PIXEL_MEANS_BGR[2 - c] for c in range(3)])
    want_dep = depth.astype(np.float32) / np.float32(DEPTH_FACTOR)
    for p in range(P):
        assert got_img[p].tobytes() == want_img.tobytes(), ("image", p)
        if with_depth:
            assert got_dep[p, 0].tobytes() == want_dep.tobytes(), ("depth", p)
    if not with_depth:   # nothing was written
        assert np.array_equal(got_dep.view(np.uint32), np.full(got_dep.shape, SENTINEL_WORD, np.uint32))
    # ... and the bits of the data layer's kernel on the same bytes
    pair_img = torch.empty((1, 3, H, W), device=DEV)
    pair_dep = torch.empty((1, 1, H, W), device=DEV)
    ops.pair_blobs_from_raw(1, H, W, DEPTH_FACTOR, PIXEL_MEANS_BGR, obs_bgr=d_frame.view(1, H, W, 3), depth_a=d_depth.view(1, H, W),
                            image_observed=pair_img, depth_a_out=pair_dep)
    assert host(pair_img)[0].tobytes() == got_img[0].tobytes()
    if with_depth:
        assert host(pair_dep)[0].tobytes() == got_dep[0].tobytes()


def test_ingest_refuses_bad_geometry(ops):
    from lib.hip.capi import DeepIMHipError

    out = GuardArena(3 * 4 * 6, fill=SENTINEL_WORD)
    with pytest.raises(DeepIMHipError, match="multiple of 4"):
        ops.track_ingest(dev(np.zeros((4, 6, 3), np.uint8)), DEPTH_FACTOR, PIXEL_MEANS_BGR, out.view((1, 3, 4, 6)))
    with pytest.raises(DeepIMHipError, match="depth_factor"):
        ops.track_ingest(dev(np.zeros((4, 8, 3), np.uint8)), 0.0, PIXEL_MEANS_BGR, torch.empty((1, 3, 4, 8), device=DEV))
    out.check("rejected ingest")
    assert np.array_equal(host(out.view()).view(np.uint32), np.full(72, SENTINEL_WORD, np.uint32))


# ------------------------------------------------------------------------------------------------ predict
def _predict_tracks():
    """P = 8: age 0, age 1, a general motion, identical poses, a 1e-7 rad turn, a 179.95 degree turn, z_prev <= 0, a NaN entry"""
    rng = np.random.RandomState(21)
    hist = np.zeros((8, 2, 3, 4), np.float32)
    for p in range(8):
        R0 = R.so3_exp(rng.randn(3))
        w = 0.3 * rng.randn(3)
        if p == 3:
            w = np.zeros(3)
        if p in (4, 5):
            w *= (1e-7 if p == 4 else np.radians(179.95)) / np.linalg.norm(w)
        tr = R.constant_velocity_poses(2, R0, w, 0.2 * rng.randn(2), (0.0 if p == 3 else 0.03) * rng.randn(2), rng.uniform(0.6, 1.5),
                                       1.0 if p == 3 else 1.0 + 0.03 * rng.randn())
        hist[p] = tr.astype(np.float32)
    hist[6, 0, 2, 3] = -0.1
    hist[7, 1, 0, 1] = np.nan
    age = np.array([0, 1, 2, 2, 2, 2, 2, 2], np.int32)
    return hist, age


@pytest.mark.parametrize("mode", ["hold", "velocity"])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_predict_matches_reference(ops, mode, alpha):
    hist, age = _predict_tracks()
    assert np.array_equal(hist[3, 0], hist[3, 1])
    turn5 = R.angle_deg(hist[5, 1, :, :3].astype(np.float64) @ hist[5, 0, :, :3].astype(np.float64).T)
    assert abs(turn5 - 179.95) < 1e-3
    want, hold = R.predict(hist, age, mode, alpha)
    assert hold.tolist() == ([True] * 8 if mode == "hold" else [True, True, False, False, False, False, True, True])
    out = GuardArena(8 * 12, fill=SENTINEL_WORD)
    got = host(ops.track_predict(dev(hist), dev(age), mode, alpha, out=out.view((8, 3, 4))))
    out.check("predict")
    for p in range(8):
        if hold[p]:
            assert got[p].tobytes() == hist[p, 1].tobytes(), p
        else:
            err = np.abs(got[p].astype(np.float64) - want[p]).max()
            print("predict {} alpha {} track {}: |device - reference| = {:.2e}".format(mode, alpha, p, err))
            assert err <= 1e-6, (p, err)
    if mode == "velocity" and alpha == 1.0:   # the prediction moves: a kernel that always held would not pass
        assert np.abs(got[2].astype(np.float64) - hist[2, 1]).max() > 1e-3
        assert np.abs(got[5].astype(np.float64) - hist[5, 1]).max() > 0.5


# ------------------------------------------------------------------------------------------------ update
def _close(got, want, what):
    """f32 outputs of double arithmetic: (rot degrees, trans metres) pairs.  +inf must be +inf; 1e-4 relative where the reference
    exceeds 1e-3 (degrees) / 1e-6 (metres), else at most 2e-3 degrees / 2e-6 metres"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and (got[inf] > 0).all(), what
    for col, floor in ((0, 1e-3), (1, 1e-6)):
        g, w = got[..., col][~inf[..., col]], want[..., col][~inf[..., col]]
        big = w > floor
        assert (np.abs(g[big] - w[big]) <= 1e-4 * w[big]).all(), (what, col, g, w)
        assert (np.abs(g[~big]) <= 2 * floor).all(), (what, col, g, w)


def test_update_runs_the_scripted_table(ops):
    T = R.TABLE
    frames = R.scripted_table()
    ref = R.run_table(frames)
    P, Wn = T["tracks"], T["Wn"]
    st0 = R.new_state(P, Wn)
    st0["hist"][:, 0] = st0["hist"][:, 1] = frames[0]["pose_before"]
    st0["age"][:] = 1
    arenas = {k: GuardArena(v.size, dtype=torch.float32 if v.dtype == np.float32 else torch.int32) for k, v in st0.items()}
    state = {k: arenas[k].view(v.shape) for k, v in st0.items()}
    for k, v in st0.items():
        state[k].copy_(dev(v))
    outs = {"flags": GuardArena(P, dtype=torch.int32), "step": GuardArena(2 * P), "mean": GuardArena(2 * P)}
    flags_all = []
    for f, fr in enumerate(frames):
        flags, step, mean = ops.track_update(dev(fr["pose_before"]), dev(fr["pose_new"]), state["hist"], state["age"], state["ring"],
                                             state["ring_n"], state["ring_pos"], T["lost_rot_deg"], T["lost_trans_m"], T["znear"],
                                             T["zfar"], status_rows=dev(fr["status_rows"]), fatal_mask=T["fatal_mask"],
                                             score=dev(fr["score"]), min_score=T["min_score"], reinit_pose=dev(fr["reinit_pose"]),
                                             reinit_valid=dev(fr["reinit_valid"]), flags=outs["flags"].view((P,)),
                                             step=outs["step"].view((P, 2)), mean=outs["mean"].view((P, 2)))
        for a in list(arenas.values()) + list(outs.values()):
            a.check("update frame {}".format(f))
        w_flags, w_step, w_mean, w_state = ref[f]
        flags_all.append(host(flags).copy())
        assert np.array_equal(flags_all[-1], w_flags), (f, flags_all[-1], w_flags)
        for k in ("age", "ring_n", "ring_pos"):
            assert np.array_equal(host(state[k]), w_state[k]), (f, k)
        assert host(state["hist"]).tobytes() == w_state["hist"].tobytes(), f
        _close(host(step), w_step, "step frame {}".format(f))
        _close(host(mean), w_mean, "mean frame {}".format(f))
        _close(host(state["ring"]), w_state["ring"], "ring frame {}".format(f))
    lost = {p: [f for f, fl in enumerate(flags_all) if fl[p] & R.LOST] for p in range(P)}
    assert lost == R.EXPECT_LOST
    # negative controls: a reference with rules 5 / 6 swapped, or with the window rule on a part-full ring, disagrees with the device
    for variant in (dict(swap_5_6=True), dict(window_on_part_full=True)):
        other = R.run_table(frames, **variant)
        assert any(not np.array_equal(flags_all[f], other[f][0]) for f in range(len(frames))), variant


def test_update_without_score_and_without_an_offer(ops):
    """score NULL: no score rule; reinit NULL: a lost track takes rule 6; n_rows 0: no status"""
    P, Wn = 2, 2
    pose = np.stack([R.pose_of([0.1, 0.2, 0.3], [0.0, 0.0, 0.8]), R.pose_of([0.3, 0.0, 0.1], [0.1, 0.0, 7.5])])
    st = R.new_state(P, Wn)
    st["hist"][:, 1] = pose
    st["age"][:] = 2
    state = {k: dev(v) for k, v in st.items()}
    flags, step, mean = ops.track_update(dev(pose), dev(pose), state["hist"], state["age"], state["ring"], state["ring_n"],
                                         state["ring_pos"], 5.0, 0.05, 0.25, 6.0)
    w_flags, w_step, w_mean = R.update(st, pose, pose, np.zeros((0, P), np.int32), 0, None, 0.5, None, None, 5.0, 0.05, 0.25, 6.0)
    assert host(flags).tolist() == w_flags.tolist() == [0, R.LOST]
    assert host(state["age"]).tolist() == st["age"].tolist() == [2, 1]
    assert host(state["hist"]).tobytes() == st["hist"].tobytes()
    assert np.array_equal(host(step), np.zeros((P, 2), np.float32))   # identical poses: a step of exactly zero
