"""The occlusion kernels of csrc/track.hip on the device, each through its lib.hip.ops wrapper, against tests/track_occ_reference.py:
  dim_track_visibility   depth_visible bit for bit and counts exactly on planes drawn from the boundary values (ties, exactly delta
                         apart and one float32 step either side, NaN, inf, 0, negatives), outputs and workspace between guard words,
                         a second call on dirty outputs, the argument errors
  dim_track_update_occ   the scripted table of the occluded state frame by frame, carrying the device's own state; and
                         tests/track_reference.py's table through dim_track_update and dim_track_update_occ side by side"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_occ_reference as O  # noqa: E402
import track_reference as R  # noqa: E402
from guard_arena import SENTINEL_WORD, GuardArena  # noqa: E402
from test_gpu_track_kernels import _close  # noqa: E402

DEV = "cuda:0"
# (P, H, W): a lone track; the 16-byte path; the one-pixel path (W % 4 != 0); more tracks than dim_scene_compose has layers; a plane
# of several workgroups (2560 pixels: 3 of 1024 on the 16-byte path)
SHAPES = [(1, 4, 8), (3, 5, 12), (3, 5, 13), (17, 6, 16), (2, 40, 64)]
DELTAS = (0.015, 0.015625)   # the default, and one that is exact next to the base depths: "exactly delta apart" occurs


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


@pytest.fixture(scope="module")
def planes():
    """per shape and delta: (depth_rendered, depth_frame, occluder_ok), made once and never written"""
    out = {}
    for P, H, W in SHAPES:
        for delta in DELTAS:
            rng = np.random.RandomState(1000 * P + 10 * W + int(delta * 1e6) % 7)
            depth, frame = O.boundary_planes(rng, P, H, W, delta)
            ok = np.ones(P, np.int32)
            ok[rng.randint(0, P)] = 0
            out[(P, H, W, delta)] = (depth, frame, ok)
    return out


# ------------------------------------------------------------------------------------------------ visibility
@pytest.mark.parametrize("mode", ["tracks", "depth", "both"])
@pytest.mark.parametrize("P,H,W", SHAPES)
def test_visibility_matches_reference(ops, planes, P, H, W, mode):
    for delta in DELTAS:
        depth, frame, ok = planes[(P, H, W, delta)]
        d_depth, d_frame = dev(depth), dev(frame)
        for use_ok in (None, ok):
            want_vis, want_cnt = O.visibility(depth, frame, use_ok, mode, delta)
            vis = GuardArena(P * H * W, fill=SENTINEL_WORD)
            cnt = GuardArena(4 * P, dtype=torch.int32, fill=SENTINEL_WORD)
            work = GuardArena(ops.lib().dim_track_visibility_workspace_bytes(P, H, W) // 4, dtype=torch.int32, fill=SENTINEL_WORD)
            args = dict(depth_frame=d_frame if mode != "tracks" else None, occluder_ok=None if use_ok is None else dev(use_ok),
                        depth_visible=vis.view((P, 1, H, W)), counts=cnt.view((P, 4)), workspace=work.view())
            for call in ("first", "second, on what the first left"):
                ops.track_visibility(d_depth, mode, delta, **args)
                what = "visibility {} P {} {}x{} delta {} ok {}: {} call".format(mode, P, H, W, delta, use_ok is not None, call)
                for a in (vis, cnt, work):
                    a.check(what)
                got_vis, got_cnt = host(vis.view((P, 1, H, W))), host(cnt.view((P, 4)))
                assert np.array_equal(got_cnt, want_cnt), (what, got_cnt, want_cnt)
                assert got_vis.tobytes() == want_vis.tobytes(), what
            assert np.array_equal(got_cnt[:, 0], got_cnt[:, 1:].sum(1))
            if P == 1:
                assert not got_cnt[:, 2].any()      # a lone track is never hidden by tracks
            elif mode != "depth" and delta == DELTAS[1]:
                assert got_cnt[:, 2].any() and got_cnt[:, 1].any(), "the planes hide nothing: the comparison guards nothing"
            if mode != "tracks":
                assert got_cnt[:, 3].any()


def test_visibility_on_unaligned_planes_takes_the_one_pixel_path(ops, planes):
    """W % 4 == 0 but the planes start 4 bytes off a 16-byte boundary: the same bits through scalar accesses"""
    P, H, W = 3, 5, 12
    delta = DELTAS[1]
    depth, frame, ok = planes[(P, H, W, delta)]
    want_vis, want_cnt = O.visibility(depth, frame, ok, "both", delta)
    src = GuardArena(P * H * W, align=16, phase=4)
    vis = GuardArena(P * H * W, fill=SENTINEL_WORD, align=16, phase=4)
    src.view((P, 1, H, W)).copy_(dev(depth))
    assert src.address() % 16 == 4 and vis.address() % 16 == 4
    _, cnt = ops.track_visibility(src.view((P, 1, H, W)), "both", delta, depth_frame=dev(frame), occluder_ok=dev(ok),
                                  depth_visible=vis.view((P, 1, H, W)))
    vis.check("unaligned visibility")
    src.check("unaligned visibility (input)")
    assert np.array_equal(host(cnt), want_cnt) and host(vis.view((P, 1, H, W))).tobytes() == want_vis.tobytes()


def test_visibility_refuses_bad_arguments(ops):
    from lib.hip.capi import DeepIMHipError

    P, H, W = 2, 4, 8
    depth = dev(np.full((P, 1, H, W), 0.5, np.float32))
    vis = GuardArena(P * H * W, fill=SENTINEL_WORD)
    cnt = GuardArena(4 * P, dtype=torch.int32, fill=SENTINEL_WORD)
    out = dict(depth_visible=vis.view((P, 1, H, W)), counts=cnt.view((P, 4)))
    with pytest.raises(ValueError, match="mode"):
        ops.track_visibility(depth, "hands", 0.015, **out)
    with pytest.raises(ValueError, match="depth_frame"):
        ops.track_visibility(depth, "both", 0.015, **out)
    for delta in (-0.001, float("inf"), float("nan")):
        with pytest.raises(DeepIMHipError, match="delta"):
            ops.track_visibility(depth, "tracks", delta, **out)
    lib, cur = ops.lib(), ops.current_stream()
    work = ops.track_visibility_workspace(P, H, W, DEV)
    ptr = lambda t: ops.dptr(t)  # noqa: E731
    for mode in (0, 4, 5):
        assert lib.dim_track_visibility(ptr(depth), ptr(depth[0, 0]), None, P, H, W, mode, 0.015, ptr(work), ptr(out["depth_visible"]),
                                        ptr(out["counts"]), cur) == -1
    assert lib.dim_track_visibility(ptr(depth), None, None, P, H, W, 2, 0.015, ptr(work), ptr(out["depth_visible"]), ptr(out["counts"]), cur) == -1
    assert lib.dim_track_visibility(ptr(depth), None, None, 0, H, W, 1, 0.015, ptr(work), ptr(out["depth_visible"]), ptr(out["counts"]), cur) == -1
    # nothing was enqueued: every output word still holds its sentinel
    for a in (vis, cnt):
        a.check("rejected visibility")
        assert np.array_equal(host(a.view()).view(np.uint32), np.full(a.numel, SENTINEL_WORD, np.uint32))


# ------------------------------------------------------------------------------------------------ update with the occluded state
STATE_KEYS = ("hist", "age", "ring", "ring_n", "ring_pos", "occ_age")
OUT_SHAPES = {"flags": ((1,), torch.int32), "step": ((2,), torch.float32), "mean": ((2,), torch.float32), "visible": ((1,), torch.float32),
              "pose_track": ((3, 4), torch.float32), "occluder_ok": ((1,), torch.int32)}


def _device_state(st0):
    arenas = {k: GuardArena(v.size, dtype=torch.float32 if v.dtype == np.float32 else torch.int32) for k, v in st0.items()}
    state = {k: arenas[k].view(v.shape) for k, v in st0.items()}
    for k, v in st0.items():
        state[k].copy_(dev(v))
    return arenas, state


def _device_outputs(P):
    arenas = {k: GuardArena(P * int(np.prod(shape)), dtype=dt, fill=SENTINEL_WORD) for k, (shape, dt) in OUT_SHAPES.items()}
    return arenas, {k: arenas[k].view((P,) + shape if shape != (1,) else (P,)) for k, (shape, _) in OUT_SHAPES.items()}


def _update_occ(ops, T, fr, state, outs, counts, min_visible, max_occluded, pose_pred):
    return ops.track_update_occ(dev(fr["pose_before"]), dev(fr["pose_new"]), state["hist"], state["age"], state["ring"], state["ring_n"],
                                state["ring_pos"], state["occ_age"], dev(counts), min_visible, max_occluded, dev(pose_pred),
                                T["lost_rot_deg"], T["lost_trans_m"], T["znear"], T["zfar"], status_rows=dev(fr["status_rows"]),
                                fatal_mask=T["fatal_mask"], score=dev(fr["score"]), min_score=T["min_score"],
                                reinit_pose=dev(fr["reinit_pose"]), reinit_valid=dev(fr["reinit_valid"]), **outs)


def test_update_occ_runs_the_occlusion_table(ops):
    """every integer state tensor and output, the history, pose_track and visible bit-equal to the reference.  The ring holds float32
    roundings of float64 angles and lengths (atan2, sqrt): its entries are bit-equal to the steps the device itself reported on the
    frames the reference says they entered, and those steps and the means are held to tests/test_gpu_track_kernels.py's bar"""
    T = O.OCC_TABLE
    frames = O.occ_table()
    ref = O.run_table(frames)
    P, Wn = T["tracks"], T["Wn"]
    arenas, state = _device_state(O.table_state(frames))
    out_arenas, outs = _device_outputs(P)
    ring_want = np.zeros((P, Wn, 2), np.float32)
    prev = O.table_state(frames)
    flags_all = []
    for f, fr in enumerate(frames):
        _update_occ(ops, T, fr, state, outs, fr["counts"], T["min_visible"], T["max_occluded"], fr["pose_pred"])
        for a in list(arenas.values()) + list(out_arenas.values()):
            a.check("update_occ frame {}".format(f))
        want, w_state = ref[f]
        got = {k: host(v).copy() for k, v in outs.items()}
        flags_all.append(got["flags"])
        for k in ("flags", "occluder_ok"):
            assert np.array_equal(got[k], want[k]), (f, k, got[k], want[k])
        for k in ("age", "ring_n", "ring_pos", "occ_age"):
            assert np.array_equal(host(state[k]), w_state[k]), (f, k, host(state[k]), w_state[k])
        assert host(state["hist"]).tobytes() == w_state["hist"].tobytes(), f
        assert got["pose_track"].tobytes() == want["pose_track"].tobytes() == w_state["hist"][:, 1].tobytes(), f
        assert got["visible"].tobytes() == want["visible"].tobytes(), (f, got["visible"], want["visible"])
        _close(got["step"], want["step"], "step frame {}".format(f))
        _close(got["mean"], want["mean"], "mean frame {}".format(f))
        for p in range(P):   # what the reference did to the ring, replayed with the device's own step
            if w_state["ring_n"][p] == 0 and not w_state["ring"][p].any():
                ring_want[p] = 0
            elif w_state["ring_pos"][p] != prev["ring_pos"][p]:
                ring_want[p, prev["ring_pos"][p]] = got["step"][p]
        assert host(state["ring"]).tobytes() == ring_want.tobytes(), f
        _close(host(state["ring"]), w_state["ring"], "ring frame {}".format(f))
        prev = w_state
    for bit, expect in ((O.OCCLUDED, O.EXPECT_OCCLUDED), (O.LOST, O.EXPECT_LOST), (O.REINIT, O.EXPECT_REINIT)):
        assert {p: [f for f, fl in enumerate(flags_all) if fl[p] & bit] for p in range(P)} == expect
    # negative control: a reference whose coasting tracks push their step into the ring disagrees with the device
    other = O.run_table(frames, coast_pushes_ring=True)
    assert any(not np.array_equal(flags_all[f], other[f][0]["flags"]) for f in range(len(frames)))


@pytest.mark.parametrize("counts", ["visible", "hidden"])
def test_update_occ_without_occlusion_is_update_bit_for_bit(ops, counts):
    """tests/track_reference.py's table through dim_track_update and dim_track_update_occ on the device, each carrying its own
    state: everything visible (min_visible 1), or nothing visible and min_visible 0 -- every shared tensor has the same bits"""
    T = R.TABLE
    frames = R.scripted_table()
    P, Wn = T["tracks"], T["Wn"]
    st0 = O.table_state(frames, T)
    _, plain = _device_state({k: st0[k] for k in STATE_KEYS[:5]})
    arenas, state = _device_state(st0)
    out_arenas, outs = _device_outputs(P)
    cnt = np.tile(np.array([50, 50, 0, 0] if counts == "visible" else [50, 0, 50, 0], np.int32), (P, 1))
    lost_seen = 0
    for f, fr in enumerate(frames):
        flags, step, mean = ops.track_update(dev(fr["pose_before"]), dev(fr["pose_new"]), plain["hist"], plain["age"], plain["ring"],
                                             plain["ring_n"], plain["ring_pos"], T["lost_rot_deg"], T["lost_trans_m"], T["znear"],
                                             T["zfar"], status_rows=dev(fr["status_rows"]), fatal_mask=T["fatal_mask"],
                                             score=dev(fr["score"]), min_score=T["min_score"], reinit_pose=dev(fr["reinit_pose"]),
                                             reinit_valid=dev(fr["reinit_valid"]))
        _update_occ(ops, T, fr, state, outs, cnt, 1.0 if counts == "visible" else 0.0, 3, fr["pose_before"])
        for a in list(arenas.values()) + list(out_arenas.values()):
            a.check("update_occ frame {}".format(f))
        for k, t in (("flags", flags), ("step", step), ("mean", mean)):
            assert host(outs[k]).tobytes() == host(t).tobytes(), (f, k)
        for k in STATE_KEYS[:5]:
            assert host(state[k]).tobytes() == host(plain[k]).tobytes(), (f, k)
        assert not host(state["occ_age"]).any()
        assert host(outs["pose_track"]).tobytes() == host(plain["hist"])[:, 1].tobytes()
        fl = host(flags)
        assert np.array_equal(host(outs["occluder_ok"]), 1 - (((fl & R.LOST) != 0) & ((fl & R.REINIT) == 0)).astype(np.int32))
        assert np.array_equal(host(outs["visible"]), np.full(P, 1.0 if counts == "visible" else 0.0, np.float32))
        lost_seen += int(((fl & R.LOST) != 0).sum())
    assert lost_seen == sum(len(v) for v in R.EXPECT_LOST.values())
