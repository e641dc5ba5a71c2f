"""CPU: pose from predicted flow -- the float64 restatement (tests/flow_pnp_reference.py) recovers known delta poses from flow
synthesised by the project's own calc_flow, rejects displaced correspondences exactly, reads `valid` at the source pixel and flags
degenerate inputs; the new TEST keys; the host side of the C ABI (workspace size, argument checks before any device call).  The
builders here also make the inputs of tests/test_gpu_flow_pnp.py, so the bars of the GPU tests are shown to be sound here."""
import ctypes

import numpy as np
import pytest

import flow_pnp_reference as fr

ITERS, WARM, HUBER, GATE = 8, 2, 2.0, 8.0
ROTS_DEG = (5.0, 15.0, 30.0)
TRANS_MM = (10.0, 30.0, 50.0)
# Bars.  The worst error of the restatement on exact correspondences over every case below was 1.24e-7 rad / 7.54e-8 m (printed by
# test_exact_correspondences): the rounding of calc_flow's float32 pose product and of the float32 flow and depth planes, not
# algorithm error.  10 x that:
BAR_ROT, BAR_TRANS = 1.3e-6, 8e-7


def small_K(H, W, f):
    return np.array([[f, 0, (W - 1) / 2.0 + 0.7], [0, f * 1.01, (H - 1) / 2.0 - 0.4], [0, 0, 1]], dtype=np.float32)


_MODELS = {}


def _model():
    from lib.utils import synthetic as syn

    if "m" not in _MODELS:
        _MODELS["m"] = syn.make_models(seed=2333, n_models=1, subdiv=3)[0]   # a lobed, anisotropically scaled blob: no hidden rotation
    return _MODELS["m"]


def make_case(H, W, K, rot_deg, trans_mm, seed, standard_rep=False, outliers=0.0, shift_px=(0.0, 0.0), fill=0.5):
    """one pair: the blob rendered (oracle/raster.c) at a seeded pose_src and at pose_tgt = pose_src turned by rot_deg about the object
    origin and moved by trans_mm (camera frame), the flow between them from lib.pair_matching.flow.calc_flow.  outliers: that fraction
    of the visible correspondences is displaced by 20-60 px in a random direction.  shift_px moves the object off the centre; it spans about `fill` of the frame's shorter side.
    -> dict(depth (H,W) f32, flow (2,H,W) f32, visible (H,W) f32, bbox (4,) int32, pose_src (3,4) f32, R_true, t_true, n_inliers)"""
    from lib.pair_matching.flow import calc_flow
    from lib.utils import synthetic as syn
    from oracle import native

    v, t, f, tex = _model()
    rng = np.random.default_rng(seed)
    K = np.asarray(K, np.float32)
    radius = float(np.linalg.norm(v, axis=1).max())
    z = float(K[0, 0]) * 2.0 * radius / (fill * min(H, W))
    c = np.array([(shift_px[0]) * z / K[0, 0], (shift_px[1]) * z / K[1, 1], z]) + np.array(
        [(W - 1) / 2.0 - K[0, 2], (H - 1) / 2.0 - K[1, 2], 0.0]) * z / np.array([K[0, 0], K[1, 1], 1.0])
    pose_src = np.concatenate([syn.random_rotation(rng), c[:, None]], axis=1).astype(np.float32)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    Rd = fr.rodrigues(axis * np.radians(rot_deg))
    pose_tgt = np.concatenate([Rd @ pose_src[:, :3].astype(np.float64),
                               (pose_src[:, 3].astype(np.float64) + direction * trans_mm * 1e-3)[:, None]], axis=1).astype(np.float32)
    d_src = native.render(v, t, f, tex, pose_src[:, :3], pose_src[:, 3], K, H=H, W=W)[1]
    d_tgt = native.render(v, t, f, tex, pose_tgt[:, :3], pose_tgt[:, 3], K, H=H, W=W)[1]
    flow, visible, _ = calc_flow(d_src, pose_src, pose_tgt, K, d_tgt, standard_rep=standard_rep)
    flow = np.ascontiguousarray(flow.transpose(2, 0, 1))
    ys, xs = np.nonzero(visible)
    n_inliers = len(ys)
    if outliers > 0:
        pick = rng.permutation(len(ys))[:int(round(outliers * len(ys)))]
        ang, mag = rng.uniform(0, 2 * np.pi, len(pick)), rng.uniform(20.0, 60.0, len(pick))
        cx_, cy_ = (0, 1) if standard_rep else (1, 0)
        flow[cx_, ys[pick], xs[pick]] += mag * np.cos(ang)
        flow[cy_, ys[pick], xs[pick]] += mag * np.sin(ang)
        n_inliers -= len(pick)
    S, Tt = pose_src.astype(np.float64), pose_tgt.astype(np.float64)
    R_true = Tt[:, :3] @ S[:, :3].T
    yy, xx = np.nonzero(d_src > 0)
    bbox = np.array([xx.min(), xx.max(), yy.min(), yy.max()], np.int32)
    return dict(depth=d_src, flow=flow.astype(np.float32), visible=visible.astype(np.float32), bbox=bbox, pose_src=pose_src,
                R_true=R_true, t_true=Tt[:, 3] - R_true @ S[:, 3], n_inliers=n_inliers, K=K)


def run(case, standard_rep=False, valid="visible", bbox=True, iters=ITERS, K=None):
    return fr.flow_pnp_pair(case["depth"], case["flow"], case["pose_src"], case["K"] if K is None else K, iters, WARM, HUBER, GATE,
                            standard_rep=standard_rep, valid=case["visible"] if isinstance(valid, str) else valid,
                            bbox=case["bbox"] if bbox else None)


def estimate_error(case, pose_out):
    """error of the estimated transform T = pose_out . pose_src^-1 against the true one"""
    S, O = case["pose_src"].astype(np.float64), np.asarray(pose_out, np.float64)
    R = O[:, :3] @ S[:, :3].T
    return fr.transform_error(R, O[:, 3] - R @ S[:, 3], case["R_true"], case["t_true"])


def gpu_batches(outliers=0.3):
    """the small-frame batches of tests/test_gpu_flow_pnp.py: (name, H, W, list of cases, standard_rep).  48x64: W % 4 == 0 (16-byte
    loads), the last pair off-centre so that its box is clipped by the frame; 37x50: the scalar path, odd row stride."""
    out = []
    for rep in (False, True):
        K1 = small_K(48, 64, 100.0)
        a = [make_case(48, 64, K1, 15.0, 30.0, 11, rep, outliers, fill=0.85),
             make_case(48, 64, small_K(48, 64, 110.0), 5.0, 10.0, 12, rep, outliers, fill=0.85),
             make_case(48, 64, K1, 10.0, 20.0, 13, rep, outliers, shift_px=(17.0, -9.0), fill=0.85)]
        K2 = small_K(37, 50, 80.0)
        b = [make_case(37, 50, K2, 12.0, 15.0, 21, rep, outliers, fill=0.85),
             make_case(37, 50, small_K(37, 50, 75.0), 8.0, 20.0, 22, rep, outliers, fill=0.85)]
        out += [("48x64", 48, 64, a, rep), ("37x50", 37, 50, b, rep)]
    return out


@pytest.fixture(scope="module")
def linemod_cases():
    from lib.utils import synthetic as syn

    return {(r, m, rep): make_case(480, 640, syn.LINEMOD_K, r, m, 100 + int(r) + int(m), rep)
            for r in ROTS_DEG for m in TRANS_MM for rep in (False, True)}


def test_exact_correspondences(linemod_cases):
    worst = [0.0, 0.0]
    for (r, m, rep), case in linemod_cases.items():
        pose, se3_q, stats, status = run(case, standard_rep=rep)
        assert status == 0 and stats[-1, 0] == case["n_inliers"] > 2000, (r, m, rep)
        er, et = estimate_error(case, pose)
        worst = [max(worst[0], er), max(worst[1], et)]
        assert er <= BAR_ROT and et <= BAR_TRANS, (r, m, rep, er, et)
        # se3_q is the transform itself, [quat, t], as flow2se3 returns it
        from oracle.se3 import quat2mat
        eq = fr.transform_error(quat2mat(se3_q[:4].astype(np.float64)), se3_q[4:], case["R_true"], case["t_true"])
        assert eq[0] <= 1e-6 and eq[1] <= 1e-6, (r, m, rep, eq)   # float32 output rounding on top
    print("exact correspondences: worst rotation error {:.3g} rad, worst translation error {:.3g} m".format(*worst))
    # the other flow order read with the wrong flag does not reach the pose (the components are told apart)
    case = linemod_cases[(15.0, 30.0, False)]
    er, et = estimate_error(case, run(case, standard_rep=True)[0])
    assert er > 1e-2 or et > 1e-3


def test_outliers_are_rejected_exactly():
    from lib.utils import synthetic as syn

    for r in ROTS_DEG:
        for m in TRANS_MM:
            for rep in (False, True):
                case = make_case(480, 640, syn.LINEMOD_K, r, m, 100 + int(r) + int(m), rep, outliers=0.3)
                pose, _, stats, status = run(case, standard_rep=rep)
                assert status == 0
                assert stats[-1, 0] == case["n_inliers"], (r, m, rep, stats[:, 0], case["n_inliers"])
                er, et = estimate_error(case, pose)
                assert er <= BAR_ROT and et <= BAR_TRANS, (r, m, rep, er, et)


def test_gpu_batches_are_sound():
    """the small-frame inputs of the GPU tests: after the warm iterations the restatement keeps exactly the undisplaced correspondences
    and no displaced one sits within 12 px of the gate, so a float32 / float64 difference cannot change a gate decision"""
    for name, H, W, cases, rep in gpu_batches():
        for k, case in enumerate(cases):
            for bbox in (True, False):
                pose, _, stats, status = run(case, standard_rep=rep, bbox=bbox)
                assert status == 0, (name, k)
                assert stats[-1, 0] == case["n_inliers"] >= 2 * fr.MIN_POINTS, (name, k, stats[:, 0], case["n_inliers"])
                er, et = estimate_error(case, pose)
                assert er <= 10 * BAR_ROT and et <= 10 * BAR_TRANS, (name, k, er, et)   # ~100 times fewer points than at 480x640
            p, uv = fr.correspondences(case["depth"], case["flow"], case["K"], rep, case["visible"], case["bbox"])
            S, O = case["pose_src"].astype(np.float64), pose.astype(np.float64)
            R = O[:, :3] @ S[:, :3].T
            mm = p @ R.T + (O[:, 3] - R @ S[:, 3])
            Kf = case["K"].astype(np.float64)
            e = np.hypot(Kf[0, 0] * mm[:, 0] / mm[:, 2] + Kf[0, 2] - uv[:, 0], Kf[1, 1] * mm[:, 1] / mm[:, 2] + Kf[1, 2] - uv[:, 1])
            assert not np.any((e > 1e-3) & (e < GATE + 12.0)), (name, k)


def test_valid_is_read_at_the_source_pixel(linemod_cases):
    """calc_flow zeroes the flow of the pixels the target view does not see; only `valid` (its visible plane, indexed by SOURCE pixel)
    keeps them out.  A small motion, so that the zeroed pixels (whose residual at the true pose is the true flow) stay under the
    8 px gate; at larger motions the gate itself removes them.  Negative controls: no `valid`, and `valid` indexed by target pixel
    (the plane moved by the flow)."""
    case = linemod_cases[(5.0, 10.0, False)]
    hidden = int(np.sum((case["depth"] > 0) & (case["visible"] == 0)))
    assert hidden > 100
    good = estimate_error(case, run(case)[0])
    assert good[0] <= BAR_ROT and good[1] <= BAR_TRANS
    none = estimate_error(case, run(case, valid=None)[0])
    assert none[0] > 100 * BAR_ROT or none[1] > 100 * BAR_TRANS, none
    ys, xs = np.nonzero(case["visible"])
    moved = np.zeros_like(case["visible"])
    vy = np.clip(np.round(ys + case["flow"][0, ys, xs]).astype(int), 0, 479)
    vx = np.clip(np.round(xs + case["flow"][1, ys, xs]).astype(int), 0, 639)
    moved[vy, vx] = 1.0
    wrong = estimate_error(case, run(case, valid=moved)[0])
    assert wrong[0] > 100 * BAR_ROT or wrong[1] > 100 * BAR_TRANS, wrong


def test_degenerate_inputs(linemod_cases):
    case = linemod_cases[(5.0, 10.0, False)]
    identity = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)

    def flagged(out):
        pose, se3_q, stats, status = out
        assert status == fr.STATUS_FLOW_PNP_FEW_POINTS
        assert np.array_equal(pose.view(np.uint32), case["pose_src"].view(np.uint32))
        assert np.array_equal(se3_q, identity)
        return stats

    empty = dict(case, depth=np.zeros_like(case["depth"]))
    assert flagged(run(empty))[:, 0].max() == 0
    ys, xs = np.nonzero(case["visible"])
    few = np.zeros_like(case["visible"])
    few[ys[:63], xs[:63]] = 1.0
    # (no update: after the warm iterations T is still the identity, the residual is the flow itself and the gate drops every point)
    assert flagged(run(case, valid=few))[:, 0].tolist() == [63.0] * WARM + [0.0] * (ITERS - WARM)
    few[ys[63], xs[63]] = 1.0   # 64 points: enough for an update
    pose, se3_q, stats, _ = run(case, valid=few)
    assert stats[0, 0] == 64 and not np.array_equal(pose, case["pose_src"]) and not np.array_equal(se3_q, identity)
    assert flagged(run(dict(case, flow=np.full_like(case["flow"], np.nan))))[:, 0].max() == 0
    for bad in (0.0, -570.0, np.nan, np.inf):
        K = case["K"].copy()
        K[0, 0] = bad
        assert flagged(run(case, K=K))[:, 0].max() == 0


def test_config_defaults():
    from deepim.config.config import config, reset_config

    reset_config()
    T = config.TEST
    assert (T.FLOW_PNP_ITER, T.FLOW_PNP_WARM, T.FLOW_PNP_HUBER_PX, T.FLOW_PNP_MAX_PX) == (0, 2, 2.0, 8.0)


def test_c_abi_host_side(hip_lib):
    """workspace size and the argument checks, which return before anything touches a device"""
    L = hip_lib
    assert L.dim_flow_pnp_workspace_bytes(0, 480, 640) == 0
    assert L.dim_flow_pnp_workspace_bytes(3, 480, 640) == 3 * L.dim_flow_pnp_workspace_bytes(1, 480, 640) > 0
    assert L.dim_flow_pnp_workspace_bytes(1, 480, 640) % 8 == 0
    K9 = np.eye(3, dtype=np.float32)
    one = ctypes.c_void_p(16)   # a non-NULL pointer that must never be dereferenced

    def call(B=1, iters=8, warm=2, huber=2.0, gate=8.0, depth=one, flow=one, pose=one, K=K9.ctypes.data, work=one, out=one):
        return L.dim_flow_pnp(depth, flow, None, None, pose, K, None, B, 48, 64, 0, iters, warm, huber, gate, work, out, None, None, None, None)

    for kw in (dict(B=0), dict(B=-1), dict(iters=-1), dict(warm=-1), dict(huber=0.0), dict(huber=-1.0), dict(gate=1.0), dict(depth=None),
               dict(flow=None), dict(pose=None), dict(K=None), dict(work=None), dict(out=None)):
        assert call(**kw) == -1, kw
        assert b"flow_pnp" in L.dim_last_error()
