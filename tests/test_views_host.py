"""CPU: the rules for one object seen by several calibrated cameras, on their float64 restatement (tests/views_reference.py), and the
Python layer's settings, refusals and extrinsics check (deepim/core/views.py).  The device side is tests/test_gpu_views_kernels.py."""
import numpy as np
import pytest

import icp_reference as ir
import icp_terms_scenes as sc
import views_reference as vr

EPS64 = float(np.finfo(np.float64).eps)


def _scene_sums(s, R, t):
    """the 29 sums of an analytic ICP scene at the correction (R, t), through icp_reference.normal_equations"""
    p = ir.source_points(s.dr, s.K, s.bbox) @ np.asarray(R).T + np.asarray(t)
    return vr.pack_sums(*ir.normal_equations(p, s.do, s.K, sc.MAX_DIST, s.mask))


# ------------------------------------------------------------------------------------------------------------------ (a) one view, X = I
def test_one_view_identity_is_the_single_view_step():
    s = sc.make("f24a", "plain")
    X = np.eye(3, 4)[None]
    R, t = np.eye(3), np.zeros(3)
    for k in range(3):
        S = _scene_sums(s, R, t)
        assert S[27] >= ir.MIN_POINTS
        want = ir.gn_step(R, t, S)
        got = vr.views_step(R, t, S[None], X)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), k
        Rs, ts = vr.conjugate(X[0], got[0], got[1])
        assert np.array_equal(Rs, got[0]) and np.array_equal(ts, got[1])     # the state row IS the rig correction
        R, t = got[0], got[1]
    # and below the bound neither steps
    S[27] = ir.MIN_POINTS - 1
    assert vr.views_step(R, t, S[None], X)[2] is None and ir.gn_step(R, t, S)[2] is None


# ------------------------------------------------------------------------------------------------------------------ (b) the adjoint rule
@pytest.mark.parametrize("V", [1, 2, 3, 16])
def test_adjoint_rule_is_exact_algebra(V):
    rng = np.random.default_rng(40 + V)
    X = np.stack([vr.random_rigid(rng) for _ in range(V)])
    n_pts = 50
    A_rig, g_rig, sums, scale = np.zeros((6, 6)), np.zeros(6), [], 0.0
    for v in range(V):
        p = rng.uniform(-0.3, 0.3, (n_pts, 3)) + [0.0, 0.0, 1.0]
        n = rng.normal(size=(n_pts, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        r = rng.normal(0, 0.01, n_pts)
        Rv, tv = vr.rt(X[v])
        pv, nv = p @ Rv.T + tv, n @ Rv.T
        Jv, J = np.concatenate([np.cross(pv, nv), nv], axis=1), np.concatenate([np.cross(p, n), n], axis=1)
        back = Jv @ vr.adjoint(X[v])                                  # rows (Ad^T J_v)^T
        assert np.abs(back - J).max() <= 64 * EPS64 * np.abs(Jv).max()
        A_rig += J.T @ J
        g_rig += J.T @ r
        sums.append(vr.pack_sums(Jv.T @ Jv, Jv.T @ r, n_pts, r @ r))
        scale = max(scale, np.abs(Jv.T @ Jv).max())
    A, g, N, rr = vr.fuse(np.stack(sums), X)
    assert N == V * n_pts
    # float64 rounding over a few hundred operations, relative to the largest entry that went in
    assert np.abs(A - A_rig).max() <= 1e-12 * max(scale, np.abs(A_rig).max())
    assert np.abs(g - g_rig).max() <= 1e-12 * max(np.abs(g_rig).max(), np.sqrt(scale) * 0.01 * np.sqrt(V * n_pts))


# ------------------------------------------------------------------------------------------------------------------ (c) conjugates
@pytest.mark.parametrize("steps", [1, 2, 5])
def test_view_states_are_conjugates_of_one_rig_correction(steps):
    rng = np.random.default_rng(7)
    scenes = [sc.make(n, "cut") for n in sc.BATCH]
    X = np.stack([vr.random_rigid(rng) for _ in scenes])
    T = vr.random_rigid(rng)                                          # the group's rig pose
    pose_in = np.stack([vr.mul(Xv, T) for Xv in X]).astype(np.float32)
    out = vr.joint_refine(lambda v, R, t: _scene_sums(scenes[v], R, t), X, steps, pose_in, T.astype(np.float32))
    assert out["stepped"] and not out["failed"]
    R, t = out["D"]
    assert np.abs(R - np.eye(3)).max() > 1e-5                         # it moved
    for v, (Rs, ts) in enumerate(out["states"]):
        want = vr.mul(X[v], vr.mul(vr.mat(R, t), vr.inverse(X[v])))
        assert np.abs(vr.mat(Rs, ts) - want).max() <= 16 * EPS64
        a = vr.mul(vr.mat(Rs, ts), vr.mul(X[v], T))                   # state_v (X_v T)
        b = vr.mul(X[v], vr.mul(vr.mat(R, t), T))                     # X_v (D T)
        assert np.abs(a - b).max() <= 64 * EPS64 * max(1.0, np.abs(b).max())
    # the outputs: every view's pose is the rig pose seen from its camera, to float32 rounding of both
    for v in range(len(X)):
        seen = vr.mul(X[v], out["pose_rig"].astype(np.float64))
        assert np.abs(out["pose"][v] - seen).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(seen).max())


def test_group_that_never_steps_returns_its_inputs():
    rng = np.random.default_rng(8)
    X = np.stack([vr.random_rigid(rng) for _ in range(2)])
    pose_in = rng.normal(size=(2, 3, 4)).astype(np.float32)
    rig_in = rng.normal(size=(3, 4)).astype(np.float32)
    empty = np.zeros(29)
    out = vr.joint_refine(lambda v, R, t: empty, X, 3, pose_in, rig_in)
    assert out["failed"] and not out["stepped"]
    assert np.array_equal(out["pose"].view(np.uint32), pose_in.view(np.uint32))
    assert np.array_equal(out["pose_rig"].view(np.uint32), rig_in.view(np.uint32))
    assert np.all(out["stats"] == 0) and np.all(out["stats_group"] == 0)


def test_the_bound_applies_to_the_group():
    """two views with 40 points each: neither would step alone, the group does"""
    s = sc.make("f24a", "plain")
    S = _scene_sums(s, np.eye(3), np.zeros(3))
    S40 = S * (40.0 / S[27])
    X = np.stack([np.eye(3, 4), vr.random_rigid(np.random.default_rng(3))])
    assert ir.gn_step(np.eye(3), np.zeros(3), S40)[2] is None
    assert vr.views_step(np.eye(3), np.zeros(3), np.stack([S40, S40]), X)[2] is not None


def test_threshold_views_have_no_borderline_gate():
    """the inputs of the GPU group-threshold test: each view alone stays below the bound at every iteration, the group steps every
    time, and no gate decision on the way is borderline (the margins of tests/test_icp_terms_host.py), so the device counts the same"""
    import views_scenes as vs

    scenes, X = vs.threshold_views()
    out = vs.float32_model_chain(scenes, X, vs.THRESHOLD_ITERS)
    assert out["stepped"] and not out["failed"]
    counts = out["stats"][:, :, 0]
    assert np.array_equal(counts, out["truth_counts"])                # the float32 model finds the truth's inliers
    assert counts.min() >= 32 and counts.max() <= 63, counts
    assert np.all(out["stats_group"][:, 0] >= ir.MIN_POINTS)
    for per_iter in out["margins"]:
        for m in per_iter:
            assert m["round_px"] >= 1e-2 and m["jump"] >= 1e-2 and m["dist"] >= 1e-2 and m["nn"] >= 1e-12 and m["flip"] >= 1e-2, m
    for s in scenes:
        assert 32 <= vs.single_view_counts(s, 1)[0] <= 63


# ------------------------------------------------------------------------------------------------------------------ (d) the consensus table
NAN, INF = float("nan"), float("inf")
FATAL = 4 | 16
# (scores, status, expected choice): one group of V = len(scores) views
CONSENSUS_TABLE = [
    ([0.2, 0.7, 0.5], [0, 0, 0], 1),
    ([0.7, 0.7, 0.5], [0, 0, 0], 0),              # a tie: the lowest v
    ([0.1, 0.7, 0.7], [0, 0, 0], 1),
    ([NAN, 0.1, 0.3], [0, 0, 0], 2),              # NaN is not eligible
    ([-INF, -0.9, NAN], [0, 0, 0], 1),            # -inf (dim_pose_score's "no score") is not eligible
    ([INF, 0.9, 0.1], [0, 0, 0], 1),              # +inf is not finite either
    ([0.9, 0.5, 0.1], [4, 0, 0], 1),              # a fatal bit rules the best view out
    ([0.9, 0.5, 0.1], [32, 0, 0], 0),             # a bit outside the mask does not
    ([0.9, 0.5, 0.6], [16, 0, 4], 1),
    ([NAN, -INF, INF], [0, 0, 0], -1),            # no eligible view
    ([0.9, 0.8, 0.7], [4, 16, 20], -1),
    ([0.3], [0], 0),
    ([NAN], [0], -1),
]


def consensus_case(scores, status, seed=0):
    """-> score (V,) f32, status (V,) i32, pose (V,3,4) f32, cam_T_rig (V,3,4) f32 of one group"""
    rng = np.random.default_rng(100 + seed)
    V = len(scores)
    pose = np.stack([vr.random_rigid(rng) + [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1.0]] for _ in range(V)]).astype(np.float32)
    X = np.stack([vr.random_rigid(rng) for _ in range(V)]).astype(np.float32)
    return np.asarray(scores, np.float32), np.asarray(status, np.int32), pose, X


@pytest.mark.parametrize("row", range(len(CONSENSUS_TABLE)))
def test_consensus_table(row):
    scores, status, want = CONSENSUS_TABLE[row]
    score, status, pose, X = consensus_case(scores, status, row)
    V = len(scores)
    choice, pose_rig, pose_views, bits = vr.consensus(score, status, FATAL, pose, X, V)
    assert choice.tolist() == [want]
    c = max(want, 0)                                                  # none eligible: view 0 is used
    assert bits.tolist() == [vr.STATUS_VIEWS_NO_CONSENSUS if want < 0 else 0] * V
    assert np.array_equal(pose_views[c], pose[c].astype(np.float64))  # the chosen row is kept
    Xc = X[c].astype(np.float64)
    assert np.abs(vr.mul(Xc, pose_rig[0]) - pose[c]).max() <= 1e-6    # float32 extrinsics are rigid to ~1e-7
    for v in range(V):
        if v != c:
            assert np.allclose(pose_views[v], vr.mul(X[v], pose_rig[0]), rtol=0, atol=1e-15)
    # NULL status: only the scores decide
    choice2 = vr.consensus(score, None, FATAL, pose, X, V)[0]
    finite = [v for v in range(V) if np.isfinite(score[v])]
    assert choice2.tolist() == [min(finite, key=lambda v: (-score[v], v)) if finite else -1]


def test_views_from_rig_and_back():
    rng = np.random.default_rng(5)
    G, V = 3, 2
    X = np.stack([vr.random_rigid(rng) for _ in range(G * V)])
    T = np.stack([vr.random_rigid(rng) for _ in range(G)])
    views = vr.views_from_rig(T, X, V)
    for b in range(G * V):
        assert np.abs(vr.mul(vr.inverse(X[b]), views[b]) - T[b // V]).max() <= 16 * EPS64


# ------------------------------------------------------------------------------------------------------------------ (e) the Python layer
def _fresh():
    from deepim.config.config import config, reset_config

    reset_config()
    return config


def test_settings_defaults_and_checks():
    from deepim.core.views import FATAL_MASK, views_on, views_settings
    from deepim.core import tracker

    cfg = _fresh()
    try:
        assert cfg.TEST.VIEWS == 1 and cfg.TEST.VIEWS_SCORE == "rgb"
        assert views_settings(cfg) == (1, "rgb", 0.02) and not views_on(cfg)
        assert FATAL_MASK == tracker.FATAL_MASK
        cfg.TEST.VIEWS, cfg.TEST.VIEWS_SCORE, cfg.TEST.HYP_DEPTH_TAU = 3, "depth", 0.03
        assert views_settings(cfg) == (3, "depth", 0.03) and views_on(cfg)
        for key, bad in (("VIEWS", 0), ("VIEWS", 17), ("VIEWS", 2.5), ("VIEWS", True), ("VIEWS_SCORE", "zncc"), ("HYP_DEPTH_TAU", 0.0),
                         ("HYP_DEPTH_TAU", float("nan"))):
            cfg = _fresh()
            cfg.TEST[key] = bad
            with pytest.raises(ValueError, match="TEST." + key):
                views_settings(cfg)
    finally:
        _fresh()


def test_refusals_name_both_keys():
    from deepim.core.tester import refuse_at_source_size
    from deepim.core.tracker import refuse_for_tracking
    from deepim.core.views import refuse_views_at_source_size, refuse_with_views, views_settings

    try:
        for key, on in (("HYP_NUM", 2), ("COARSE_VIEWS", 8), ("FLOW_PNP_ITER", 4)):
            cfg = _fresh()
            cfg.TEST.VIEWS = 2
            cfg.TEST[key] = on
            with pytest.raises(ValueError, match=r"TEST\.VIEWS.*TEST\." + key):
                views_settings(cfg)
            cfg.TEST.VIEWS = 1
            views_settings(cfg)                                       # off: nothing to refuse
        cfg = _fresh()
        cfg.TEST.VIEWS = 2
        views_settings(cfg)
        with pytest.raises(ValueError, match=r"TEST\.VIEWS.*lit ModelNet renderer"):
            views_settings(cfg, lit=True)
        for what in ("load_staged", "the Tracker", "pred_eval"):
            with pytest.raises(ValueError, match=r"TEST\.VIEWS.*" + what):
                refuse_with_views(cfg, what)
        with pytest.raises(ValueError, match=r"TEST\.VIEWS.*Tracker"):
            refuse_for_tracking(cfg)
        # another source size: the consensus is refused under TEST.VIEWS, a joint stage under its own key
        with pytest.raises(ValueError, match=r"TEST\.VIEWS.*SCALES"):
            refuse_views_at_source_size(cfg, (240, 320), (480, 640))
        refuse_views_at_source_size(cfg, (480, 640), (480, 640))
        cfg.TEST.ICP_ITER = 4
        with pytest.raises(ValueError, match=r"TEST\.ICP_ITER.*SCALES"):
            refuse_at_source_size(cfg, (240, 320))
        cfg.TEST.VIEWS, cfg.TEST.ICP_ITER = 1, 0
        refuse_with_views(cfg, "pred_eval")
        refuse_views_at_source_size(cfg, (240, 320), (480, 640))
        refuse_at_source_size(cfg, (240, 320))
    finally:
        _fresh()


def test_pred_eval_refuses_views_before_any_work():
    from deepim.core.tester import pred_eval

    cfg = _fresh()
    try:
        cfg.TEST.VIEWS = 2
        with pytest.raises(ValueError, match=r"TEST\.VIEWS.*pred_eval"):
            pred_eval(cfg, None, [], None)
    finally:
        _fresh()


def test_cam_T_rig_check():
    from deepim.core.views import check_cam_T_rig

    rng = np.random.default_rng(9)
    rig = np.stack([vr.random_rigid(rng) for _ in range(2)]).astype(np.float32)
    out = check_cam_T_rig(rig, 6, 2)
    assert out.shape == (6, 3, 4) and out.dtype == np.float32
    assert np.array_equal(out, np.tile(rig, (3, 1, 1)))               # the V rows repeated G times: sample b = g V + v
    full = np.stack([vr.random_rigid(rng) for _ in range(6)]).astype(np.float32)
    assert np.array_equal(check_cam_T_rig(full, 6, 2), full)
    import torch
    assert np.array_equal(check_cam_T_rig(torch.from_numpy(full), 6, 2), full)
    with pytest.raises(ValueError, match="cam_T_rig"):
        check_cam_T_rig(None, 6, 2)
    with pytest.raises(ValueError, match="cam_T_rig must be"):
        check_cam_T_rig(full[:3], 6, 2)
    for what in ("scale", "shear", "mirror", "nan"):
        bad = full.copy()
        if what == "scale":
            bad[4, :, :3] *= 1.001
        elif what == "shear":
            bad[4, 0, 1] += 0.001
        elif what == "mirror":
            bad[4, :, 0] *= -1
        else:
            bad[4, 1, 3] = np.nan
        with pytest.raises(ValueError, match=r"cam_T_rig\[4\]"):
            check_cam_T_rig(bad, 6, 2)
    ok = full.copy()
    ok[4, :, :3] *= 1.00002                                           # within 1e-4: float32 extrinsics from a calibration file
    check_cam_T_rig(ok, 6, 2)


# ------------------------------------------------------------------------------------------------------------------ the synthetic rig
def test_synthetic_rig_tables():
    from lib.dataset.synthetic_views import rig_samples, ring_rig

    X, Ks = ring_rig(2)
    assert X.dtype == np.float32 and X.shape == (2, 3, 4) and Ks.shape == (2, 3, 3)
    assert abs(float(X[0][2, :3] @ X[1][2, :3])) < 1e-6                # two cameras: principal axes at right angles
    for v in range(2):
        R, t = vr.rt(X[v])
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0
        assert np.allclose(t, [0.0, 0.0, 0.8], atol=1e-6)             # the rig origin lies on the optical axis, a radius away
    assert not np.array_equal(Ks[0], Ks[1]) and np.abs(Ks[0] - Ks[1]).max() < 30
    X4, _ = ring_rig(4, span_deg=120.0)
    assert np.allclose(np.degrees(np.arccos(np.clip(X4[0][2, :3] @ X4[3][2, :3], -1, 1))), 120.0, atol=1e-3)
    s, s2 = rig_samples(3, 2, 11), rig_samples(3, 2, 11)
    assert all(np.array_equal(s[k], s2[k]) for k in s)                # seeded: the same bytes
    assert s["pose_gt"].shape == (6, 3, 4) and s["cam_T_rig"].shape == (6, 3, 4) and s["class_index"].shape == (6,)
    assert np.array_equal(s["cam_T_rig"][:2], s["cam_T_rig"][2:4])    # the rig's V rows repeated per group
    for b in range(6):
        assert np.abs(s["pose_gt"][b] - vr.mul(s["cam_T_rig"][b], s["pose_rig_gt"][b // 2])).max() < 1e-6
        assert 1e-4 < np.abs(s["pose_init"][b] - s["pose_gt"][b]).max() < 0.2
        assert 0.6 < s["pose_gt"][b][2, 3] < 1.0                      # in front of every camera
    assert np.abs(s["pose_init"][0] - s["pose_gt"][0]).max() != np.abs(s["pose_init"][1] - s["pose_gt"][1]).max()   # perturbed per view
    from deepim.core.views import check_cam_T_rig
    check_cam_T_rig(s["cam_T_rig"], 6, 2)


def test_multiview_table_helpers():
    import importlib.util
    import os
    from conftest import PKG
    from lib.dataset.synthetic_views import rig_samples

    spec = importlib.util.spec_from_file_location("multiview_cli", os.path.join(PKG, "deepim", "multiview.py"))
    here = os.getcwd()
    import sys
    sys.path.insert(0, os.path.join(PKG, "deepim"))
    try:
        mv = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mv)
    finally:
        sys.path.remove(os.path.join(PKG, "deepim"))
        os.chdir(here)
    s = rig_samples(2, 2, 3)
    start = mv.axis_shift_poses(s, 2, 0.015)
    models = [(np.random.default_rng(0).uniform(-0.1, 0.1, (50, 3)),)]
    rigs = {"loop": s["pose_rig_gt"]}
    rows = mv.views_table(["loop"], {"loop": start}, {"loop": s["pose_gt"]}, rigs, s, 2, models)
    alone, joint = rows
    assert alone["which"] == "independent" and joint["which"] == "joint"
    assert abs(alone["axis"] - 0.015) < 1e-5 and alone["rot_deg"] < 0.02    # 15 mm along camera 0's axis in EVERY view; no turn
    # (pose_error.re takes arccos of the trace: float32 rotations leave it ~1e-4 rad from 0)
    assert 0.015 < alone["trans"] < 0.02 and alone["gap"] < 1e-5             # ... and consistently so: a rigid shift of the rig pose
    assert joint["add"] < 1e-6 and joint["gap"] < 1e-6
