"""tests/rig_reference.py, the float64 restatement of the rig calibration rule, fixed on the CPU: its special cases against
tests/views_reference.py, the Schur form against a dense Cholesky of the full system, convergence on a problem with fixed
correspondences, the branches of "who takes part" on scripted sums; and the settings and refusals of the Python layer."""
import numpy as np
import pytest

import icp_reference as ir
import rig_reference as rr
import views_reference as vr
import views_scenes as vs

EPS64 = float(np.finfo(np.float64).eps)
FEW, HELD = rr.FEW, rr.STATUS_VIEWS_CALIB_HELD


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[np.asarray(a).dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


def _model_sums(scenes, V, edit=None):
    """sample_sums of rig_refine from the float32 model of icp_accumulate_kernel; edit(g, v, sums) may script them"""
    def sums(g, v, R, t):
        s = scenes[g * V + v].partial(R, t, np.float32)[0].sum(axis=0)
        return s if edit is None else edit(g, v, s)
    return sums


def _inputs(G, V, seed):
    scenes, X = vs.batch_scenes(G * V), vs.rig(seed, V)
    return scenes, X, np.stack([s.pose_in for s in scenes]), vs.rig_poses(seed, G)


# ------------------------------------------------------------------------------------------------------------------ the special cases
def test_one_view_is_views_step_per_group():
    G = 3
    scenes, X, pose_in, rig_in = _inputs(G, 1, 4)
    out = rr.rig_refine(_model_sums(scenes, 1), X, G, 3, pose_in, rig_in)
    assert not np.any(out["status"]) and _same(out["cam_T_rig"], X)
    for g in range(G):
        want = vr.joint_refine(lambda v, R, t: scenes[g].partial(R, t, np.float32)[0].sum(axis=0), X, 3, pose_in[g:g + 1], rig_in[g])
        assert want["stepped"] and not want["failed"]
        assert _same(out["D"][g][0], want["D"][0]) and _same(out["D"][g][1], want["D"][1])
        assert _same(out["states"][g][0], want["states"][0][0]) and _same(out["states"][g][1], want["states"][0][1])
        assert _same(out["pose"][g], want["pose"][0]) and _same(out["pose_rig"][g], want["pose_rig"])
        assert _same(out["stats"][g], want["stats"][0]) and _same(out["stats_group"][g], want["stats_group"])
        assert _same(out["stats_view"][0, :, 0].sum(), out["stats"][:, :, 0].sum())


def test_no_free_view_is_the_joint_step():
    """the gauge camera's counts are scripted below the bound: every other view is held, and the step is joint_refine's"""
    G, V = 2, 3

    def few_in_camera_0(g, v, s):
        s = s.copy()
        if v == 0:
            s[27] = 10.0
        return s

    scenes, X, pose_in, rig_in = _inputs(G, V, 6)
    out = rr.rig_refine(_model_sums(scenes, V, few_in_camera_0), X, G, 3, pose_in, rig_in)
    assert out["status"].tolist() == [0, HELD, HELD] * G and not np.any(out["moved"]) and _same(out["cam_T_rig"], X)
    for g in range(G):
        rows = slice(g * V, (g + 1) * V)
        want = vr.joint_refine(lambda v, R, t: few_in_camera_0(g, v, scenes[g * V + v].partial(R, t, np.float32)[0].sum(axis=0)),
                               X, 3, pose_in[rows], rig_in[g])
        assert want["stepped"] and not want["failed"]
        assert _same(out["pose"][rows], want["pose"]) and _same(out["pose_rig"][g], want["pose_rig"])
        for v in range(V):
            assert _same(out["states"][g * V + v][0], want["states"][v][0]) and _same(out["states"][g * V + v][1], want["states"][v][1])


# ------------------------------------------------------------------------------------------------------------------ Schur against dense
@pytest.mark.parametrize("G,V", [(1, 2), (2, 2), (1, 3), (3, 2), (2, 8), (1, 16)])
def test_schur_against_dense(G, V):
    scenes, X, pose_in, rig_in = _inputs(G, V, 10 * G + V)
    out = rr.rig_refine(_model_sums(scenes, V), X, G, 3, pose_in, rig_in)
    assert not np.any(out["status"]) and np.all(out["moved"][1:]) and np.all(out["stepped"])
    for k, step in enumerate(out["steps"]):
        bk = step["blocks"]
        assert bk["fl"] == list(range(1, V)) and bk["gl"] == list(range(G))
        H, _ = rr.dense_system(bk)
        assert np.all(np.linalg.eigvalsh(H) > 0)                          # positive definite
        schur, dense = rr.schur_solve(bk), rr.dense_solve(bk)
        x_s = np.concatenate([schur[0][v] for v in bk["fl"]] + [schur[1][g] for g in bk["gl"]])
        x_d = np.concatenate([dense[0][v] for v in bk["fl"]] + [dense[1][g] for g in bk["gl"]])
        tol = 1e3 * EPS64 * np.linalg.cond(H)
        print("G={} V={} k={}: |schur - dense| {:.3g}, |x| {:.3g}, cond {:.3g}".format(G, V, k, np.abs(x_s - x_d).max(), np.abs(x_d).max(),
                                                                                      np.linalg.cond(H)))
        assert np.abs(x_s - x_d).max() <= tol * np.abs(x_d).max()
    dense_out = rr.rig_refine(_model_sums(scenes, V), X, G, 3, pose_in, rig_in, solve=rr.dense_solve)
    assert np.abs(dense_out["pose"] - out["pose"]).max() <= 1e-5 and np.abs(dense_out["cam_T_rig"] - out["cam_T_rig"]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ convergence, gauge
def _plane_errors(p, out):
    Xc = rr.current_extrinsics(p.X, out["C"], out["moved"])
    e_x = np.abs(Xc - p.X_true).max()
    e_p = max(np.abs(vr.mul(vr.mat(*out["D"][g]), p.P[g]) - p.P_true[g]).max() for g in range(p.G))
    return e_x, e_p


def test_convergence_on_fixed_correspondences():
    p = rr.PlaneProblem(G=3, V=3, n=200)
    errors = [_plane_errors(p, rr.rig_refine(p.sums, p.X, p.G, n, p.pose_in, p.P)) for n in range(5)]
    print("extrinsic and pose error after 0..4 iterations:", errors)
    assert errors[0][0] > 1e-3 and errors[0][1] > 1e-3                    # about 0.5 degrees and 5 mm off
    assert errors[4][0] < 1e-12 and errors[4][1] < 1e-12
    assert errors[2][0] < 1e-3 * errors[1][0]                             # quadratic, not linear


def test_gauge_camera_keeps_its_bits():
    p = rr.PlaneProblem(G=2, V=3, n=100, seed=3)
    X32 = p.X.astype(np.float32)
    out = rr.rig_refine(p.sums, X32, p.G, 3, p.pose_in, p.P)
    assert _same(out["cam_T_rig"][0], X32[0]) and not out["moved"][0] and np.all(out["moved"][1:])
    assert out["C"][0] is rr.IDENTITY
    assert np.abs(out["cam_T_rig"][1:] - X32[1:]).max() > 1e-4


# ------------------------------------------------------------------------------------------------------------------ the branch table
def _scripted(rng, N, bad=False):
    """29 sums of N random points with unit normals around (0, 0, 1); bad: a system that cannot pass the Cholesky"""
    if N == 0:
        return np.zeros(29)
    p = rng.uniform(-0.1, 0.1, (int(N), 3)) + [0, 0, 1.0]
    n = rng.normal(size=(int(N), 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    J = np.concatenate([np.cross(p, n), n], axis=1)
    r = rng.normal(size=int(N)) * 1e-3
    A = -np.eye(6) if bad else J.T @ J
    return vr.pack_sums(A, J.T @ r, N, float(r @ r))


#        name                counts (G x V)              bad (g, v)  iters  FEW on         HELD on views  moved views  stepped groups
TABLE = [
    ("all-in",               [[100, 100], [100, 100]],   None,       2,     [],            [],            [1],         [0, 1]),
    ("inactive-group",       [[100, 100], [30, 33]],     None,       2,     [2, 3],        [],            [1],         [0]),
    ("held-view",            [[100, 63, 100]],           None,       2,     [],            [1],           [2],         [0]),
    ("free-through-gauge",   [[0, 100], [100, 100]],     None,       1,     [],            [],            [1],         [0, 1]),
    ("held-without-gauge",   [[0, 100], [63, 100]],      None,       1,     [],            [1],           [],          [0, 1]),
    ("bad-pivot",            [[100, 100], [100, 100]],   (1, 0),     2,     [0, 1, 2, 3],  [],            [],          []),
    ("bad-pivot-no-free",    [[10, 100], [10, 100]],     (1, 1),     2,     [2, 3],        [1],           [],          [0]),
    ("never-steps",          [[100, 100], [0, 0]],       None,       3,     [2, 3],        [],            [1],         [0]),
    ("no-iterations",        [[100, 100]],               None,       0,     [],            [],            [],          []),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_branch_table(row):
    _, counts, bad, iters, few, held, moved, stepped = row
    G, V = len(counts), len(counts[0])
    rng = np.random.default_rng(5)
    table = [[_scripted(rng, counts[g][v], bad == (g, v)) for v in range(V)] for g in range(G)]
    X, pose_in, rig_in = vs.rig(2, V), np.tile(vs.rig_poses(3, 1), (G * V, 1, 1)), vs.rig_poses(4, G)
    out = rr.rig_refine(lambda g, v, R, t: table[g][v], X, G, iters, pose_in, rig_in)
    want = np.zeros(G * V, np.int64)
    want[few] |= FEW
    for v in held:
        want[v::V] |= HELD
    assert out["status"].tolist() == want.tolist()
    assert np.flatnonzero(out["moved"]).tolist() == moved and np.flatnonzero(out["stepped"]).tolist() == stepped
    assert _same(out["cam_T_rig"][0], X[0])
    for v in range(V):
        assert _same(out["cam_T_rig"][v], X[v]) == (v not in moved)       # a view that never moved: its nominal row, bit for bit
    for g in range(G):
        rows = slice(g * V, (g + 1) * V)
        if g in stepped:
            assert np.abs(out["pose_rig"][g] - rig_in[g]).max() > 0 and np.abs(out["pose"][rows] - pose_in[rows]).max() > 0
        else:                                                             # a group that never stepped: its inputs, bit for bit
            assert _same(out["pose_rig"][g], rig_in[g]) and _same(out["pose"][rows], pose_in[rows])
    assert out["stats"].shape == (G * V, iters, 2) and out["stats_view"].shape == (V, iters, 2)
    if iters:
        assert out["stats"][:, 0, 0].tolist() == [float(c) for c in np.ravel(counts)]
        assert out["stats_view"][:, 0, 0].tolist() == [float(c) for c in np.sum(counts, axis=0)]
        assert out["stats_group"][:, 0, 0].tolist() == [float(c) for c in np.sum(counts, axis=1)]


# ------------------------------------------------------------------------------------------------------------------ the Python layer
def _fresh():
    from deepim.config.config import config, reset_config

    reset_config()
    return config


def test_settings_defaults_and_refusals_name_their_keys():
    from deepim.core.views import calib_settings, views_settings

    cfg = _fresh()
    try:
        assert cfg.TEST.VIEWS_CALIB_ITER == 0 and cfg.TEST.VIEWS_CALIB_MAX_DIST is None
        assert calib_settings(cfg) == (0, float(cfg.TEST.ICP_MAX_DIST))
        cfg.TEST.ICP_MAX_DIST = 0.03
        assert calib_settings(cfg) == (0, 0.03)                           # the gate defaults to ICP_MAX_DIST
        cfg.TEST.VIEWS_CALIB_MAX_DIST = 0.01
        assert calib_settings(cfg) == (0, 0.01)
        cfg.TEST.VIEWS_CALIB_ITER = 4
        with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_ITER > 0 needs TEST\.VIEWS > 1"):
            calib_settings(cfg)
        cfg.TEST.VIEWS = 2
        assert calib_settings(cfg) == (4, 0.01)
        for bad in (-1, 2.5, True, "x"):
            cfg.TEST.VIEWS_CALIB_ITER = bad
            with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_ITER"):
                calib_settings(cfg)
        cfg.TEST.VIEWS_CALIB_ITER = 4
        for bad in (0.0, -0.01, float("nan"), float("inf")):
            cfg.TEST.VIEWS_CALIB_MAX_DIST = bad
            with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_MAX_DIST"):
                calib_settings(cfg)
        cfg.TEST.VIEWS_CALIB_MAX_DIST = None
        for key, on in (("HYP_NUM", 2), ("COARSE_VIEWS", 8), ("FLOW_PNP_ITER", 4)):   # what VIEWS > 1 refuses stays refused
            cfg.TEST[key] = on
            with pytest.raises(ValueError, match=r"TEST\.VIEWS.*TEST\.{}".format(key)):
                views_settings(cfg)
            cfg.TEST[key] = {"HYP_NUM": 1}.get(key, 0)
    finally:
        _fresh()


def test_one_rig_check_and_round_trip():
    from deepim.core.views import check_cam_T_rig, check_one_rig

    rng = np.random.default_rng(11)
    rig = np.stack([vr.random_rigid(rng) for _ in range(3)]).astype(np.float32)
    full = check_cam_T_rig(rig, 6, 3)
    assert _same(check_one_rig(full, 3), full)
    other = full.copy()
    other[4, 0, 3] = np.nextafter(other[4, 0, 3], np.float32(9))          # one ulp in camera 1 of group 1
    check_cam_T_rig(other, 6, 3)                                          # rigid still: the joint stages take it
    with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_ITER.*cam_T_rig\[4\].*cam_T_rig\[1\]"):
        check_one_rig(other, 3)
    # what a calibration returns is accepted by the next load
    p = rr.PlaneProblem(G=2, V=3, n=100, seed=8)
    out = rr.rig_refine(p.sums, p.X.astype(np.float32), p.G, 4, p.pose_in, p.P)
    assert np.all(out["moved"][1:]) and out["cam_T_rig"].dtype == np.float32
    again = check_cam_T_rig(out["cam_T_rig"], 6, 3)
    assert _same(check_one_rig(again, 3)[:3], out["cam_T_rig"])
