"""CPU: several hypotheses per pair -- the TEST.HYP_* keys and their checks, the rotation table of deepim.core.tester against the
float64 restatement tests/hyp_reference.py, the restatement itself on hand-made cases, the host side of the C ABI, and pred_eval's
out["hyp"] with a fake refiner on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hyp_reference as hr
from conftest import ROOT

NEW_SYMBOLS = ("dim_hyp_expand", "dim_hyp_broadcast", "dim_pose_score_workspace_bytes", "dim_pose_score", "dim_hyp_select")


def test_config_defaults():
    from deepim.config.config import config, reset_config

    reset_config()
    assert config.TEST.HYP_NUM == 1 and config.TEST.HYP_ROT_DEG == 30.0
    assert config.TEST.HYP_SCORE == "rgb" and config.TEST.HYP_DEPTH_TAU == 0.02
    from deepim.core.tester import hyp_settings

    assert hyp_settings(config) == (1, 30.0, "rgb", 0.02)


@pytest.mark.parametrize("key,value", [("HYP_NUM", 0), ("HYP_NUM", 2.5), ("HYP_NUM", -3), ("HYP_SCORE", "mask"), ("HYP_SCORE", None),
                                       ("HYP_DEPTH_TAU", 0.0), ("HYP_DEPTH_TAU", -0.01), ("HYP_DEPTH_TAU", float("nan")),
                                       ("HYP_ROT_DEG", float("inf"))])
def test_config_validation(key, value):
    from deepim.config.config import config, reset_config
    from deepim.core.tester import hyp_settings

    reset_config()
    config.TEST[key] = value
    try:
        with pytest.raises(ValueError, match=key):
            hyp_settings(config)
    finally:
        reset_config()


def test_rotation_table():
    from deepim.core.tester import hypothesis_rotations

    for N in (1, 2, 4, 8, 17):
        R = hypothesis_rotations(N, 30.0)
        assert R.shape == (N, 3, 3)
        np.testing.assert_array_equal(R[0], np.eye(3))   # hypothesis 0: the loaded pose
        np.testing.assert_array_equal(R, hypothesis_rotations(N, 30.0))   # deterministic
        np.testing.assert_allclose(R, hr.rotation_table(N, 30.0), rtol=0, atol=1e-12)
        for h in range(1, N):
            np.testing.assert_allclose(R[h] @ R[h].T, np.eye(3), atol=1e-12)
            assert abs(np.linalg.det(R[h]) - 1.0) < 1e-12
            ang = np.degrees(np.arccos(np.clip((np.trace(R[h]) - 1.0) / 2.0, -1.0, 1.0)))
            assert abs(ang - 30.0) < 1e-6, (N, h, ang)
        flat = R.reshape(N, 9)
        for i in range(N):
            for j in range(i + 1, N):
                assert np.abs(flat[i] - flat[j]).max() > 1e-3, (N, i, j)   # distinct
    for M in (1, 3, 7, 16):
        A = hr.fibonacci_axes(M)
        np.testing.assert_allclose(np.linalg.norm(A, axis=1), 1.0, atol=1e-12)   # unit axes
        assert len({tuple(np.round(a, 9)) for a in A}) == M


def test_restatement_expand():
    from lib.utils import synthetic as syn

    _, gt, _ = syn.sample_pairs(3, 3)
    T = hr.rotation_table(4, 45.0)
    out = hr.expand(T, gt)
    for p in range(3):
        np.testing.assert_array_equal(out[p * 4], gt[p].astype(np.float64))
        for h in range(1, 4):
            np.testing.assert_allclose(out[p * 4 + h][:, :3], T[h] @ gt[p][:, :3], atol=1e-12)
            np.testing.assert_array_equal(out[p * 4 + h][:, 3], gt[p][:, 3])   # about the object origin: t stays


def _planes(H=24, W=32, seed=0):
    rng = np.random.default_rng(seed)
    obs = rng.normal(0, 20, (3, H, W))
    ren = rng.normal(0, 20, (3, H, W))
    dr = np.zeros((H, W))
    dr[4:20, 6:26] = 0.8
    return obs, ren, dr


def test_restatement_rgb_score():
    obs, ren, dr = _planes()
    # the same image up to gain and offset -> 1; inverted -> -1
    assert hr.score_one("rgb", obs, 3.0 * obs + 7.0, dr) == pytest.approx(1.0, abs=1e-12)
    assert hr.score_one("rgb", obs, -obs, dr) == pytest.approx(-1.0, abs=1e-12)
    s = hr.score_one("rgb", obs, ren, dr)
    assert -0.3 < s < 0.3
    # only S counts: the pixels outside the drawn region do not matter
    obs2 = obs.copy()
    obs2[:, 0:4] = 1e6
    assert hr.score_one("rgb", obs2, ren, dr) == s
    # a box that cuts S
    s_box = hr.score_one("rgb", obs, ren, dr, bbox=(6, 15, 4, 19))
    a = obs.sum(0)[4:20, 6:16].ravel()
    r = ren.sum(0)[4:20, 6:16].ravel()
    assert s_box == pytest.approx(np.corrcoef(a, r)[0, 1], abs=1e-12)
    # a large common offset: the same score
    assert hr.score_one("rgb", obs + 400.0, ren, dr) == pytest.approx(s, abs=1e-12)
    # constant plane, too few pixels, empty box, NaN: -inf
    assert hr.score_one("rgb", np.full_like(obs, 5.0), ren, dr) == -np.inf
    assert hr.score_one("rgb", obs, np.full_like(ren, 5.0), dr) == -np.inf
    assert hr.score_one("rgb", obs, ren, dr, bbox=(6, 12, 4, 9)) == -np.inf   # 7 x 6 = 42 < 64 pixels
    assert hr.score_one("rgb", obs, ren, dr, bbox=(32, -1, 24, -1)) == -np.inf
    nan = obs.copy()
    nan[0, 10, 10] = np.nan
    assert hr.score_one("rgb", nan, ren, dr) == -np.inf


def test_restatement_depth_score():
    _, _, dr = _planes()
    do = dr.copy()
    assert hr.score_one("depth", None, None, dr, depth_observed=do, tau=0.02) == 1.0
    do[4:12] += 0.05   # half of S beyond the gate
    assert hr.score_one("depth", None, None, dr, depth_observed=do, tau=0.02) == pytest.approx(0.5)
    do[4:12] = 0.0     # no reading there: not counted
    assert hr.score_one("depth", None, None, dr, depth_observed=do, tau=0.02) == 1.0
    assert hr.score_one("depth", None, None, dr, depth_observed=np.zeros_like(dr), tau=0.02) == -np.inf
    assert hr.score_one("depth", None, None, dr, depth_observed=np.full_like(dr, np.nan), tau=0.02) == -np.inf


def test_restatement_select():
    c, none = hr.select([0.1, 0.5, 0.5, -np.inf, np.nan, -np.inf, -np.inf, np.inf, 0.2, np.nan, 0.2, 0.3], 4)
    assert c.tolist() == [1, 0, 3] and none.tolist() == [False, True, False]   # ties: smaller h; +inf is not finite
    c, none = hr.select([np.nan, -0.9, 0.4, 0.4], 2)
    assert c.tolist() == [1, 0] and none.tolist() == [False, False]
    poses = np.arange(2 * 6 * 12, dtype=np.float64).reshape(2, 6, 3, 4)
    st = np.arange(12).reshape(2, 6)
    icp = -np.arange(6 * 12, dtype=np.float64).reshape(6, 3, 4)
    p, s, i = hr.gather(np.array([2, 0]), 3, poses, st, icp)
    np.testing.assert_array_equal(p, poses[:, [2, 3]])
    np.testing.assert_array_equal(s, st[:, [2, 3]])
    np.testing.assert_array_equal(i, icp[[2, 3]])


def test_header_ctypes_and_library(hip_lib):
    from lib.hip import capi

    header = open(os.path.join(ROOT, "include", "deepim_hip.h")).read()
    assert "#define DIM_STATUS_HYP_NO_SCORE 64" in header
    assert "#define DIM_HYP_SCORE_RGB 0" in header and "#define DIM_HYP_SCORE_DEPTH 1" in header
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in capi.SIGNATURES, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.dim_pose_score_workspace_bytes(64, 480, 640) == 64 * 16 * 16 * 8
    assert hip_lib.dim_pose_score_workspace_bytes(0, 480, 640) == 0


def test_argument_checks_before_any_device_call(hip_lib):
    """bad sizes and NULL pointers return DIM_ERR_ARG (-1) on the host, before anything is launched"""
    fake = ctypes.c_void_p(16)
    assert hip_lib.dim_hyp_expand(fake, fake, 0, 4, fake, None) == -1
    assert hip_lib.dim_hyp_expand(None, fake, 2, 4, fake, None) == -1
    assert hip_lib.dim_hyp_broadcast(fake, fake, 2, 0, 16, None) == -1
    assert hip_lib.dim_hyp_broadcast(fake, None, 2, 2, 16, None) == -1
    assert hip_lib.dim_pose_score(fake, fake, None, fake, None, 2, 480, 640, 2, 0.02, fake, fake, None, None) == -1   # mode
    assert hip_lib.dim_pose_score(fake, fake, None, fake, None, 2, 480, 640, 1, 0.02, fake, fake, None, None) == -1   # no depth
    assert hip_lib.dim_pose_score(fake, fake, fake, fake, None, 2, 480, 640, 1, 0.0, fake, fake, None, None) == -1    # tau
    assert hip_lib.dim_pose_score(fake, fake, None, fake, None, 0, 480, 640, 0, 0.02, fake, fake, None, None) == -1
    assert hip_lib.dim_hyp_select(fake, 2, 4, 0, fake, None, None, None, fake, fake, None, None, None) == -1
    assert hip_lib.dim_hyp_select(None, 2, 4, 3, fake, None, None, None, fake, fake, None, None, None) == -1
    assert b"pose_score" in hip_lib.dim_last_error() or b"hyp_select" in hip_lib.dim_last_error()


def test_c_loop_object_refuses_hypotheses():
    from lib.hip.refiner_capi import CRefiner
    from scene import make_test_config

    cfg = make_test_config()
    cfg.TEST.HYP_NUM = 4
    try:
        with pytest.raises(ValueError, match="HYP_NUM"):
            CRefiner(cfg, {}, None, 2)
    finally:
        cfg.TEST.HYP_NUM = 1


# ------------------------------------------------------------------------------------------------------------------ pred_eval
class _FakeHypRefiner(object):
    """what pred_eval reads from a Refiner with N hypotheses, on CPU tensors"""

    def __init__(self, P, N, runs):
        self.P, self.N, self.B = P, N, P * N
        self._runs = runs
        self.pose_icp = self.pose_icp_sel = None
        self.loaded = []

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None, hyp_poses=None):
        self.loaded.append(hyp_poses)
        self.poses_iter, self.hyp_score, self.hyp_choice, self._sel = self._runs.pop(0)

    def refine(self):
        return self._sel


def test_pred_eval_scores_the_winners():
    from deepim.core.tester import pred_eval
    from lib.dataset.evaluation import PoseEvaluator
    from lib.utils import synthetic as syn
    from scene import make_test_config

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "cat"]
    rng = np.random.default_rng(5)
    pts = {c: rng.uniform(-0.05, 0.05, size=(200, 3)) for c in cfg.dataset.class_name}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, {c: 0.15 for c in cfg.dataset.class_name})
    P, N, T = 4, 3, 2
    batches, runs, want_sel, want_best = [], [], [], []
    for k in range(2):
        cls, gt, init = syn.sample_pairs(200 + k, P, n_classes=2)
        # hypothesis h of pair p ends (h+1) * 2 degrees off about x; the score favours h = (p + k) % N
        poses = np.zeros((T, P * N, 3, 4), np.float32)
        for p in range(P):
            for h in range(N):
                a = np.radians(2.0 * (h + 1))
                Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
                poses[:, p * N + h, :, :3] = Rx @ gt[p][:, :3]
                poses[:, p * N + h, :, 3] = gt[p][:, 3]
        score = np.full((P * N,), 0.1, np.float32)
        choice = np.array([(p + k) % N for p in range(P)], np.int32)
        score[np.arange(P) * N + choice] = 0.9
        sel = poses[:, np.arange(P) * N + choice]
        runs.append((torch.from_numpy(poses), torch.from_numpy(score), torch.from_numpy(choice), torch.from_numpy(sel)))
        want_sel.append(sel)
        want_best += [int(c) == 0 for c in choice]
        z = torch.zeros((P, 1, 4, 4))
        batches.append({"image_observed": z, "image_rendered": z, "mask_observed": z, "mask_rendered": z, "src_pose": torch.from_numpy(init),
                        "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt)})
    ref = _FakeHypRefiner(P, N, runs)
    out = pred_eval(cfg, ref, batches, ev)
    hyp = out["hyp"]
    assert hyp["num"] == N and len(hyp["choice"]) == 2 * P and len(hyp["score"]) == 2 * P
    assert hyp["choice"] == [int(c) for r in (0, 1) for c in [(p + r) % N for p in range(P)]]
    for p in range(2 * P):
        assert len(hyp["rot_err"][p]) == N and np.argmin(hyp["rot_err"][p]) == 0
        np.testing.assert_allclose(hyp["rot_err"][p], [2.0, 4.0, 6.0], atol=1e-3)
    assert hyp["chosen_is_least_rot_err"] == pytest.approx(np.mean(want_best))
    # the tables score the selected trajectory: its last-iteration errors are those of the chosen hypotheses
    last = sorted(r for c in range(2) for r in out["all_rot_err"][c][T - 1])
    chosen = sorted(hyp["rot_err"][p][hyp["choice"][p]] for p in range(2 * P))
    np.testing.assert_allclose(last, chosen, atol=1e-9)
    assert ref.loaded == [None, None]
