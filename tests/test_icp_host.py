"""CPU: the depth ICP after the refinement loop -- the float64 restatement (tests/icp_reference.py) converges on seeded synthetic
depth, the new TEST keys, the host side of the C ABI (dim_icp_workspace_bytes, argument checks before any device call) and the
out["icp"] table of pred_eval with a fake refiner on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import icp_reference as ir
from conftest import ROOT

ICP_NOISE = dict(angle_std=2.0, angle_max=6.0, xy_std=0.003, z_std=0.01)


def icp_pairs(B, seed=7):
    """-> models, class_index, pose_gt, pose_init: B seeded pairs of lib/utils/synthetic.py, init = GT perturbed by a few degrees and
    millimetres (the range a refinement loop leaves for the ICP)"""
    from lib.utils import synthetic as syn

    models = syn.make_models(seed=2333, n_models=1, subdiv=4)
    cls, gt, init = syn.sample_pairs(seed, B, **ICP_NOISE)
    return models, cls, gt, init


def noisy_depth(depth, seed):
    """mm-quantised depth plus Gaussian noise (sigma 1 mm) where there is a reading"""
    rng = np.random.default_rng(seed)
    d = np.round(depth * 1000.0) / 1000.0 + rng.normal(0.0, 1e-3, depth.shape)
    return np.where(depth > 0, d, 0.0).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    from lib.utils import synthetic as syn
    from oracle import native

    models, cls, gt, init = icp_pairs(8)
    v, t, f, tex = models[0]
    K = syn.LINEMOD_K
    Dr = np.stack([native.render(v, t, f, tex, p[:, :3], p[:, 3], K)[1] for p in init])
    Do = np.stack([native.render(v, t, f, tex, p[:, :3], p[:, 3], K)[1] for p in gt])
    return v.astype(np.float64), K, gt, init, Dr, Do


def test_restatement_converges_on_exact_depth(scene):
    pts, K, gt, init, Dr, Do = scene
    pose, stats, status = ir.icp_refine(Dr, Do, init, K, 10, 0.02)
    assert status.tolist() == [0] * 8
    for b in range(8):
        assert ir.add_error(init[b], gt[b], pts) > 2e-3, b     # the input is off by millimetres
        assert ir.add_error(pose[b], gt[b], pts) <= 1e-3, b
        assert np.linalg.norm(pose[b][:, 3].astype(np.float64) - gt[b][:, 3]) <= 5e-4, b
        assert stats[b, 0, 0] > 4 * ir.MIN_POINTS and stats[b, -1, 1] < stats[b, 0, 1], b


def test_restatement_converges_on_noisy_depth(scene):
    pts, K, gt, init, Dr, Do = scene
    pose, stats, status = ir.icp_refine(Dr, noisy_depth(Do, 1), init, K, 10, 0.02)
    assert status.tolist() == [0] * 8
    before = np.array([ir.add_error(init[b], gt[b], pts) for b in range(8)])
    after = np.array([ir.add_error(pose[b], gt[b], pts) for b in range(8)])
    assert after.mean() <= 3e-3, after
    assert int(np.sum(after < before)) >= 7, (before, after)


def test_negative_control_tight_gate_flags_and_keeps_the_pose(scene):
    """1 cm of depth error against a 1 mm gate: no inlier, the pair is flagged and its pose is the input's, bit for bit"""
    pts, K, gt, init, Dr, Do = scene
    start = gt[:1].copy()
    start[0, 2, 3] += 0.01
    from oracle import native

    models, _, _, _ = icp_pairs(1)
    v, t, f, tex = models[0]
    dr = native.render(v, t, f, tex, start[0][:, :3], start[0][:, 3], K)[1]
    pose, stats, status = ir.icp_refine(dr[None], Do[:1], start, K, 3, 1e-3)
    assert status.tolist() == [ir.STATUS_ICP_FEW_POINTS]
    assert np.array_equal(pose.view(np.uint32), start.view(np.uint32))
    assert stats[0, :, 0].max() < ir.MIN_POINTS
    # the same pair with the default gate does move
    pose2, _, status2 = ir.icp_refine(dr[None], Do[:1], start, K, 3, 0.02)
    assert status2.tolist() == [0] and ir.add_error(pose2[0], gt[0], pts) < 1e-3 < ir.add_error(start[0], gt[0], pts)


def test_bbox_restricts_the_source_points(scene):
    pts, K, gt, init, Dr, Do = scene
    ys, xs = np.nonzero(Dr[0] > 0)
    full = ir.source_points(Dr[0], K)
    box = ir.source_points(Dr[0], K, [xs.min(), xs.max(), ys.min(), ys.max()])
    np.testing.assert_array_equal(full, box)
    assert len(ir.source_points(Dr[0], K, [640, -1, 480, -1])) == 0    # the render's empty box
    half = ir.source_points(Dr[0], K, [xs.min(), (xs.min() + xs.max()) // 2, ys.min(), ys.max()])
    assert 0 < len(half) < len(full)


# ------------------------------------------------------------------------------------------------------------------ config
def test_config_defaults_and_yaml_merge(tmp_path):
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    assert config.TEST.ICP_ITER == 0 and config.TEST.ICP_MAX_DIST == 0.02
    assert config.TEST.PRECOMPUTED_ICP is False and config.TEST.BEFORE_ICP is False
    p = tmp_path / "icp.yaml"
    p.write_text("TEST:\n  ICP_ITER: 10\n  ICP_MAX_DIST: 0.015\n  test_iter: 4\n")
    update_config(str(p))
    assert config.TEST.ICP_ITER == 10 and config.TEST.ICP_MAX_DIST == 0.015 and config.TEST.test_iter == 4
    assert config.TEST.FAST_TEST is False   # untouched keys keep their defaults
    reset_config()
    assert config.TEST.ICP_ITER == 0


def test_shipped_yaml_keeps_icp_off():
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    update_config(os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test.yaml"))
    assert config.TEST.ICP_ITER == 0
    reset_config()


# ------------------------------------------------------------------------------------------------------------------ C ABI, host side
def test_workspace_bytes(hip_lib):
    per_pair = (16 + 16 * 32) * 8     # T_delta state + 16 workgroup partials of 32 doubles
    assert hip_lib.dim_icp_workspace_bytes(1, 480, 640) == per_pair
    assert hip_lib.dim_icp_workspace_bytes(16, 480, 640) == 16 * per_pair
    assert hip_lib.dim_icp_workspace_bytes(16, 48, 64) == 16 * per_pair
    assert hip_lib.dim_icp_workspace_bytes(0, 480, 640) == 0


def test_bad_arguments_return_err_arg_without_a_device(hip_lib):
    K9 = (ctypes.c_float * 9)(572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is enqueued

    def call(B=2, H=480, W=640, iters=10, max_dist=0.02, dr=fake, do=fake, pose=fake, k9=K9, ws=fake, out=fake):
        return hip_lib.dim_icp_refine(dr, do, None, None, pose, k9, None, B, H, W, iters, max_dist, ws, out, None, None, None)

    cases = {"B=0": dict(B=0), "B<0": dict(B=-3), "iters<0": dict(iters=-1), "max_dist=0": dict(max_dist=0.0),
             "max_dist<0": dict(max_dist=-0.01), "max_dist=nan": dict(max_dist=float("nan")), "W=2": dict(W=2), "H=2": dict(H=2),
             "depth_rendered": dict(dr=None), "depth_observed": dict(do=None), "pose_in": dict(pose=None), "K9": dict(k9=None),
             "workspace": dict(ws=None), "pose_out": dict(out=None)}
    for name, kw in cases.items():
        assert call(**kw) == -1, name
        assert hip_lib.dim_last_error().decode().startswith("icp_refine"), name


# ------------------------------------------------------------------------------------------------------------------ pred_eval
class _FakeNet(object):
    device = "cpu"


class _FakeRefiner(object):
    """stands in for deepim.core.tester.Refiner: fixed poses per batch on CPU tensors; records what load() received"""

    def __init__(self, B, poses_iter, poses_icp, icp):
        self.B, self.net = B, _FakeNet()
        self._poses, self._icp = list(poses_iter), list(poses_icp)
        self.icp = icp
        self.loaded_depth = []
        self.pose_icp = None

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None):
        self.loaded_depth.append(depth_observed)
        self.pose_icp = torch.from_numpy(self._icp.pop(0)) if self.icp else None
        self._cur = torch.from_numpy(self._poses.pop(0))

    def refine(self):
        return self._cur


def _fake_run(icp, n_batches=2, B=4, test_iter=3):
    from deepim.core.tester import pred_eval
    from lib.dataset.evaluation import PoseEvaluator
    from scene import make_test_config

    cfg = make_test_config(test_iter=test_iter)
    cfg.dataset.class_name = ["ape", "cat"]
    cfg.TEST.ICP_ITER = 10 if icp else 0
    rng = np.random.default_rng(5)
    pts = {c: rng.uniform(-0.05, 0.05, size=(200, 3)) for c in cfg.dataset.class_name}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, {c: 0.15 for c in cfg.dataset.class_name})
    batches, iters, icps = [], [], []
    for k in range(n_batches):
        from lib.utils import synthetic as syn

        cls, gt, init = syn.sample_pairs(100 + k, B, n_classes=2)
        init = init.copy()
        if k == 1:
            init[2] = -1.0   # undetected (tester.py:419-445)
        steps = np.stack([gt + rng.normal(0, 0.02 / (it + 1), gt.shape).astype(np.float32) for it in range(test_iter)])
        iters.append(steps.astype(np.float32))
        icps.append((gt + rng.normal(0, 0.001, gt.shape)).astype(np.float32))
        z = torch.zeros((B, 1, 4, 4))
        batches.append({"image_observed": z, "image_rendered": z, "mask_observed": z, "mask_rendered": z, "src_pose": torch.from_numpy(init),
                        "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt), "depth_observed": z + 0.5})
    ref = _FakeRefiner(B, iters, icps, icp)
    out = pred_eval(cfg, ref, batches, ev)
    return cfg, out, ref, batches


def _same(a, b, path="out"):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "{}[{!r}]".format(path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "{}[{}]".format(path, i))
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=path)
    else:
        assert a == b, path


def test_pred_eval_scores_icp_as_one_row_table():
    cfg_off, off, _, _ = _fake_run(False)
    assert "icp" not in off
    cfg, on, ref, batches = _fake_run(True)
    assert int(cfg.TEST.test_iter) == 3   # the one-row scoring does not touch the config
    assert all(d is not None for d in ref.loaded_depth) and torch.equal(ref.loaded_depth[0], batches[0]["depth_observed"])
    _same({k: v for k, v in on.items() if k != "icp"}, off)
    icp = on["icp"]
    assert set(icp) >= {"pose", "add", "arp_2d"}
    assert icp["pose"]["rot_acc"].shape == (2, 1, 10) and len(icp["pose"]["overall"]) == 1
    assert len(icp["add"]["overall"]) == 1 and len(icp["arp_2d"]["overall"]) == 1
    # 8 pairs over the two classes, one undetected: scored as the loop scores it, 1000 deg / 1000 m
    rot = [r for c in range(2) for r in icp["all_rot_err"][c][0]]
    trans = [t for c in range(2) for t in icp["all_trans_err"][c][0]]
    assert len(rot) == 8 and sorted(rot)[-1] == 1000 and sorted(trans)[-1] == 1000 and sorted(rot)[-2] < 10
    loop_last = [r for c in range(2) for r in on["all_rot_err"][c][2]]
    assert sorted(loop_last)[-1] == 1000
    # the ICP poses (1 mm off) score better than the loop's last row (7 mm off)
    assert icp["add"]["overall"][0]["0.02"] >= on["add"]["overall"][2]["0.02"]
    assert icp["add"]["overall"][0]["auc"] > on["add"]["overall"][2]["auc"]
