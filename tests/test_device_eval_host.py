"""CPU: the host side of TEST.DEVICE_EVAL -- the config key, PoseEvaluator's `errors=` option against its own recomputation on seeded
poses (a plain class, glue = ADD-S, eggbox with estimates past 90 degrees), and the argument checks of dim_pose_errors (nothing is
enqueued: no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN


def test_config_default_and_yaml(tmp_path):
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    assert config.TEST.DEVICE_EVAL is False
    src = os.path.join(GOLDEN, "cfgs", "deepim_flownet_LM_SIXD_v1_ape_RFMx4_8epoch.yaml")
    import yaml

    with open(src) as f:
        y = yaml.safe_load(f)
    y["TEST"]["DEVICE_EVAL"] = True
    p = tmp_path / "device_eval.yaml"
    p.write_text(yaml.safe_dump(y))
    try:
        update_config(str(p))
        assert config.TEST.DEVICE_EVAL is True
    finally:
        reset_config()


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _pose(rng):
    R = _rot(rng.normal(size=3), rng.uniform(0, 180))
    t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.2)])
    return np.concatenate([R, t[:, None]], axis=1)


def _seeded_lists(n_it=2, n_pose=12, seed=5):
    """-> evaluator, classes, all_poses_est[cls][iter], all_poses_gt[cls][iter]: estimates 0.5-12 deg / up to 3 cm from the ground
    truth; the eggbox class also holds estimates turned 120-179 deg about z (the flip rule) and one near 100 deg about x"""
    from lib.dataset.evaluation import PoseEvaluator

    rng = np.random.default_rng(seed)
    classes = ["ape", "glue", "eggbox"]
    pts = {c: rng.uniform(-0.05, 0.05, size=(n, 3)) * np.array([1.0, 0.6, 0.3]) for c, n in zip(classes, (200, 150, 180))}
    diam = {c: float(np.linalg.norm(p.max(0) - p.min(0))) for c, p in pts.items()}
    est = [[[] for _ in range(n_it)] for _ in classes]
    gt = [[[] for _ in range(n_it)] for _ in classes]
    for c, name in enumerate(classes):
        for j in range(n_pose):
            g = _pose(rng)
            for it in range(n_it):
                d = _rot(rng.normal(size=3), rng.uniform(0.5, 12.0) / (it + 1))
                e = np.concatenate([d @ g[:, :3], (g[:, 3] + rng.normal(size=3) * 0.01 / (it + 1))[:, None]], axis=1)
                if name == "eggbox" and j % 3 == 0:
                    e[:, :3] = e[:, :3] @ _rot([0, 0, 1], rng.uniform(120, 179))
                if name == "eggbox" and j == 1:
                    e[:, :3] = e[:, :3] @ _rot([1, 0, 0], 100.0)
                est[c][it].append(e)
                gt[c][it].append(g)
    return PoseEvaluator(classes, pts, diam), classes, est, gt


def _errors_by_pose_error_py(ev, cfg, classes, est, gt):
    """the per-pose numbers straight from lib/utils/pose_error.py with evaluation.py's eggbox rule applied here"""
    from lib.dataset.evaluation import RT_Z, SYM_CLASSES, se3_mul
    from lib.utils import pose_error as pe

    K = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float64)
    out = {k: [[[] for _ in est[c]] for c in range(len(classes))] for k in ("re", "te", "add", "arp_2d")}
    flipped = 0
    for c, name in enumerate(classes):
        P = ev._points[name]
        for it in range(len(est[c])):
            for e, g in zip(est[c][it], gt[c][it]):
                f = e
                if name == "eggbox" and pe.re(e[:, :3], g[:, :3]) > 90:
                    f = se3_mul(e, RT_Z)
                    flipped += 1
                out["re"][c][it].append(pe.re(f[:, :3], g[:, :3]))
                out["te"][c][it].append(pe.te(f[:, 3], g[:, 3]))
                fn = pe.adi if name in SYM_CLASSES else pe.add
                out["add"][c][it].append(fn(e[:, :3], e[:, 3], g[:, :3], g[:, 3], P))
                out["arp_2d"][c][it].append(pe.arp_2d(f[:, :3], f[:, 3], g[:, :3], g[:, 3], P, K))
    return out, flipped


def _same(a, b, path=""):
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "{}/{}".format(path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "{}[{}]".format(path, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, path
        assert np.array_equal(a, b), path
    else:
        assert a == b, (path, a, b)


def test_errors_option_reproduces_the_recomputation():
    from scene import make_test_config

    cfg = make_test_config(test_iter=2)
    ev, classes, est, gt = _seeded_lists()
    errors, flipped = _errors_by_pose_error_py(ev, cfg, classes, est, gt)
    assert flipped >= 8   # the eggbox rule is exercised
    for name, kw in (("evaluate_pose", {}), ("evaluate_pose_add", {"output_dir": None}), ("evaluate_pose_arp_2d", {"output_dir": None})):
        plain = getattr(ev, name)(cfg, est, gt, **kw)
        given = getattr(ev, name)(cfg, est, gt, errors=errors, **kw)
        _same(plain, given, name)
    # the lists are what is read: a changed one changes the table
    worse = {k: v for k, v in errors.items()}
    worse["add"] = [[[x + 1.0 for x in row] for row in c] for c in errors["add"]]
    assert ev.evaluate_pose_add(cfg, est, gt, errors=worse)["count_correct"]["0.10"].sum() == 0
    # and host_pose_errors (pred_eval's scorer of pairs that were not refined) gives the same four numbers
    for c, name in enumerate(classes):
        for j in (0, 1, 3):
            got = ev.host_pose_errors(cfg, name, est[c][0][j], gt[c][0][j])
            assert got == tuple(errors[k][c][0][j] for k in ("re", "te", "add", "arp_2d")), (name, j)
    short = {k: [[row[:-1] for row in c] for c in v] for k, v in errors.items()}
    with pytest.raises(ValueError, match="values for"):
        ev.evaluate_pose(cfg, est, gt, errors=short)


def test_device_table_flags_follow_the_class_names():
    """device_tables' flags are a pure function of the names (the upload itself needs a device: tests/test_gpu_pose_errors.py)"""
    from lib.dataset.evaluation import SYM_CLASSES
    from lib.hip import ops

    assert ops.POSE_ERR_ADI == 1 and ops.POSE_ERR_FLIP_Z180 == 2 and ops.STATUS_BAD_CLASS == 4
    assert ops.POSE_ERR_COLUMNS == ("re", "te", "add", "adi", "arp_2d")
    assert set(SYM_CLASSES) == {"eggbox", "glue", "bowl", "cup"}


def test_pose_errors_host_argument_checks(hip_lib):
    from conftest import ROOT

    header = open(os.path.join(ROOT, "include", "deepim_hip.h")).read()
    assert "#define DIM_POSE_ERR_ADI 1" in header and "#define DIM_POSE_ERR_FLIP_Z180 2" in header
    for T, B, n in ((1, 1, 1), (3, 7, 1025), (4, 16, 5841)):
        w = hip_lib.dim_pose_errors_workspace_bytes(T, B, n)
        assert w > 0 and w % 8 == 0, (T, B, n, w)
    assert hip_lib.dim_pose_errors_workspace_bytes(0, 4, 100) == 0 and hip_lib.dim_pose_errors_workspace_bytes(2, -1, 100) == 0
    # host-only: every call below is refused before a launch, so the pointers (host arrays) are never dereferenced on a device
    K = (ctypes.c_double * 9)(*np.eye(3).reshape(-1))
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    ERR_ARG = -1

    def call(poses32, poses64, T=1, B=1, n_classes=1, points=ptr, errors=ptr, workspace=ptr):
        return hip_lib.dim_pose_errors(points, ptr, ptr, n_classes, ptr, poses32, poses64, ptr, ctypes.cast(K, ctypes.c_void_p), T, B,
                                       workspace, errors, None, None)

    assert call(ptr, None, B=0) == ERR_ARG
    assert call(ptr, None, T=0) == ERR_ARG
    assert call(ptr, None, n_classes=0) == ERR_ARG
    assert call(ptr, ptr) == ERR_ARG and b"exactly one" in hip_lib.dim_last_error()
    assert call(None, None) == ERR_ARG and b"exactly one" in hip_lib.dim_last_error()
    assert call(ptr, None, points=None) == ERR_ARG
    assert call(None, ptr, errors=None) == ERR_ARG
    assert call(None, ptr, workspace=None) == ERR_ARG
