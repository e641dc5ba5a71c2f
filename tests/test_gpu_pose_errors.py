"""Pose errors on the device (csrc/metrics.hip, ops.pose_errors, pred_eval with TEST.DEVICE_EVAL) against lib/utils/pose_error.py.

The bar of every comparison: |dev - ref| <= 1e-10 * max(1, |ref|) in the column's unit (deg, m, m, m, px).  Float64 rounding over
500-term sums is ~1e-13; the same computation restated in float32 misses the golden file by 5e-10 .. 4e-8 m on every pair, so the bar
separates the two.  The rotation errors compared are 0.5 .. 175 deg, where arccos is conditioned to <= 12 ulp."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_test_config  # noqa: E402

DEV = "cuda:0"
COLS = ("re", "te", "add", "adi", "arp_2d")
K_LM = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float64)
ADI, FLIP, BAD_CLASS = 1, 2, 4


def ops():
    from lib.hip import ops as o

    return o


def _within_bar(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    diff = np.abs(dev - ref)
    bar = 1e-10 * np.maximum(1.0, np.abs(ref))
    print("{}: max |dev - ref| = {:.3e} (bar 1e-10 * max(1, |ref|), largest ratio {:.3e})".format(what, diff.max(), (diff / bar).max()))
    assert np.all(diff <= bar), (what, float(diff.max()), int(np.argmax(diff / bar)))


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _gt_pose(rng):
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
    return np.concatenate([_rot(rng.normal(size=3), rng.uniform(0, 180)), t[:, None]], axis=1)


def _tables(sizes, flags, seed=3):
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(-0.05, 0.05, size=(n, 3)) * np.array([1.0, 0.7, 0.4]) for n in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    allp = np.concatenate(pts) if sum(sizes) else np.zeros((0, 3))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return pts, (d(allp), d(off), d(np.asarray(flags, np.int32)))


def _host_rows(pts, flags, cls, est, gt, K):
    """(T,B,5) by lib/utils/pose_error.py, the flip rule as lib/dataset/evaluation.py applies it"""
    from lib.dataset.evaluation import RT_Z, se3_mul
    from lib.utils import pose_error as pe

    est = np.asarray(est, np.float64)
    est = est[None] if est.ndim == 3 else est
    out = np.full(est.shape[:2] + (5,), np.nan)
    for t in range(est.shape[0]):
        for b in range(est.shape[1]):
            e, g, P = est[t, b], gt[b], pts[cls[b]]
            f = se3_mul(e, RT_Z) if (flags[cls[b]] & FLIP) and pe.re(e[:, :3], g[:, :3]) > 90 else e
            out[t, b, 0] = pe.re(f[:, :3], g[:, :3])
            out[t, b, 1] = pe.te(f[:, 3], g[:, 3])
            out[t, b, 2] = pe.add(e[:, :3], e[:, 3], g[:, :3], g[:, 3], P)
            if flags[cls[b]] & ADI:
                out[t, b, 3] = pe.adi(e[:, :3], e[:, 3], g[:, :3], g[:, 3], P)
            out[t, b, 4] = pe.arp_2d(f[:, :3], f[:, 3], g[:, :3], g[:, 3], P, K)
    return out


def _run(tables, cls, est, gt, K=K_LM, **kw):
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    est = torch.from_numpy(np.ascontiguousarray(est)).to(DEV)
    return ops().pose_errors(tables[0], tables[1], tables[2], d(np.asarray(cls), torch.int32), est, d(gt, torch.float64), K, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_golden_file_all_five_columns(hip_lib):
    g = np.load(os.path.join(GOLDEN, "pose_error_golden.npz"))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    tables = (d(g["pts"]), d(np.array([0, 500], np.int32)), d(np.array([ADI], np.int32)))
    assert g["pose_est"].dtype == np.float64 and g["pts"].shape == (500, 3)
    err = _run(tables, np.zeros(16, np.int32), g["pose_est"], g["pose_gt"], K=g["K"]).cpu().numpy()
    assert err.shape == (16, 5) and err.dtype == np.float64
    for k, name in enumerate(COLS):
        _within_bar(err[:, k], g[name], "golden " + name)


# ------------------------------------------------------------------------------------------------------------------ 2. tiling
# query tile 512 (two points per lane), candidate tile 256, 16 workgroups per pose
SIZES = (1, 255, 256, 257, 1025, 511, 512, 513)
FLAGS = (ADI, 0, ADI, ADI, ADI, 0, ADI, ADI)


def _est_f32(rng, gt, T):
    """(T,B,3,4) float32: the ground truth turned by 0.5 .. 175 deg and moved by up to ~3 cm, rounded to float32"""
    B = gt.shape[0]
    est = np.zeros((T, B, 3, 4))
    for t in range(T):
        for b in range(B):
            est[t, b, :, :3] = _rot(rng.normal(size=3), rng.uniform(0.5, 175.0)) @ gt[b][:, :3]
            est[t, b, :, 3] = gt[b][:, 3] + rng.normal(size=3) * 0.015
    return est.astype(np.float32)


@pytest.mark.parametrize("draw", [(4, 0, 2, 3, 1, 7, 5), (6, 4, 3, 0, 5, 2, 7)])
def test_sizes_around_the_tiles_mixed_classes_float32_poses(hip_lib, draw):
    pts, tables = _tables(SIZES, FLAGS)
    rng = np.random.default_rng(17 + draw[0])
    gt = np.stack([_gt_pose(rng) for _ in draw])
    est = _est_f32(rng, gt, T=3)
    want = _host_rows(pts, FLAGS, draw, est, gt, K_LM)
    assert 0.5 <= want[..., 0].min() and want[..., 0].max() <= 175.0 + 1e-3 and want[..., 0].max() > 90.0
    status = torch.zeros((7,), dtype=torch.int32, device=DEV)
    err = _run(tables, draw, est, gt, status=status).cpu().numpy()
    assert err.shape == (3, 7, 5) and status.cpu().tolist() == [0] * 7
    no_adi = np.array([not (FLAGS[c] & ADI) for c in draw])
    assert no_adi.any() and not no_adi.all()
    assert np.array_equal(np.isnan(err[..., 3]), np.broadcast_to(no_adi, (3, 7)))   # adi is NaN exactly where the flag is off
    assert not np.isnan(err[..., [0, 1, 2, 4]]).any()
    for k, name in enumerate(COLS):
        keep = ~np.isnan(want[..., k])
        _within_bar(err[..., k][keep], want[..., k][keep], "tiles {} {}".format(draw[0], name))


def test_class_larger_than_one_pass_of_the_grid(hip_lib):
    """16 workgroups x 512 query points cover 8192 points in one pass; 8705 points send workgroup 0 round its loop a second time, with
    one query point in the last tile (the only size in this file past 1k points: no smaller one reaches that path)"""
    pts, tables = _tables((8705, 300), (ADI, 0), seed=5)
    rng = np.random.default_rng(23)
    cls = (0, 1, 0)
    gt = np.stack([_gt_pose(rng) for _ in cls])
    est = _est_f32(rng, gt, T=1)[0]
    err = _run(tables, cls, est, gt).cpu().numpy()
    want = _host_rows(pts, (ADI, 0), cls, est, gt, K_LM)[0]
    assert err.shape == (3, 5)
    for k, name in enumerate(COLS):
        keep = ~np.isnan(want[:, k])
        _within_bar(err[:, k][keep], want[:, k][keep], "two passes " + name)
    assert np.isnan(err[1, 3]) and not np.isnan(err[[0, 2], 3]).any()


# ------------------------------------------------------------------------------------------------------------------ 3. eggbox
def test_flip_rule_on_both_sides_of_90_degrees(hip_lib):
    from lib.dataset.evaluation import PoseEvaluator

    pts, tables = _tables((300,), (ADI | FLIP,), seed=7)
    _, plain = _tables((300,), (ADI,), seed=7)
    rng = np.random.default_rng(29)
    angles = (89.9, 90.1, 170.0)
    gt = np.stack([_gt_pose(rng) for _ in angles])
    est = gt.copy()
    for b, a in enumerate(angles):
        est[b, :, :3] = gt[b][:, :3] @ _rot([0, 0, 1], a)   # about the object's z
        est[b, :, 3] += [0.004, -0.003, 0.01]
    # evaluation.py's own rule, through the evaluator's scorer of single poses (class named eggbox) and with the config's camera
    cfg = make_test_config(test_iter=1)
    K = np.asarray(cfg.dataset.INTRINSIC_MATRIX, dtype=np.float64)
    err = _run(tables, (0, 0, 0), est, gt, K=K).cpu().numpy()
    raw = _run(plain, (0, 0, 0), est, gt, K=K).cpu().numpy()
    ev = PoseEvaluator(["eggbox"], {"eggbox": pts[0]}, {"eggbox": 0.1})
    want = np.array([ev.host_pose_errors(cfg, "eggbox", est[b], gt[b]) for b in range(3)])   # re, te, adi, arp_2d
    for k, col in enumerate((0, 1, 3, 4)):
        _within_bar(err[:, col], want[:, k], "eggbox " + COLS[col])
    np.testing.assert_allclose(err[:, 0], [89.9, 89.9, 10.0], rtol=0, atol=1e-6)     # below 90: as is; above: 180 - angle
    np.testing.assert_allclose(raw[:, 0], angles, rtol=0, atol=1e-6)
    # add and adi never see the flip: bit for bit the unflagged class's; arp_2d changes only past 90 degrees
    assert np.array_equal(err[:, 2:4].view(np.uint64), raw[:, 2:4].view(np.uint64))
    assert err[0, 4] == raw[0, 4] and err[1, 4] != raw[1, 4] and err[2, 4] < raw[2, 4] - 1.0
    assert np.array_equal(err[:, 1], raw[:, 1])   # est . RT_Z keeps the translation


# ------------------------------------------------------------------------------------------------------------------ 4. degenerate
def test_equal_poses_bad_classes_and_an_empty_class(hip_lib):
    sizes, flags = (257, 0, 130), (ADI, ADI, 0)
    pts, tables = _tables(sizes, flags, seed=11)
    rng = np.random.default_rng(31)
    cls = np.array([0, -1, 2, 3, 0, 1, 2], np.int32)      # -1 and n_classes = 3: bad; class 1: no points
    gt = np.stack([_gt_pose(rng) for _ in cls])
    est = gt.copy()
    est[4:, :, 3] += 0.01                                  # rows 0..3 have est == gt, rows 4.. a 1 cm offset
    status = torch.zeros((7,), dtype=torch.int32, device=DEV)
    status[4] = 8                                          # bits of other stages stay
    err = _run(tables, cls, est, gt, status=status).cpu().numpy()
    assert status.cpu().tolist() == [0, BAD_CLASS, 0, BAD_CLASS, 8, 0, 0]
    assert np.isnan(err[[1, 3, 5]]).all()                  # bad, bad, empty
    for b in (0, 2):                                       # est == gt
        assert err[b, 1] == 0.0 and err[b, 2] == 0.0 and err[b, 4] == 0.0, err[b]
        assert 0.0 <= err[b, 0] <= 1e-5, err[b, 0]         # arccos near 1 is conditioned to sqrt(2 eps) only
    assert err[0, 3] == 0.0 and np.isnan(err[2, 3])
    # the neighbours of the bad rows: what the same pairs give in a batch without them, bit for bit, and the host's numbers
    ok = [0, 2, 4, 6]
    alone = _run(tables, cls[ok], est[ok], gt[ok]).cpu().numpy()
    assert np.array_equal(err[ok].view(np.uint64), alone.view(np.uint64))
    want = _host_rows(pts, flags, cls[[4, 6]], est[[4, 6]], gt[[4, 6]], K_LM)[0]
    for k, name in enumerate(COLS):
        keep = ~np.isnan(want[:, k])
        _within_bar(err[[4, 6], k][keep], want[:, k][keep], "neighbours " + name)
    # status is optional
    assert np.array_equal(_run(tables, cls, est, gt).cpu().numpy().view(np.uint64), err.view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ 5. determinism
def test_second_call_with_a_dirty_workspace_is_bit_identical(hip_lib):
    pts, tables = _tables(SIZES, FLAGS)
    rng = np.random.default_rng(37)
    draw = (4, 0, 2, 3, 1, 7, 6)
    gt = np.stack([_gt_pose(rng) for _ in draw])
    est = _est_f32(rng, gt, T=3)
    # exactly dim_pose_errors_workspace_bytes between guards, at the documented minimum alignment (8 mod 16), full of NaN bits
    arena = guard_arena.workspace(ops().lib().dim_pose_errors_workspace_bytes(3, 7, max(SIZES)), 8, DEV)
    work = arena.view()
    a = _run(tables, draw, est, gt, workspace=work).cpu().numpy().copy()
    arena.check("dim_pose_errors workspace, NaN before the call")
    work.copy_(torch.randn(work.shape, dtype=torch.float64, device=DEV) * 1e6)
    b = _run(tables, draw, est, gt, workspace=work).cpu().numpy()
    arena.check("dim_pose_errors workspace, noise before the call")
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    c = _run(tables, draw, est.astype(np.float64), gt).cpu().numpy()   # the float64 entry on the same (float32-valued) poses
    assert np.array_equal(a.view(np.uint64), c.view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ 6. pred_eval
PAIRS, BATCH = 8, 4


def _thresholds_clear(out, diam, classes, lists, eps=1e-9):
    """no host error within eps of a threshold it is compared with: a count that differs cannot be blamed on rounding"""
    rot, trans = np.arange(1, 11, 1).astype(np.float64), np.arange(0.01, 0.11, 0.01)
    for c in range(len(classes)):
        for it in range(len(lists[0][c])):
            for v, thr in ((lists[0][c][it], rot), (lists[1][c][it], trans)):
                if len(v):
                    assert np.abs(np.asarray(v, np.float64)[:, None] - thr[None, :]).min() > eps
    for (name, it), err in out["add"]["errors"].items():
        scale = diam[name]
        thr = np.concatenate([(np.arange(0, 0.1, 0.0001).astype(np.float32) * np.float32(scale)).astype(np.float32).astype(np.float64),
                              [float(np.float32(f * scale)) for f in (0.02, 0.05, 0.10)]])
        assert np.abs(err[:, None] - thr[None, :]).min() > eps, (name, it)
    for (name, it), err in out["arp_2d"]["errors"].items():
        thr = np.concatenate([np.arange(0, 50, 0.1).astype(np.float32).astype(np.float64), [2.0, 5.0, 10.0, 20.0]])
        assert np.abs(err[:, None] - thr[None, :]).min() > eps, (name, it)


def _compare_tables(off, on, what):
    for key in ("add", "arp_2d"):
        a, b = off[key], on[key]
        assert np.array_equal(a["count_all"], b["count_all"]), (what, key)
        assert set(a["count_correct"]) == set(b["count_correct"])
        for k in a["count_correct"]:
            assert np.array_equal(a["count_correct"][k], b["count_correct"][k]), (what, key, k)
        assert set(a["errors"]) == set(b["errors"]) and len(a["errors"]) > 0
        for k in a["errors"]:
            _within_bar(b["errors"][k], a["errors"][k], "{} {} {}".format(what, key, k))
        assert a["overall"] == b["overall"] and a["per_class"] == b["per_class"]
    for k in ("rot_acc", "trans_acc", "space_acc"):
        assert np.array_equal(off["pose"][k], on["pose"][k]), (what, k)
    assert off["pose"]["overall"] == on["pose"]["overall"] and off["pose"]["num_valid_class"] == on["pose"]["num_valid_class"]


@pytest.mark.parametrize("variant", ["plain", "icp", "hyp"])
def test_pred_eval_device_errors_equal_the_host_tables(hip_lib, variant):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "glue"]   # glue: ADD-S
    n_hyp = 2 if variant == "hyp" else 1
    cfg.TEST.ICP_ITER = 2 if variant == "icp" else 0
    cfg.TEST.HYP_NUM = n_hyp
    try:
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
        data = SyntheticPairs(cfg, PAIRS, BATCH, seed=2333, subdiv=3)
        ev = data.evaluator()
        assert all(len(p) <= 1100 for p in ev._points.values())
        flags = ev.device_tables(DEV)[2].cpu().tolist()
        assert flags == [0, ADI] and ev.device_tables(DEV)[0] is ev.device_tables(DEV)[0]
        ref = Refiner(cfg, Predictor(cfg, params, BATCH * n_hyp), data.render_machine, BATCH)
        batches = list(data.test_batches())
        assert len(batches) == PAIRS // BATCH
        assert {int(c) for b in batches for c in b["class_index"].cpu().tolist()} == {0, 1}   # both classes are scored
        cfg.TEST.DEVICE_EVAL = False
        off = pred_eval(cfg, ref, batches, ev)
        cfg.TEST.DEVICE_EVAL = True
        on = pred_eval(cfg, ref, batches, ev)
        assert "device_eval" not in off and on["device_eval"] is True
        # the loop is deterministic: both runs scored the same poses (these lists are host numbers in both)
        assert off["all_rot_err"] == on["all_rot_err"] and off["all_trans_err"] == on["all_trans_err"]
        _thresholds_clear(off, ev._diameters, ev.classes, (off["all_rot_err"], off["all_trans_err"]))
        _compare_tables(off, on, variant)
        if variant == "icp":
            assert off["icp"]["all_rot_err"] == on["icp"]["all_rot_err"]
            _thresholds_clear(off["icp"], ev._diameters, ev.classes, (off["icp"]["all_rot_err"], off["icp"]["all_trans_err"]))
            _compare_tables(off["icp"], on["icp"], "icp row")
        if variant == "hyp":
            assert on["hyp"]["choice"] == off["hyp"]["choice"] and on["hyp"]["num"] == 2
    finally:
        cfg.TEST.ICP_ITER = 0
        cfg.TEST.HYP_NUM = 1
        cfg.TEST.DEVICE_EVAL = False
