"""CPU: coarse pose from a detection box -- the viewpoint grid of deepim.core.coarse against the restatement tests/coarse_reference.py,
the TEST.COARSE_* keys and their checks, the convergence of the restated box fit on 1000 seeded cases, the restated top-k on hand-made
cases, the pipeline scene of tests/test_gpu_coarse.py through the CPU rasteriser, and the host side of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import coarse_reference as cr
from conftest import ROOT

NEW_SYMBOLS = ("dim_pose_from_box", "dim_pose_score_indexed", "dim_hyp_topk")
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------------------ grid, settings
@pytest.mark.parametrize("views,inplane", [(1, 1), (2, 3), (12, 4), (48, 12), (7, 1)])
def test_rotation_grid(views, inplane):
    from deepim.core.coarse import coarse_rotations

    R = coarse_rotations(views, inplane)
    M = views * inplane
    assert R.shape == (M, 3, 3) and R.dtype == np.float64
    np.testing.assert_allclose(R, cr.rotation_grid(views, inplane), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.tile(np.eye(3), (M, 1, 1)), atol=1e-12)   # orthonormal
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
    flat = R.reshape(M, 9)
    d = np.abs(flat[:, None, :] - flat[None, :, :]).max(axis=2) + np.eye(M)
    assert d.min() > 1e-3   # pairwise distinct
    # the indexing rule m = v * n_inplane + j: the turns of one view share its optical axis (the third row, -d_v), entry j is the
    # view's entry 0 turned by 2 pi j / n_inplane about the optical axis, and the axes are the Fibonacci directions
    for v in range(views):
        z = 1.0 - (2.0 * v + 1.0) / views
        np.testing.assert_allclose(R[v * inplane][2, 2], -z, atol=1e-12)
        for j in range(inplane):
            a = 2.0 * np.pi * j / inplane
            Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            np.testing.assert_allclose(R[v * inplane + j], Rz @ R[v * inplane], atol=1e-12)
            np.testing.assert_allclose(R[v * inplane + j][2], R[v * inplane][2], atol=1e-12)


def test_config_defaults():
    from deepim.config.config import config, reset_config
    from deepim.core.coarse import coarse_settings

    reset_config()
    assert config.TEST.COARSE_VIEWS == 0   # off
    assert coarse_settings(config) == (0, 1, 8, 1.0, "rgb", 0.02, 256)
    for k in ("COARSE_VIEWS", "COARSE_INPLANE", "COARSE_BOX_ITER", "COARSE_Z_INIT", "COARSE_SCORE", "COARSE_DEPTH_TAU", "COARSE_CHUNK"):
        del config.TEST[k]   # a config from before the keys: the same
    try:
        assert coarse_settings(config) == (0, 1, 8, 1.0, "rgb", 0.02, 256)
    finally:
        reset_config()


@pytest.mark.parametrize("key,value", [("COARSE_VIEWS", -1), ("COARSE_VIEWS", 2.5), ("COARSE_VIEWS", True), ("COARSE_INPLANE", 0),
                                       ("COARSE_INPLANE", 1.5), ("COARSE_BOX_ITER", 0), ("COARSE_BOX_ITER", 3.2),
                                       ("COARSE_Z_INIT", 0.0), ("COARSE_Z_INIT", float("inf")), ("COARSE_Z_INIT", float("nan")),
                                       ("COARSE_SCORE", "mask"), ("COARSE_SCORE", None), ("COARSE_DEPTH_TAU", 0.0),
                                       ("COARSE_DEPTH_TAU", float("nan")), ("COARSE_CHUNK", 0), ("COARSE_CHUNK", 7.5),
                                       ("COARSE_INPLANE", 70000)])
def test_config_validation(key, value):
    from deepim.config.config import config, reset_config
    from deepim.core.coarse import coarse_settings

    reset_config()
    config.TEST.COARSE_VIEWS = 2
    config.TEST[key] = value
    try:
        with pytest.raises(ValueError, match=key):
            coarse_settings(config)
    finally:
        reset_config()


def test_box_convention():
    import torch

    from deepim.core.coarse import boxes_from_int

    got = boxes_from_int(torch.tensor([[3, 9, 0, 4]], dtype=torch.int32))
    assert got.dtype == torch.float32 and got.tolist() == [[2.5, 9.5, -0.5, 4.5]]
    np.testing.assert_array_equal(cr.int_box(np.array([2.6, 9.4, -0.2, 4.5])), [2.5, 9.5, -0.5, 4.5])


# ------------------------------------------------------------------------------------------------------------------ the box fit
# The worst case of |t - t*| / t_z after 24 iterations over the committed cases (seed 20240), measured with this restatement:
# 7.9e-2 after 1 iteration, 2.0e-4 after 8, 2.0e-7 after 16, 1.97e-10 after 24.  The bar is 10 x the measured value.
WORST_24 = 1.97e-10
# float64 cannot tell two errors apart below this: u and v (up to 640 px) carry a few eps of relative rounding, i.e. some 1e-13 px,
# against boxes some tens of px across, which is 1e-14 in s and therefore in t_z; 64 eps = 1.4e-14
FLOOR = 64 * EPS


@pytest.fixture(scope="module")
def exact_errors():
    return cr.convergence_errors(lambda box: box, iters=(1, 8, 24))


def test_box_fit_converges_on_exact_boxes(exact_errors):
    """1000 seeded cases, the box the exact one of the true pose: the error falls from 1 to 8 to 24 iterations in every case, and the
    worst case after 24 is below 10 x its measured value.  'Falls' is asserted as written wherever float64 can tell: 11 of the 1000
    cases have reached the resolution of float64 after 8 iterations already (errors of 7e-17 .. 4e-16, against 7e-17 .. 9e-16 after
    24: rounding noise both times), and there the assertion is that the error stays below FLOOR."""
    e1, e8, e24 = exact_errors.T
    print("worst case after 1 / 8 / 24 iterations:", e1.max(), e8.max(), e24.max(), "; at the float64 floor after 8:", int((e8 <= FLOOR).sum()))
    assert np.all(e8 < e1)
    assert np.all((e24 < e8) | ((e8 <= FLOOR) & (e24 <= FLOOR)))
    assert np.all(e24[e8 > FLOOR] < e8[e8 > FLOOR]) and (e8 > FLOOR).sum() >= 900   # the floor rule covers a small minority
    assert e24.max() < 10 * WORST_24
    assert e24.max() > WORST_24 / 10   # the recorded value is the measured one


def test_box_fit_int_boxes_stop_at_the_quantisation_floor(exact_errors):
    """the boxes rounded outward to whole pixels: the worst error stops at the quantisation floor, 3.35e-2 after 8 and after 24
    iterations (8.1e-2 after 1).  It does not grow from 8 to 24 -- up to what the fit still moves after 8 iterations, which is the
    8-iteration error on exact boxes (2.0e-4): the fit converges to the fixed point of the rounded box, and its state after 8
    iterations is that close to it (measured: the worst case moves by +1.4e-11)."""
    q1, q8, q24 = cr.convergence_errors(cr.int_box, iters=(1, 8, 24)).T
    print("int boxes, worst case after 1 / 8 / 24 iterations:", q1.max(), q8.max(), q24.max())
    assert q24.max() <= q8.max() + exact_errors[:, 1].max()
    assert q8.max() < q1.max() and q24.max() > 100 * exact_errors[:, 2].max()   # a floor far above the exact boxes' error


def test_box_fit_failures():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.1, 0.1, size=(70, 3))
    R = cr.random_rotation(rng)
    K = cr.LINEMOD_K
    box = cr.exact_box(pts, R, np.array([0.05, -0.02, 0.8]), K)
    t, ok = cr.box_fit(pts, R, box, K, 8, 1.0)
    assert ok and np.linalg.norm(t - [0.05, -0.02, 0.8]) < 1e-3
    nan = float("nan")
    for bad in ([box[1], box[0], box[2], box[3]], [box[0], box[1], box[3], box[3]], [nan, box[1], box[2], box[3]],
                [box[0], float("inf"), box[2], box[3]]):
        t, ok = cr.box_fit(pts, R, bad, K, 8, 1.0)
        assert not ok and t.tolist() == [0.0, 0.0, 1.0]
    t, ok = cr.box_fit(pts[:0], R, box, K, 8, 1.0)      # a class without points
    assert not ok and t.tolist() == [0.0, 0.0, 1.0]
    t, ok = cr.box_fit(pts, R, box, K, 8, 0.05)         # z_init inside the object: a point behind the camera
    assert not ok and t.tolist() == [0.0, 0.0, 0.05]
    # the entry: class index out of range -> the fallback row with DIM_STATUS_BAD_CLASS, its neighbours untouched
    off = np.array([0, 70, 70])
    grid = cr.rotation_grid(2, 2).astype(np.float32).reshape(-1, 9)
    boxes = np.tile(box.astype(np.float32), (3, 1))
    pose, st = cr.pose_from_box(pts, off, [0, 5, 1], grid, boxes, K, 8, 1.0)
    assert st.reshape(3, 4).tolist() == [[0] * 4, [cr.STATUS_BAD_CLASS] * 4, [cr.STATUS_COARSE_BAD_BOX] * 4]
    alone, _ = cr.pose_from_box(pts, off, [0], grid, boxes[:1], K, 8, 1.0)
    np.testing.assert_array_equal(pose[:4], alone)
    np.testing.assert_array_equal(pose[4:, :, 3], np.tile([0.0, 0.0, 1.0], (8, 1)))
    np.testing.assert_array_equal(pose[4:8, :, :3], grid.reshape(4, 3, 3).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ the top-k
def test_topk_restatement():
    score, status, mask = cr.topk_cases()
    M, k = cr.TOPK_M, cr.TOPK_K
    idx, filler = cr.topk(score, M, k, status, mask)
    # pair 0: the rejected 0.9 and the infinity are skipped; the three 0.75 in the order of m; then 0.6
    assert idx[0].tolist() == [7, 19, 30, 20] and not filler[0].any()
    # pair 1: two candidates (0.5 is rejected), the other slots repeat slot 0
    assert idx[1].tolist() == [36, 0, 36, 36] and filler[1].tolist() == [False, False, True, True]
    # pair 2: none: candidate 0 everywhere
    assert idx[2].tolist() == [0, 0, 0, 0] and filler[2].all()
    # without the status the rejected candidates count
    idx2, _ = cr.topk(score, M, k)
    assert idx2[0].tolist() == [3, 7, 19, 30] and idx2[1].tolist() == [17, 36, 0, 17] and idx2[2].tolist() == [5, 5, 5, 5]
    # -0 and +0 tie: the smaller m first
    z = np.full((1, 6), -np.inf, np.float32)
    z[0, [4, 1]] = [0.0, -0.0]
    assert cr.topk(z.reshape(-1), 6, 2)[0].tolist() == [[1, 4]]
    # the gathered outputs
    poses = np.arange(3 * M * 12, dtype=np.float32).reshape(3 * M, 3, 4)
    i, s, p, st = cr.topk_outputs(score, M, k, poses, status, mask)
    assert s[0].tolist() == [0.75, 0.75, 0.75, pytest.approx(0.6)] and s[1].tolist() == [-0.25, -0.75, -0.25, -0.25]
    np.testing.assert_array_equal(p[1, 1], poses[M + 0])
    assert st[1].tolist() == [int(status[M + 36]), int(status[M]), int(status[M + 36]) | 64, int(status[M + 36]) | 64]
    assert st[2].tolist() == [int(status[2 * M]) | 64] * 4


# ------------------------------------------------------------------------------------------------------------------ the pipeline scene
@pytest.mark.parametrize("mode", ["rgb", "depth"])
def test_pipeline_scene_ranks_the_true_view_on_the_cpu(mode):
    """the scene of tests/test_gpu_coarse.py::test_pipeline through oracle's CPU rasteriser and the restatements: the true grid entry
    of both pairs scores first, by a wide margin (rgb: 0.916 against 0.158 and 0.665 against 0.100; depth: 1.000 against 0.552 and
    0.985 against 0.733), so the device's f32 rasteriser cannot turn the ranking"""
    from oracle import native

    native.build()
    score, boxes, pose = cr.pipeline_cpu(mode)
    M = score.shape[1]
    for p, m_true in enumerate(cr.PIPE_TRUE_M):
        order = np.argsort(-score[p], kind="stable")
        print(mode, "pair", p, "first", order[0], score[p, order[0]], "second", order[1], score[p, order[1]],
              "top-1 |t - t*| / t_z", np.linalg.norm(pose[p * M + m_true][:, 3] - cr.PIPE_T[p]) / cr.PIPE_T[p][2])
        assert order[0] == m_true
        assert score[p, order[0]] - score[p, order[1]] > 0.2
    assert cr.PIPE_TRUE_M[0] != cr.PIPE_TRUE_M[1]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_ctypes_and_library(hip_lib):
    from lib.hip import capi, ops

    header = open(os.path.join(ROOT, "include", "deepim_hip.h")).read()
    assert "#define DIM_STATUS_COARSE_BAD_BOX 512" in header
    assert ops.STATUS_COARSE_BAD_BOX == cr.STATUS_COARSE_BAD_BOX == 512 and ops.HYP_TOPK_MAX == 64
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in capi.SIGNATURES, name
        assert hasattr(hip_lib, name), name


def test_argument_checks_before_any_device_call(hip_lib):
    """every bad-argument case of the three entries returns DIM_ERR_ARG (-1) with a message on the host, before anything is launched"""
    f = ctypes.c_void_p(16)
    err = lambda: hip_lib.dim_last_error()  # noqa: E731

    def fit(points=f, table_off=f, n_classes=2, class_index=f, rot=f, boxes=f, K=f, kps=None, P=2, M=4, iters=8, z=1.0, out=f, out64=None,
            status=f):
        return hip_lib.dim_pose_from_box(points, table_off, n_classes, class_index, rot, boxes, K, kps, P, M, iters, z, out, out64, status, None)

    for kw in ({"P": 0}, {"P": 65536}, {"M": 0}, {"M": 65536}, {"iters": 0}, {"z": 0.0}, {"z": -1.0}, {"z": float("inf")},
               {"z": float("nan")}, {"points": None}, {"table_off": None}, {"class_index": None}, {"rot": None}, {"boxes": None},
               {"K": None}, {"out": None}, {"status": None}, {"n_classes": 0}):
        assert fit(**kw) == -1, kw
        assert b"pose_from_box" in err(), kw

    def score(obs=f, ren=f, dobs=None, dren=f, bbox=None, row=f, n_obs=2, B=6, H=48, W=64, mode=0, tau=0.02, work=f, out=f):
        return hip_lib.dim_pose_score_indexed(obs, ren, dobs, dren, bbox, row, n_obs, B, H, W, mode, tau, work, out, None, None)

    for kw in ({"row": None}, {"n_obs": 0}, {"B": 0}, {"H": 0}, {"mode": 2}, {"mode": 1}, {"mode": 1, "dobs": f, "tau": 0.0}, {"obs": None},
               {"ren": None}, {"dren": None}, {"work": None}, {"out": None}):
        assert score(**kw) == -1, kw
        assert b"pose_score_indexed" in err(), kw

    def topk(score=f, status=None, mask=0, P=3, M=37, k=4, poses=f, idx=f, sout=f, pout=f, stout=f):
        return hip_lib.dim_hyp_topk(score, status, mask, P, M, k, poses, idx, sout, pout, stout, None)

    for kw in ({"k": 0}, {"k": 38}, {"M": 100, "k": 65}, {"P": 0}, {"P": 65536}, {"M": 0}, {"M": 65536}, {"score": None}, {"poses": None},
               {"idx": None}, {"sout": None}, {"pout": None}, {"stout": None}):
        assert topk(**kw) == -1, kw
        assert b"hyp_topk" in err(), kw


def test_refiner_load_contract_without_a_device():
    """coarse off: det_boxes is refused before anything else is touched; the C loop object refuses the keys"""
    from deepim.core.tester import Refiner
    from lib.hip.refiner_capi import CRefiner
    from scene import make_test_config

    ref = Refiner.__new__(Refiner)
    ref.coarse = None
    with pytest.raises(ValueError, match="COARSE_VIEWS"):
        Refiner.load(ref, None, None, None, None, None, None, det_boxes=np.zeros((2, 4), np.float32))
    cfg = make_test_config()
    cfg.TEST.COARSE_VIEWS = 12
    try:
        with pytest.raises(ValueError, match="COARSE_VIEWS"):
            CRefiner(cfg, {}, None, 2)
    finally:
        cfg.TEST.COARSE_VIEWS = 0


# ------------------------------------------------------------------------------------------------------------------ pred_eval
class _FakeCoarseRefiner(object):
    """what pred_eval reads from a Refiner with a coarse stage and one hypothesis per pair, on CPU tensors"""

    def __init__(self, P, runs):
        self.P = self.B = P
        self.N = 1
        self.coarse = object()
        self._runs = runs
        self.loaded = []

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None, hyp_poses=None, det_boxes=None):
        assert image_rendered is None and mask_rendered is None and src_pose is None and hyp_poses is None
        self.loaded.append(det_boxes)
        self.coarse_out, self._poses = self._runs.pop(0)

    def refine(self):
        return self._poses


def test_pred_eval_reports_the_coarse_stage():
    import torch

    from deepim.core.tester import pred_eval
    from lib.dataset.evaluation import PoseEvaluator
    from lib.utils import synthetic as syn
    from scene import make_test_config

    cfg = make_test_config(test_iter=2)
    rng = np.random.default_rng(5)
    pts = {"ape": rng.uniform(-0.05, 0.05, size=(200, 3))}
    ev = PoseEvaluator(["ape"], pts, {"ape": 0.15})
    P, T, k = 3, 2, 1
    batches, runs, boxes = [], [], []
    for b in range(2):
        cls, gt, init = syn.sample_pairs(300 + b, P)
        co = {"pose": torch.from_numpy(init.reshape(P, k, 3, 4)), "idx": torch.full((P, k), 7 + b, dtype=torch.int32),
              "score": torch.full((P, k), 0.5), "status": torch.zeros((P, k), dtype=torch.int32)}
        runs.append((co, torch.from_numpy(np.stack([init, gt]))))   # the loop ends on the ground truth
        box = torch.full((P, 4), float(b))
        boxes.append(box)
        z = torch.zeros((P, 1, 4, 4))
        batches.append({"image_observed": z, "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt), "det_bbox": box})
    ref = _FakeCoarseRefiner(P, runs)
    out = pred_eval(cfg, ref, batches, ev)
    assert [bool(torch.equal(a, b)) for a, b in zip(ref.loaded, boxes)] == [True, True]   # the batch's own boxes, no src_pose needed
    co = out["coarse"]
    assert co["idx"] == [[7]] * P + [[8]] * P and co["status"] == [[0]] * (2 * P) and len(co["score"]) == 2 * P
    assert len(co["pose"]) == 2 * P and co["pose"][0].shape == (k, 3, 4)
    assert max(out["all_rot_err"][0][T - 1]) < 0.1 and min(out["all_rot_err"][0][0]) > 0.5   # degrees: the scored rows are the refined ones
