"""Coarse pose from a detection box on the device (csrc/coarse.hip, the indexed score of csrc/hyp.hip, deepim.core.coarse.CoarseInit,
Refiner.load(..., det_boxes=)): the box fit bit for bit against the float64 restatement tests/coarse_reference.py, the indexed score
against dim_pose_score on broadcast copies, the top-k against the restatement, the whole stage on a small two-class scene, and the
Refiner / pred_eval plumbing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import coarse_reference as cr  # noqa: E402
from scene import make_test_config  # noqa: E402

DEV = "cuda:0"
LDS_CAP = 2048   # kCoarseLdsPoints of csrc/coarse.hip: classes above it are rotated anew in every iteration


def ops():
    from lib.hip import ops as o

    return o


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------------------------ the box fit
def _tables(counts, seed, radius=None):
    """classes of the given point counts: anisotropic clouds about 0.2 m across (radius: per class half-width instead)"""
    rng = np.random.default_rng(seed)
    pts = []
    for c, n in enumerate(counts):
        r = 0.1 if radius is None else radius[c]
        pts.append(rng.uniform(-1, 1, size=(n, 3)) * rng.uniform(0.5, 1.0, size=3) * r)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return np.concatenate(pts).astype(np.float64), off


def _fit(points, off, cls, grid, boxes, K, iters, z_init, kps=None):
    P, M = len(cls), len(grid)
    out64 = torch.full((P * M, 3, 4), -7.0, dtype=torch.float64, device=DEV)
    status = torch.zeros((P * M,), dtype=torch.int32, device=DEV)
    pose, _ = ops().pose_from_box(d(points), d(off), d(np.asarray(cls, np.int32)), d(grid), d(boxes), K, iters, z_init,
                                  K_per_sample=None if kps is None else d(kps), pose_out_f64=out64, status=status)
    return pose.cpu().numpy(), out64.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("per_pair_K", [False, True])
@pytest.mark.parametrize("big", [LDS_CAP + 52, LDS_CAP])   # rotated anew per iteration / the largest class kept in LDS
def test_box_fit_parity(hip_lib, big, per_pair_K):
    """3 pairs over two classes (70 points: under one workgroup, no multiple of 64; `big` points: around the LDS cap), 5 rotations,
    boxes of nearby poses: pose_out_f64 is the restatement bit for bit, pose_out its float32 rounding"""
    points, off = _tables([70, big], seed=5)
    rng = np.random.default_rng(6)
    grid = np.stack([cr.random_rotation(rng) for _ in range(5)]).astype(np.float32).reshape(5, 9)
    cls = [0, 1, 0]
    K = cr.LINEMOD_K
    kps = None
    if per_pair_K:
        kps = np.stack([K * s for s in (1.0, 0.8, 1.1)])
        kps[:, 2, 2] = 1.0
        kps[2, 0, 1] = 0.7   # a skew: every entry of K is read
    boxes = []
    for p in range(3):
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.5, 1.2)])
        pts = points[off[cls[p]]:off[cls[p] + 1]]
        boxes.append(cr.exact_box(pts, cr.random_rotation(rng), t, K if kps is None else kps[p]))
    boxes = np.array(boxes, np.float32)
    for iters in (1, 3, 8):
        got32, got64, st = _fit(points, off, cls, grid, boxes, K, iters, 1.0, kps)
        want, want_st = cr.pose_from_box(points, off, cls, grid, boxes, K, iters, 1.0, K_per_sample=kps)
        assert not want_st.any() and not st.any()
        assert np.array_equal(bits(got64), bits(want)), (iters, np.abs(got64 - want).max())
        assert np.array_equal(bits(got32), bits(want.astype(np.float32))), iters
    assert np.abs(want[:, :, 3] - [0.0, 0.0, 1.0]).max() > 0.05   # the fit moved


def test_box_fit_bad_rows(hip_lib):
    """one bad pair of each kind among good ones: the stated bits, the fallback row [R_m | (0, 0, z_init)], and the good pairs' rows
    equal a run without the bad pairs bit for bit"""
    # classes: 70 points, above the cap, none, and a cloud 1 to 2 m across that z_init = 0.3 puts partly behind the camera
    points, off = _tables([70, LDS_CAP + 52, 0, 100], seed=8, radius=[0.1, 0.1, 0.1, 1.0])
    rng = np.random.default_rng(9)
    M, z_init = 5, 0.3
    grid = np.stack([cr.random_rotation(rng) for _ in range(M)]).astype(np.float32).reshape(M, 9)
    K = cr.LINEMOD_K
    good = np.array([250.5, 330.5, 180.5, 260.5], np.float32)
    nan = np.float32("nan")
    cls = [0, 1, 0, -1, 2, 3, 1, 7]
    boxes = np.array([good, [330.5, 250.5, 180.5, 260.5], [250.5, nan, 180.5, 260.5], good, good, good, good + 20, good], np.float32)
    BOX, CLS = cr.STATUS_COARSE_BAD_BOX, cr.STATUS_BAD_CLASS
    want_bits = [0, BOX, BOX, CLS, BOX, BOX, 0, CLS]
    got32, got64, st = _fit(points, off, cls, grid, boxes, K, 8, z_init)
    want, want_st = cr.pose_from_box(points, off, cls, grid, boxes, K, 8, z_init)
    assert st.reshape(-1, M).tolist() == [[b] * M for b in want_bits] == want_st.reshape(-1, M).tolist()
    assert np.array_equal(bits(got64), bits(want)) and np.array_equal(bits(got32), bits(want.astype(np.float32)))
    fall = np.concatenate([grid.reshape(M, 3, 3), np.tile(np.array([0.0, 0.0, z_init], np.float32).reshape(1, 3, 1), (M, 1, 1))], axis=2)
    for p, b in enumerate(want_bits):
        if b:
            assert np.array_equal(bits(got32[p * M:(p + 1) * M]), bits(fall)), p
    keep = [0, 6]
    alone32, alone64, alone_st = _fit(points, off, [cls[p] for p in keep], grid, boxes[keep], K, 8, z_init)
    assert not alone_st.any()
    for k, p in enumerate(keep):
        assert np.array_equal(bits(alone64[k * M:(k + 1) * M]), bits(got64[p * M:(p + 1) * M])), p
        assert np.abs(got64[p * M:(p + 1) * M, :, 3] - [0.0, 0.0, z_init]).max() > 0.05
    # status is OR-ed into: bits that were there stay
    status = torch.full((len(cls) * M,), 2, dtype=torch.int32, device=DEV)
    ops().pose_from_box(d(points), d(off), d(np.asarray(cls, np.int32)), d(grid), d(boxes), K, 8, z_init, status=status)
    assert status.cpu().numpy().reshape(-1, M).tolist() == [[b | 2] * M for b in want_bits]


# ------------------------------------------------------------------------------------------------------------------ the indexed score
@pytest.mark.parametrize("W", [32, 30])   # the float4 path and the scalar one
@pytest.mark.parametrize("mode", ["rgb", "depth"])
def test_indexed_score_equals_broadcast(hip_lib, mode, W):
    """6 samples over 2 observed rows on a 24 x W frame, each with a drawn rectangle of at least 64 pixels: bit-equal to dim_pose_score on
    per-sample copies of the rows; a row outside [0, 2) gives -inf and the status bit and leaves the others alone"""
    H, B, n_obs = 24, 6, 2
    rng = np.random.default_rng(15)
    obs = rng.normal(0, 20, (n_obs, 3, H, W)).astype(np.float32)
    dobs = rng.uniform(0.7, 0.9, (n_obs, 1, H, W)).astype(np.float32)
    ren = rng.normal(0, 20, (B, 3, H, W)).astype(np.float32)
    dren = np.zeros((B, 1, H, W), np.float32)
    bbox = np.zeros((B, 4), np.int32)
    for b in range(B):
        x0, y0 = 1 + b, 2 + b % 3
        dren[b, 0, y0:y0 + 9, x0:x0 + 11] = rng.uniform(0.78, 0.82, (9, 11))   # 99 pixels
        bbox[b] = [x0 - 1, x0 + 11, y0, y0 + 8]
    row = np.array([0, 1, 1, 0, 1, 0], np.int32)
    kw = dict(mode=mode, tau=0.05, bbox=d(bbox))
    st_i = torch.zeros((B,), dtype=torch.int32, device=DEV)
    got = ops().pose_score(d(obs), d(ren), d(dren), depth_observed=d(dobs) if mode == "depth" else None, obs_row=d(row), status=st_i, **kw)
    st_b = torch.zeros((B,), dtype=torch.int32, device=DEV)
    want = ops().pose_score(d(obs[row]), d(ren), d(dren), depth_observed=d(dobs[row]) if mode == "depth" else None, status=st_b, **kw)
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.all(np.isfinite(want)) and np.ptp(want) > 0.01, want
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert st_i.cpu().tolist() == st_b.cpu().tolist() == [0] * B
    swapped = ops().pose_score(d(obs), d(ren), d(dren), depth_observed=d(dobs) if mode == "depth" else None, obs_row=d(1 - row), **kw)
    assert not np.array_equal(bits(swapped.cpu().numpy()), bits(want))   # the index is read
    bad = row.copy()
    bad[2], bad[4] = 2, -1
    st = torch.zeros((B,), dtype=torch.int32, device=DEV)
    out = ops().pose_score(d(obs), d(ren), d(dren), depth_observed=d(dobs) if mode == "depth" else None, obs_row=d(bad), status=st, **kw)
    out = out.cpu().numpy()
    assert out[2] == -np.inf and out[4] == -np.inf
    assert st.cpu().tolist() == [0, 0, cr.STATUS_HYP_NO_SCORE, 0, cr.STATUS_HYP_NO_SCORE, 0]
    assert np.array_equal(bits(out[[0, 1, 3, 5]]), bits(want[[0, 1, 3, 5]]))


# ------------------------------------------------------------------------------------------------------------------ the top-k
def test_topk_matches_restatement(hip_lib):
    score, status, mask = cr.topk_cases()
    M, k = cr.TOPK_M, cr.TOPK_K
    poses = np.random.default_rng(2).normal(size=(3 * M, 3, 4)).astype(np.float32)
    for st_in in (status, None):
        want = cr.topk_outputs(score, M, k, poses, st_in, mask)
        runs = []
        for _ in range(2):
            got = ops().hyp_topk(d(score), M, k, d(poses), status_in=None if st_in is None else d(st_in), reject_mask=mask)
            runs.append([t.cpu().numpy() for t in got])
        idx, sc, ps, st = runs[0]
        assert idx.tolist() == want[0].tolist(), (idx, want[0])
        assert np.array_equal(bits(sc), bits(want[1])) and np.array_equal(bits(ps), bits(want[2]))   # NaN and -0 included
        assert st.tolist() == want[3].tolist()
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(bits(a), bits(b))   # a second call is bit-identical
    # k = 1 and k = M, M above one pass of the workgroup
    M2 = 300
    s2 = np.random.default_rng(4).permutation(2 * M2).astype(np.float32)
    p2 = np.zeros((2 * M2, 3, 4), np.float32)
    for k2 in (1, 64):
        idx = ops().hyp_topk(d(s2), M2, k2, d(p2))[0].cpu().numpy()
        assert idx.tolist() == cr.topk(s2, M2, k2)[0].tolist()


# ------------------------------------------------------------------------------------------------------------------ the pipeline
def _pipe_config(chunk, mode="rgb"):
    cfg = make_test_config(test_iter=1)
    cfg.dataset.INTRINSIC_MATRIX = cr.PIPE_K.copy()
    cfg.dataset.class_name = ["a", "b"]
    cfg.TEST.COARSE_VIEWS, cfg.TEST.COARSE_INPLANE = cr.PIPE_VIEWS, cr.PIPE_INPLANE
    cfg.TEST.COARSE_CHUNK, cfg.TEST.COARSE_SCORE = chunk, mode
    return cfg


@pytest.mark.parametrize("mode", ["rgb", "depth"])
def test_pipeline(hip_lib, mode):
    """2 pairs of two classes on a 240 x 320 frame, a 12 x 4 grid (M = 48): each observed frame is the render at [R_grid[m_p] | t_p], the
    box that of its drawn pixels.  The stage ranks m_p first in both pairs; chunks of 20 (which cross the pair boundary and leave a last
    chunk of 16) give the bits of one chunk of 96, and of the stages called one by one with the numpy top-k.
    The same scene through oracle's CPU rasteriser and the restatements (tests/test_coarse_host.py) ranks m_p first with margins of
    0.76 and 0.56 (rgb) and 0.45 and 0.25 (depth) between the first and the second score."""
    from deepim.core.coarse import CoarseInit, boxes_from_int
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    models, cls, pose_true = cr.pipeline_scene()
    H, W, P, k = cr.PIPE_H, cr.PIPE_W, 2, 3
    M = cr.PIPE_VIEWS * cr.PIPE_INPLANE
    try:
        cfg = _pipe_config(20, mode)
        rm = Render_Py(None, ["a", "b"], cr.PIPE_K, width=W, height=H, meshes=models)
        pm = syn.plane_means()
        img_o = torch.zeros((P, 3, H, W), device=DEV)
        dep_o = torch.zeros((P, 1, H, W), device=DEV)
        rm.render_batch(d(cls), d(pose_true), image=img_o, depth=dep_o, plane_means=pm, mask_thr=0.0)
        boxes = boxes_from_int(ops().mask_bbox(dep_o, 0.0))
        dep_wall = torch.where(dep_o > 0, dep_o, torch.full_like(dep_o, 1.5))
        small = CoarseInit(cfg, rm, None, P, k)
        assert [e - a for a, e in small.chunks()] == [20, 20, 20, 20, 16]
        got = [t.cpu().numpy().copy() for t in small.run(img_o, boxes, cls, depth_observed=dep_wall)]
        all_small = [t.cpu().numpy().copy() for t in (small.poses_all, small.score_all, small.status_all)]
        poses, idx, score, status = got
        assert idx[:, 0].tolist() == list(cr.PIPE_TRUE_M), (idx, score)
        assert not status.any() and np.all(np.isfinite(score)) and np.all(np.diff(score, axis=1) <= 0)
        t_err = [float(np.linalg.norm(poses[p, 0, :, 3] - cr.PIPE_T[p]) / cr.PIPE_T[p][2]) for p in range(P)]
        print(mode, "scores", score.tolist(), "top-1 |t - t*| / t_z", t_err)
        # (no bar on the error: the parity below is the assertion; the restatement's own figures for these boxes are in DESIGN.md)
        # one chunk of 96
        one = CoarseInit(_pipe_config(96, mode), rm, None, P, k)
        assert one.chunks() == [(0, 96)]
        for a, b in zip(got, one.run(img_o, boxes, cls, depth_observed=dep_wall)):
            assert np.array_equal(bits(a), bits(b.cpu().numpy()))
        for a, b in zip(all_small, (one.poses_all, one.score_all, one.status_all)):
            assert np.array_equal(bits(a), bits(b.cpu().numpy()))
        # the stages one by one: the fit against the restatement, one render, the indexed score, the numpy top-k
        pts, off = one.points.cpu().numpy(), one.table_off.cpu().numpy()
        want_pose, want_st = cr.pose_from_box(pts, off, cls, one.rot_table.cpu().numpy(), boxes.cpu().numpy(), cr.PIPE_K, 8, 1.0)
        assert np.array_equal(bits(all_small[0]), bits(want_pose.astype(np.float32))) and not want_st.any()
        cand = d(want_pose.astype(np.float32))
        img = torch.zeros((P * M, 3, H, W), device=DEV)
        dep = torch.zeros((P * M, 1, H, W), device=DEV)
        bb = torch.zeros((P * M, 4), dtype=torch.int32, device=DEV)
        rm.render_batch(d(np.repeat(cls, M)), cand, image=img, depth=dep, bbox=bb, plane_means=pm, mask_thr=0.0)
        sc = ops().pose_score(img_o, img, dep, mode, cfg.TEST.COARSE_DEPTH_TAU, depth_observed=dep_wall if mode == "depth" else None, bbox=bb,
                              obs_row=d(np.repeat(np.arange(P, dtype=np.int32), M)))
        assert np.array_equal(bits(sc.cpu().numpy()), bits(all_small[1]))
        want = cr.topk_outputs(sc.cpu().numpy(), M, k, want_pose.astype(np.float32), np.zeros(P * M, np.int32), small.reject_mask)
        assert idx.tolist() == want[0].tolist()
        assert np.array_equal(bits(score), bits(want[1])) and np.array_equal(bits(poses), bits(want[2])) and status.tolist() == want[3].tolist()
    finally:
        make_test_config()


# ------------------------------------------------------------------------------------------------------------------ the Refiner
@pytest.mark.parametrize("n_hyp", [2, 1])
def test_refiner_starts_from_boxes(hip_lib, n_hyp):
    """2 pairs, HYP_NUM = 2 and 1, untrained weights, a 6 x 2 grid in chunks of 5: load(..., det_boxes=) leaves the coarse stage's
    top poses in pose_init and their renders in the initial planes; refine() and pred_eval run; the argument contract of load()"""
    from deepim.core.coarse import CoarseInit, boxes_from_int
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs

    P = 2
    cfg = make_test_config(test_iter=2)
    try:
        cfg.TEST.HYP_NUM = n_hyp
        cfg.TEST.COARSE_VIEWS, cfg.TEST.COARSE_INPLANE, cfg.TEST.COARSE_CHUNK = 6, 2, 5
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = sym.init_weights(cfg, {}, {}, seed=0)
        data = SyntheticPairs(cfg, 2 * P, P, subdiv=3)
        rm = data.render_machine
        pred = Predictor(cfg, params, P * n_hyp)
        ref = Refiner(cfg, pred, rm, P, evaluator=data.evaluator())
        batches = list(data.test_batches())
        bl = batches[0]
        det = boxes_from_int(ops().mask_bbox(bl["mask_observed"], 0.5))
        ref.load(bl["image_observed"], None, None, None, None, bl["class_index"], det_boxes=det)
        want = CoarseInit(cfg, rm, data.evaluator(), P, n_hyp).run(bl["image_observed"], det, bl["class_index"])
        for key, w in zip(("pose", "idx", "score", "status"), want):
            assert np.array_equal(bits(ref.coarse_out[key].cpu().numpy()), bits(w.cpu().numpy())), key
        assert np.all(np.isfinite(want[2].cpu().numpy()))
        start = ref.pose_init.cpu().numpy()
        assert np.array_equal(bits(start), bits(want[0].cpu().numpy().reshape(P * n_hyp, 3, 4)))
        # the initial planes: a direct render at those poses
        B, H, W = P * n_hyp, 480, 640
        img = torch.zeros((B, 3, H, W), device=DEV)
        mask = torch.zeros((B, 1, H, W), device=DEV)
        bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        rm.render_batch(ref.batch["class_index"], ref.pose_init, image=img, mask=mask, bbox=bbox, plane_means=ref.net.plane_means, mask_thr=0.2)
        assert torch.equal(ref.init["image_rendered"], img) and torch.equal(ref.init["mask_rendered"], mask)
        assert float(mask.sum()) > 0
        assert torch.equal(ref.init["mask_observed"], ops().box_mask(bbox, torch.zeros_like(mask)))
        assert ref.batch["class_index"].cpu().tolist() == np.repeat(bl["class_index"].cpu().numpy(), n_hyp).tolist()
        out = ref.refine()
        assert tuple(out.shape) == (2, P, 3, 4) and bool(torch.isfinite(out).all())
        # the argument contract
        with pytest.raises(ValueError, match="det_boxes"):
            ref.load(bl["image_observed"], bl["image_rendered"], bl["mask_observed"], bl["mask_rendered"], bl["src_pose"], bl["class_index"])
        with pytest.raises(ValueError, match="det_boxes"):
            ref.load(bl["image_observed"], None, None, None, None, bl["class_index"], det_boxes=det[:1])
        # pred_eval: the boxes of mask_observed, out["coarse"]
        res = pred_eval(cfg, ref, batches, data.evaluator())
        co = res["coarse"]
        assert len(co["idx"]) == len(co["score"]) == len(co["status"]) == len(co["pose"]) == 2 * P
        assert all(len(i) == n_hyp for i in co["idx"]) and all(np.asarray(p).shape == (n_hyp, 3, 4) for p in co["pose"])
        assert co["idx"][:P] == want[1].cpu().tolist()
        assert len(res["all_rot_err"][0][-1]) == 2 * P
        # coarse off: det_boxes is refused
        cfg.TEST.COARSE_VIEWS = 0
        off = Refiner(cfg, pred, rm, P)
        assert off.coarse is None
        with pytest.raises(ValueError, match="COARSE_VIEWS"):
            off.load(bl["image_observed"], bl["image_rendered"], bl["mask_observed"], bl["mask_rendered"], bl["src_pose"], bl["class_index"],
                     det_boxes=det)
    finally:
        make_test_config()


def test_lit_renderer_is_refused(hip_lib):
    from deepim.core.coarse import CoarseInit

    class Lit(object):
        normals = None

    cfg = make_test_config()
    cfg.TEST.COARSE_VIEWS = 4
    try:
        with pytest.raises(ValueError, match="lit"):
            CoarseInit(cfg, Lit(), None, 2, 1)
    finally:
        make_test_config()
