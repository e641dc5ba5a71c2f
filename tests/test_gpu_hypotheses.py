"""Several hypotheses per pair on the device (csrc/hyp.hip; deepim.core.tester.Refiner with TEST.HYP_NUM > 1): the four kernels
against the float64 restatement tests/hyp_reference.py on GPU-rendered planes, the selection of the true pose through the captured
Refiner, hypothesis 0 against the plain loop, graph replay, load_staged, and pred_eval's out["hyp"]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import hyp_reference as hr  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640


def ops():
    from lib.hip import ops as o

    return o


@pytest.fixture(scope="module")
def rscene(hip_lib):
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    models = syn.make_models(seed=2333, n_models=1, subdiv=3)
    rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
    return models, rm


PLANE_MEANS = np.array([103.939, 116.779, 123.68], np.float32)


def _render(rm, poses, K=None):
    """-> image (B,3,H,W) (plane means subtracted), depth (B,1,H,W), bbox (B,4) of every drawn pixel"""
    B = poses.shape[0]
    img = torch.zeros((B, 3, H, W), device=DEV)
    depth = torch.zeros((B, 1, H, W), device=DEV)
    bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    rm.render_batch(torch.zeros((B,), dtype=torch.int32, device=DEV), torch.as_tensor(poses, dtype=torch.float32).to(DEV).contiguous(),
                    K=K, image=img, depth=depth, bbox=bbox, plane_means=PLANE_MEANS, mask_thr=0.0)
    return img, depth, bbox


def _rot(axis, deg):
    return hr.rodrigues(axis, np.radians(deg))


# ------------------------------------------------------------------------------------------------------------------ the kernels
def test_expand_matches_restatement(hip_lib):
    from deepim.core.tester import hypothesis_rotations
    from lib.utils import synthetic as syn

    P, N = 3, 4
    _, gt, _ = syn.sample_pairs(11, P)
    table = hypothesis_rotations(N, 37.0)
    tab = torch.from_numpy(table.astype(np.float32).reshape(N, 9)).to(DEV)
    out = ops().hyp_expand(tab, torch.from_numpy(gt).to(DEV), N).cpu().numpy()
    want = hr.expand(table.astype(np.float32).astype(np.float64), gt)
    for p in range(P):
        assert np.array_equal(out[p * N].view(np.uint32), gt[p].view(np.uint32))   # hypothesis 0: bit for bit
        for h in range(1, N):
            np.testing.assert_allclose(out[p * N + h], want[p * N + h], rtol=0, atol=1e-6)


def test_broadcast_rows(hip_lib):
    P, N = 3, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    planes = torch.randn((P, 3, H, W), device=DEV, generator=g)
    dst = torch.zeros((P * N, 3, H, W), device=DEV)
    ops().hyp_broadcast(dst, planes, N)
    assert torch.equal(dst, planes.repeat_interleave(N, 0))
    K = torch.randn((P, 9), device=DEV, generator=g)   # 9 words a row: the scalar path
    dK = torch.zeros((P * N, 9), device=DEV)
    ops().hyp_broadcast(dK, K, N)
    assert torch.equal(dK, K.repeat_interleave(N, 0))
    ci = torch.tensor([5, -1, 7], dtype=torch.int32, device=DEV)
    dci = torch.zeros((P * N,), dtype=torch.int32, device=DEV)
    ops().hyp_broadcast(dci, ci, N)
    assert dci.cpu().tolist() == [5] * 4 + [-1] * 4 + [7] * 4


@pytest.fixture(scope="module")
def score_planes(rscene):
    """8 samples: an object rendered at 8 poses, observed at nearby ones (colour texture + noise, depth)"""
    from lib.utils import synthetic as syn

    models, rm = rscene
    cls, gt, init = syn.sample_pairs(21, 8)
    img_r, dep_r, bbox = _render(rm, init)
    img_o, dep_o, _ = _render(rm, gt)
    dep_o = torch.where(dep_o > 0, dep_o, torch.full_like(dep_o, 1.5))   # in front of a wall: every pixel of S has a reading
    g = torch.Generator(device=DEV).manual_seed(9)
    img_o = img_o + 4.0 * torch.randn(img_o.shape, device=DEV, generator=g)
    return img_r, dep_r, bbox, img_o, dep_o


def _hostile(score_planes):
    img_r, dep_r, bbox, img_o, dep_o = [t.clone() for t in score_planes]
    bb = bbox.cpu().numpy()
    bbox[1] = torch.tensor([bb[1][0] - 700, bb[1][1], bb[1][2] - 500, bb[1][3] + 900], dtype=torch.int32)   # partly outside the frame
    bbox[2] = torch.tensor([W, -1, H, -1], dtype=torch.int32)                                              # empty
    img_r[3] = 7.25                                                                                          # constant render
    img_o[4] = 400.0 + 0.01 * torch.randn((3, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))   # 400 + texture
    dep_o[5] = 0.0                                                                                           # no depth reading
    dep_o[6] = float("nan")
    img_o[7] = -3.5                                                                                          # constant observation
    return img_r, dep_r, bbox, img_o, dep_o


@pytest.mark.parametrize("mode", ["rgb", "depth"])
def test_pose_score_matches_restatement(score_planes, mode):
    img_r, dep_r, bbox, img_o, dep_o = _hostile(score_planes)
    B = img_r.shape[0]
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    # the workspace: exactly dim_pose_score_workspace_bytes between guards, at the documented minimum alignment (8 mod 16), NaN bits
    work = guard_arena.workspace(ops().lib().dim_pose_score_workspace_bytes(B, H, W), 8, DEV)
    s = ops().pose_score(img_o, img_r, dep_r, mode, 0.02, depth_observed=dep_o if mode == "depth" else None, bbox=bbox, status=status,
                         workspace=work.view())
    work.check("dim_pose_score workspace, mode " + mode)
    got = s.cpu().numpy().astype(np.float64)
    want = hr.scores(mode, img_o.cpu().numpy(), img_r.cpu().numpy(), dep_r.cpu().numpy(), bbox.cpu().numpy(), dep_o.cpu().numpy(), 0.02)
    st = status.cpu().numpy()
    for b in range(B):
        if np.isinf(want[b]):
            assert got[b] == -np.inf and st[b] == hr.STATUS_HYP_NO_SCORE, (mode, b, got[b])
        else:
            assert abs(got[b] - want[b]) <= 1e-5, (mode, b, got[b], want[b])
            assert st[b] == 0, (mode, b)
    undefined = {"rgb": {2, 3, 7}, "depth": {2, 5, 6}}[mode]
    assert {b for b in range(B) if np.isinf(want[b])} == undefined
    assert np.ptp(want[[b for b in range(B) if b not in undefined]]) > 0.05   # the scores differ: the check is not vacuous
    # the whole frame gives the same score (S is the drawn pixels); the box only restricts the work
    s_full = ops().pose_score(img_o, img_r, dep_r, mode, 0.02, depth_observed=dep_o if mode == "depth" else None, bbox=None)
    for b in (0, 1, 4):
        assert abs(float(s_full[b]) - want[b]) <= 1e-5, (mode, b)
    # the same launch twice: bit-identical (fixed summation order)
    s2 = ops().pose_score(img_o, img_r, dep_r, mode, 0.02, depth_observed=dep_o if mode == "depth" else None, bbox=bbox)
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32))


def test_select_matches_restatement(hip_lib):
    P, N, T = 5, 4, 3
    nan, inf = float("nan"), float("inf")
    score = np.array([0.1, 0.5, 0.5, -inf,      # tie: the smaller h
                      nan, -inf, -inf, -inf,    # nothing finite: h = 0 and the status bit
                      0.2, nan, 0.2, 0.3,
                      nan, -0.9, nan, -0.95,
                      -inf, -inf, -inf, 0.0], np.float32)
    rng = np.random.default_rng(1)
    poses = rng.normal(size=(T, P * N, 3, 4)).astype(np.float32)
    status = rng.integers(0, 16, size=(T, P * N)).astype(np.int32)
    icp = rng.normal(size=(P * N, 3, 4)).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    load = np.zeros((P * N,), np.int32)
    load[[1, 4, 7]] = [16, 8, 4]   # render bits of the load-time renders: only the winner's reach its pair (samples 1 and 4 win)
    choice, psel, ssel, isel = ops().hyp_select(d(score), N, d(poses), status_iter=d(status), pose_icp=d(icp), status_load=d(load))
    c, none = hr.select(score, N)
    assert choice.cpu().tolist() == c.tolist() == [1, 0, 3, 1, 3]
    wp, ws, wi = hr.gather(c, N, poses, status, icp)
    np.testing.assert_array_equal(psel.cpu().numpy(), wp)
    np.testing.assert_array_equal(isel.cpu().numpy(), wi)
    ws = ws.copy()
    ws[T - 1, none] |= hr.STATUS_HYP_NO_SCORE
    ws[T - 1, :2] |= [16, 8]
    np.testing.assert_array_equal(ssel.cpu().numpy(), ws)
    # optional outputs
    choice2, psel2, ssel2, isel2 = ops().hyp_select(d(score), N, d(poses))
    assert ssel2 is None and isel2 is None and torch.equal(choice2, choice) and torch.equal(psel2, psel)


# ------------------------------------------------------------------------------------------------------------------ the Refiner
P, N = 2, 4


def _cfg(test_iter=2, n=N, mode="rgb"):
    cfg = make_test_config(test_iter=test_iter)
    cfg.TEST.HYP_NUM = n
    cfg.TEST.HYP_SCORE = mode
    return cfg


def _params(cfg, head):
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    if head == "identity":   # the pose head emits (1,0,0,0 | 0,0,0) whatever it sees: every sample keeps its starting pose
        for k in ("rot_weight", "trans_weight", "trans_bias"):
            params[k] = np.zeros_like(params[k])
        params["rot_bias"] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    else:
        moving_head(params, seed=1)
    return params


@pytest.fixture(scope="module")
def identity_setup(rscene):
    from deepim.core.tester import Predictor
    from lib.utils import synthetic as syn

    models, rm = rscene
    cfg = _cfg()
    params = _params(cfg, "identity")
    pred = Predictor(cfg, params, P * N)
    # the observed pairs: device renders at GT; the hypotheses: GT at a non-zero index, the others 15-60 deg away
    _, gt, _ = syn.sample_pairs(31, P)
    img_o, dep_o, _ = _render(rm, gt)
    dep_o = torch.where(dep_o > 0, dep_o, torch.full_like(dep_o, 1.5))   # in front of a wall: a silhouette mismatch counts as an outlier
    hyp = np.zeros((P, N, 3, 4), np.float32)
    gt_idx = [1 + p % (N - 1) for p in range(P)]
    axes = hr.fibonacci_axes(N)
    for p in range(P):
        for h in range(N):
            hyp[p, h] = gt[p]
            if h != gt_idx[p]:
                hyp[p, h, :, :3] = _rot(axes[h], 15.0 + 15.0 * h) @ gt[p][:, :3]
    return cfg, rm, pred, gt, img_o, dep_o, hyp, gt_idx


def _load_hyp(ref, img_o, dep_o, hyp, src=None):
    z3 = torch.zeros((P, 3, H, W), device=DEV)
    z1 = torch.zeros((P, 1, H, W), device=DEV)
    src = hyp[:, 0] if src is None else src
    ref.load(img_o, z3, z1, z1, src, torch.zeros((P,), dtype=torch.int32), depth_observed=dep_o, hyp_poses=hyp)


def test_identity_head_keeps_the_pose(hip_lib):
    cfg = _cfg()
    pose = torch.from_numpy(np.array([[[0.6, -0.8, 0.0, 0.01], [0.8, 0.6, 0.0, -0.02], [0.0, 0.0, 1.0, 0.9]]], np.float32)).to(DEV)
    se3 = torch.tensor([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
    out = ops().se3_compose(pose, se3, cfg.network.ROT_COORD, np.zeros(3, np.float32), np.ones(3, np.float32))
    np.testing.assert_allclose(out.cpu().numpy(), pose.cpu().numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("mode", ["rgb", "depth"])
def test_selection_picks_the_true_pose(identity_setup, mode):
    from deepim.core.tester import Refiner

    cfg, rm, pred, gt, img_o, dep_o, hyp, gt_idx = identity_setup
    _cfg()   # the config is global: re-establish the one the fixture's Predictor was built for
    cfg.TEST.HYP_SCORE = mode
    try:
        ref = Refiner(cfg, pred, rm, P, capture_graph=True)
        _load_hyp(ref, img_o, dep_o, hyp)
        sel = ref.refine().cpu().numpy()
        assert ref.graph is not None
        score = ref.hyp_score.cpu().numpy().reshape(P, N)
        assert ref.hyp_choice.cpu().tolist() == gt_idx, (mode, score)
        np.testing.assert_allclose(sel[-1], gt, rtol=0, atol=1e-5)
        assert np.all(np.isfinite(score)) and ref.status_sel.cpu().numpy()[-1].tolist() == [0] * P
        assert ref.status_hyp.cpu().tolist() == [0] * (P * N)
        np.testing.assert_allclose(ref.poses_iter.cpu().numpy()[-1], hyp.reshape(P * N, 3, 4), rtol=0, atol=1e-5)
        # negative control: the observed images (and depths) swapped between the pairs -> another choice
        _load_hyp(ref, img_o.flip(0).contiguous(), dep_o.flip(0).contiguous(), hyp)
        ref.refine()
        assert ref.hyp_choice.cpu().tolist() != gt_idx, (mode, ref.hyp_score.cpu().numpy().reshape(P, N))
    finally:
        cfg.TEST.HYP_SCORE = "rgb"


@pytest.mark.parametrize("input_depth", [False, True])
def test_hypothesis_zero_matches_the_plain_loop(rscene, input_depth):
    """generated hypotheses under a head that moves 3-12 deg per iteration: row h = 0 is the HYP_NUM = 1 loop on the same pairs.
    INPUT_DEPTH: the observed depth reaches every hypothesis row and the loaded rendered depth stays with h = 0 (the 10-channel first
    layer reads both, with weights on the depth lanes)"""
    from deepim.core.tester import Predictor, Refiner

    models, rm = rscene
    scene = make_scene(B=P, seed=2333, subdiv=3)
    bl = scene["blobs"]
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    from lib.render_hip.render_py_multi import Render_Py

    rm = Render_Py(None, ["ape"], scene["K"], meshes=scene["models"])
    cfg1 = _cfg(n=1)
    cfg1.network.INPUT_DEPTH = input_depth
    params = _params(cfg1, "moving")
    dkw = {}
    if input_depth:
        rng = np.random.RandomState(3)
        params["flow_conv1_weight"][:, 6:] = (rng.randn(64, params["flow_conv1_weight"].shape[1] - 6, 7, 7) * 0.05).astype(np.float32)
        dkw = {"depth_observed": (0.6 + 0.6 * rng.rand(P, 1, H, W)).astype(np.float32),
               "depth_rendered": (0.6 + 0.6 * rng.rand(P, 1, H, W)).astype(np.float32)}
    plain = Refiner(cfg1, Predictor(cfg1, params, P), rm, P)
    plain.load(*args, **dkw)
    want = plain.refine().cpu().numpy()
    cfg = _cfg()
    cfg.network.INPUT_DEPTH = input_depth
    ref = Refiner(cfg, Predictor(cfg, params, P * N), rm, P)
    ref.load(*args, **dkw)
    ref.refine()
    if input_depth:
        np.testing.assert_array_equal(ref.batch["depth_observed"].cpu().numpy(), np.repeat(dkw["depth_observed"], N, axis=0))
        np.testing.assert_array_equal(ref.init["depth_rendered"].cpu().numpy()[::N], dkw["depth_rendered"])
        assert float(ref.init["depth_rendered"][1].max()) > 0.2   # the other hypotheses carry their own rendered depth
    got = ref.poses_iter.cpu().numpy()[:, ::N]
    # the first iteration sees identical inputs in both batches: equal to f32 summation order (the batch-slice bar).  Under this head
    # a 1e-6 difference grows 10-200x per iteration (tests/loop_parity.py), so the last one is held to a looser bound
    assert np.abs(got[0] - want[0]).max() <= 2e-5 * max(1.0, float(np.abs(want[0]).max())), np.abs(got[0] - want[0]).max()
    assert np.abs(got - want).max() <= 2e-3, np.abs(got - want).max()
    start = ref.pose_init.cpu().numpy().reshape(P, N, 3, 4)
    np.testing.assert_array_equal(start[:, 0], bl["src_pose"])
    for p in range(P):   # the generated starts: [R_h R_p | t_p]
        np.testing.assert_allclose(start[p], hr.expand(hr.rotation_table(N, 30.0), bl["src_pose"][p:p + 1]), rtol=0, atol=1e-6)
    # the loaded planes stay with hypothesis 0; the others were rendered
    ir = ref.init["image_rendered"].cpu().numpy()
    np.testing.assert_array_equal(ir[::N], bl["image_rendered"])
    assert not np.array_equal(ir[1], ir[0])


def test_graph_replay_and_new_load(identity_setup):
    from deepim.core.tester import Refiner

    cfg, rm, pred, gt, img_o, dep_o, hyp, gt_idx = identity_setup
    _cfg()   # the config is global: re-establish the one the fixture's Predictor was built for
    ref = Refiner(cfg, pred, rm, P, capture_graph=True)
    _load_hyp(ref, img_o, dep_o, hyp)
    ref.refine()
    a = (ref.hyp_score.cpu().numpy().copy(), ref.hyp_choice.cpu().numpy().copy())
    ref.refine()
    b = (ref.hyp_score.cpu().numpy().copy(), ref.hyp_choice.cpu().numpy().copy())
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    # a new load(): GT moved to hypothesis 0 -- the replayed graph reads the resident buffers
    hyp2 = hyp.copy()
    for p in range(P):
        hyp2[p, [0, gt_idx[p]]] = hyp[p, [gt_idx[p], 0]]
    _load_hyp(ref, img_o, dep_o, hyp2)
    ref.refine()
    assert ref.hyp_choice.cpu().tolist() == [0] * P
    assert not np.array_equal(ref.hyp_score.cpu().numpy(), a[0])


def test_load_staged_equals_load(rscene):
    from deepim.core.loader import ArraySource, TestDataLoader, raw_from_device_batch
    from deepim.core.tester import Predictor, Refiner
    from lib.utils import synthetic as syn

    models, rm = rscene
    cfg = _cfg()
    cfg.TEST.MASK_DILATE = False
    params = _params(cfg, "moving")
    ref = Refiner(cfg, Predictor(cfg, params, P * N), rm, P, capture_graph=True)
    b = syn.build_device_batch(rm, P, seed=70)
    depth = torch.empty((P, 1, H, W), device=DEV)
    rm.render_batch(b["class_index"], b["src_pose"], depth=depth)
    raw = raw_from_device_batch(b, cfg.network.PIXEL_MEANS, depth)
    loader = TestDataLoader(None, cfg, batch_size=P, device=DEV, workers=2, source=ArraySource(*raw))
    batch = next(iter(loader))
    ref.load(batch["image_observed"], batch["image_rendered"], batch["mask_observed"], batch["mask_rendered"], batch["src_pose"],
             batch["class_index"])
    direct = [t.cpu().numpy().copy() for t in (ref.refine(), ref.hyp_score, ref.poses_iter)]
    loader.close()
    loader = TestDataLoader(None, cfg, batch_size=P, device=DEV, workers=2, source=ArraySource(*raw))
    ref.load_staged(loader, loader.next_raw())
    staged = [t.cpu().numpy() for t in (ref.refine(), ref.hyp_score, ref.poses_iter)]
    loader.close()
    for x, y in zip(direct, staged):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_pred_eval_with_hypotheses_and_icp(hip_lib):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from lib.dataset.synthetic_pairs import SyntheticPairs

    cfg = _cfg(mode="depth")
    cfg.TEST.ICP_ITER = 3
    try:
        params = _params(cfg, "moving")
        data = SyntheticPairs(cfg, 4, P, subdiv=3)
        pred = Predictor(cfg, params, P * N)
        with pytest.raises(ValueError, match="Predictor was built for"):
            Refiner(cfg, Predictor(cfg, params, P), data.render_machine, P)
        ref = Refiner(cfg, pred, data.render_machine, P, capture_graph=True)
        batches = list(data.test_batches())
        with pytest.raises(ValueError, match="depth_observed"):
            bl = batches[0]
            ref.load(*[bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
        sel_icp = []

        class Spy(object):   # pred_eval's refiner, recording the ICP outputs of every batch
            def __getattr__(self, k):
                return getattr(ref, k)

            def refine(self):
                out = ref.refine()
                idx = np.arange(P) * N + ref.hyp_choice.cpu().numpy()
                sel_icp.append((ref.pose_icp_sel.cpu().numpy().copy(), ref.pose_icp.cpu().numpy()[idx]))
                return out

        out = pred_eval(cfg, Spy(), batches, data.evaluator())
        hyp = out["hyp"]
        assert hyp["num"] == N and len(hyp["choice"]) == 4 and all(len(s) == N for s in hyp["score"])
        last = sorted(r for c in range(len(out["all_rot_err"])) for r in out["all_rot_err"][c][-1])
        np.testing.assert_allclose(last, sorted(hyp["rot_err"][p][hyp["choice"][p]] for p in range(4)), rtol=1e-9, atol=1e-9)
        assert 0.0 <= hyp["chosen_is_least_rot_err"] <= 1.0
        assert len(out["icp"]["add"]["overall"]) == 1
        for got, want in sel_icp:
            np.testing.assert_array_equal(got, want)
    finally:
        cfg.TEST.ICP_ITER = 0
        cfg.TEST.HYP_NUM = 1


def test_lit_renderer_is_refused(hip_lib):
    from deepim.core.tester import Refiner

    class Lit(object):
        normals = None

    class FakePred(object):
        class net(object):
            B = P * N

    with pytest.raises(ValueError, match="lit"):
        Refiner(_cfg(), FakePred(), Lit(), P)
