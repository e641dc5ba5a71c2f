"""Depth ICP after the refinement loop on the device (csrc/icp.hip, dim_icp_refine / ops.icp_refine): against the float64 restatement
tests/icp_reference.py on GPU-rendered planes, convergence, robustness, per-pair K, the Refiner stage inside the captured loop,
pred_eval's out["icp"] table and TestDataLoader's depth_observed blob."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import icp_reference as ir  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402
from test_icp_host import icp_pairs, noisy_depth  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
MAX_DIST = 0.02


def _cam(K, sx, sy, dx, dy):
    K = np.array(K, dtype=np.float32).copy()
    K[0, 0] *= sx
    K[1, 1] *= sy
    K[0, 2] += dx
    K[1, 2] += dy
    return K


@pytest.fixture(scope="module")
def icp_scene(hip_lib):
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    models, cls, gt, init = icp_pairs(16)
    rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
    return models, rm, cls, gt, init


def _render(rm, poses, K=None):
    """-> depth (B,1,H,W), bbox (B,4) of every drawn pixel, status: the ICP's render"""
    B = poses.shape[0]
    depth = torch.zeros((B, 1, H, W), dtype=torch.float32, device=DEV)
    bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    rm.render_batch(torch.zeros((B,), dtype=torch.int32, device=DEV), torch.as_tensor(poses).to(DEV), K=K, depth=depth, bbox=bbox,
                    mask_thr=0.0, status=status)
    return depth, bbox, status


def _icp(rm, dr, do, pose_in, iters, K=None, bbox=None, max_dist=MAX_DIST):
    B = pose_in.shape[0]
    stats = torch.zeros((B, max(iters, 1), 2), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    # the workspace: exactly dim_icp_workspace_bytes between guards, at the documented minimum alignment (8 mod 16), full of NaN bits
    work = guard_arena.workspace(ops().lib().dim_icp_workspace_bytes(B, H, W), 8, DEV)
    out = ops().icp_refine(dr, do, torch.as_tensor(pose_in).to(DEV), rm.K, iters, max_dist, bbox=bbox, K_per_sample=K, stats=stats,
                           status=status, workspace=work.view())
    work.check("dim_icp_refine workspace, B = {}".format(B))
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()


def ops():
    from lib.hip import ops as o

    return o


def _rot_err(Ra, Rb):
    """angle of Ra Rb^T in radians, from both its sine and cosine (arccos of the trace alone loses ~1e-4 rad near 0 in float32 poses)"""
    M = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.arctan2(s, (np.trace(M) - 1.0) / 2.0))


# ------------------------------------------------------------------------------------------------------------------ the kernels
def test_hip_matches_restatement_mixed_K(icp_scene):
    models, rm, cls, gt, init = icp_scene
    B = 8
    K0 = rm.K
    Ks = np.stack([K0 if b % 2 == 0 else _cam(K0, 1.0 + 0.03 * b, 1.0 + 0.02 * b, 4.0 * b - 10.0, 12.0 - 3.0 * b) for b in range(B)])
    Kd = torch.from_numpy(Ks.reshape(B, 9)).to(DEV)
    dr, bbox, st_r = _render(rm, init[:B], K=Kd)
    do, _, st_o = _render(rm, gt[:B], K=Kd)
    assert int(st_r.abs().sum()) == 0 and int(st_o.abs().sum()) == 0
    dr_h, do_h, bb_h = dr.cpu().numpy(), do.cpu().numpy(), bbox.cpu().numpy()
    pts = models[0][0].astype(np.float64)
    # one iteration: the data association and the solve
    p1, s1, f1 = _icp(rm, dr, do, init[:B], 1, K=Kd, bbox=bbox)
    r1, rs1, rf1 = ir.icp_refine(dr_h, do_h, init[:B], Ks, 1, MAX_DIST, bbox=bb_h)
    assert f1.tolist() == [0] * B and rf1.tolist() == [0] * B
    for b in range(B):
        n_hip, n_ref = s1[b, 0, 0], rs1[b, 0, 0]
        assert n_ref > 4 * ir.MIN_POINTS, b
        assert abs(n_hip - n_ref) <= 1e-3 * n_ref, (b, n_hip, n_ref)   # borderline float32 gate decisions
        assert _rot_err(p1[b][:, :3], r1[b][:, :3]) <= 2e-5, b
        assert np.linalg.norm(p1[b][:, 3].astype(np.float64) - r1[b][:, 3]) <= 2e-6, b
        assert abs(s1[b, 0, 1] - rs1[b, 0, 1]) <= 1e-3 * rs1[b, 0, 1] + 1e-7, b
    # ten iterations: the same ADD
    p10, s10, f10 = _icp(rm, dr, do, init[:B], 10, K=Kd, bbox=bbox)
    r10, _, _ = ir.icp_refine(dr_h, do_h, init[:B], Ks, 10, MAX_DIST, bbox=bb_h)
    assert f10.tolist() == [0] * B
    for b in range(B):
        assert abs(ir.add_error(p10[b], gt[b], pts) - ir.add_error(r10[b], gt[b], pts)) <= 1e-4, b
    # the box only restricts the work: the whole frame finds the same inliers (the lanes sum other pixels: last-bit differences)
    pf, sf, _ = _icp(rm, dr, do, init[:B], 10, K=Kd, bbox=None)
    np.testing.assert_array_equal(sf[:, 0, 0], s10[:, 0, 0])
    np.testing.assert_allclose(pf, p10, rtol=0, atol=1e-5)


def test_convergence_16_pairs(icp_scene):
    """the bars of tests/test_icp_host.py (fixed there on the restatement) on GPU renders at B = 16"""
    models, rm, cls, gt, init = icp_scene
    pts = models[0][0].astype(np.float64)
    dr, bbox, _ = _render(rm, init)
    do, _, _ = _render(rm, gt)
    pose, stats, status = _icp(rm, dr, do, init, 10, bbox=bbox)
    assert status.tolist() == [0] * 16
    for b in range(16):
        assert ir.add_error(init[b], gt[b], pts) > 2e-3, b
        assert ir.add_error(pose[b], gt[b], pts) <= 1e-3, b
        assert np.linalg.norm(pose[b][:, 3].astype(np.float64) - gt[b][:, 3]) <= 5e-4, b
        assert stats[b, -1, 1] < stats[b, 0, 1], b
    noisy = torch.from_numpy(noisy_depth(do.cpu().numpy(), 1)).to(DEV)
    pose, _, status = _icp(rm, dr, noisy, init, 10, bbox=bbox)
    assert status.tolist() == [0] * 16
    before = np.array([ir.add_error(init[b], gt[b], pts) for b in range(16)])
    after = np.array([ir.add_error(pose[b], gt[b], pts) for b in range(16)])
    assert after.mean() <= 3e-3, after
    assert int(np.sum(after < before)) >= 14, (before, after)


def test_empty_observed_depth_flags_one_pair_only(icp_scene):
    models, rm, cls, gt, init = icp_scene
    B = 4
    dr, bbox, _ = _render(rm, init[:B])
    do, _, _ = _render(rm, gt[:B])
    do[1].zero_()
    pose, stats, status = _icp(rm, dr, do, init[:B], 10, bbox=bbox)
    assert status.tolist() == [0, ir.STATUS_ICP_FEW_POINTS, 0, 0]
    assert np.array_equal(pose[1].view(np.uint32), init[1].view(np.uint32))
    assert stats[1, :, 0].max() == 0
    for b in (0, 2, 3):   # its neighbours are bit-identical to running them alone
        solo, solo_stats, solo_status = _icp(rm, dr[b:b + 1].contiguous(), do[b:b + 1].contiguous(), init[b:b + 1], 10,
                                             bbox=bbox[b:b + 1].contiguous())
        assert solo_status.tolist() == [0]
        assert np.array_equal(pose[b].view(np.uint32), solo[0].view(np.uint32)), b
        np.testing.assert_array_equal(stats[b], solo_stats[0])
    # iters == 0: a copy
    p0, _, s0 = _icp(rm, dr, do, init[:B], 0, bbox=bbox)
    assert np.array_equal(p0.view(np.uint32), init[:B].view(np.uint32)) and s0.tolist() == [0] * B


def test_per_pair_K(icp_scene):
    """a pair seen by another camera converges with its own K; given the config K it misses the bars (negative control)"""
    models, rm, cls, gt, init = icp_scene
    pts = models[0][0].astype(np.float64)
    Kb = _cam(rm.K, 1.15, 1.1, 25.0, -18.0)
    K2 = torch.from_numpy(np.stack([rm.K, Kb]).reshape(2, 9)).to(DEV)
    poses_i = np.stack([init[1], init[0]])
    poses_g = np.stack([gt[1], gt[0]])
    dr, bbox, _ = _render(rm, poses_i, K=K2)
    do, _, _ = _render(rm, poses_g, K=K2)
    pose, _, status = _icp(rm, dr, do, poses_i, 10, K=K2, bbox=bbox)
    assert status.tolist() == [0, 0]
    for b in range(2):
        assert ir.add_error(pose[b], poses_g[b], pts) <= 1e-3, b
        assert np.linalg.norm(pose[b][:, 3].astype(np.float64) - poses_g[b][:, 3]) <= 5e-4, b
    wrong, _, _ = _icp(rm, dr, do, poses_i, 10, K=None, bbox=bbox)
    assert not (ir.add_error(wrong[1], poses_g[1], pts) <= 1e-3 and np.linalg.norm(wrong[1][:, 3].astype(np.float64) - poses_g[1][:, 3]) <= 5e-4)
    np.testing.assert_array_equal(wrong[0], pose[0])   # the pair with the config K is unaffected


# ------------------------------------------------------------------------------------------------------------------ the Refiner stage
@pytest.fixture(scope="module")
def loop_setup(hip_lib):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.render_hip.render_py_multi import Render_Py

    cfg = make_test_config(test_iter=4)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1, rot_scale=1e-4, trans_scale=1e-4)   # a head that barely moves: the loop ends near the initial pose
    B = 2
    scene = make_scene(B=B, seed=2333, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    # the observed depth: the object a degree and a few millimetres from the initial pose, in front of a wall at 1.5 m
    from lib.utils import synthetic as syn

    rng = np.random.default_rng(9)
    obs = np.stack([syn.perturb_pose(rng, p, angle_std=1.0, angle_max=3.0, xy_std=0.002, z_std=0.004) for p in scene["pose_init"]])
    d, _, _ = _render(rm, torch.from_numpy(obs))
    wall = torch.where(d > 0, d, torch.full_like(d, 1.5))
    return cfg, scene, rm, pred, wall


def _refiner(setup, icp_iter, graph=False):
    from deepim.core.tester import Refiner

    cfg, scene, rm, pred, wall = setup
    cfg.TEST.ICP_ITER = icp_iter
    try:
        return Refiner(cfg, pred, rm, 2, capture_graph=graph)
    finally:
        cfg.TEST.ICP_ITER = 0


def _load(ref, setup, depth=None, K=None):
    bl = setup[1]["blobs"]
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    ref.load(*args, depth_observed=setup[4] if depth is None else depth, K=K)


def _loop_out(ref):
    return [t.cpu().numpy().copy() for t in (ref.poses_iter, ref.se3_iter, ref.status_iter)]


def _icp_out(ref):
    return [t.cpu().numpy().copy() for t in (ref.pose_icp, ref.icp_stats, ref.status_icp)]


@pytest.mark.parametrize("graph", [False, True])
def test_refiner_icp_leaves_the_loop_alone(loop_setup, graph):
    off = _refiner(loop_setup, 0, graph)
    assert off.pose_icp is None
    _load(off, loop_setup)
    off.refine()
    on = _refiner(loop_setup, 10, graph)
    _load(on, loop_setup)
    on.refine()
    torch.cuda.synchronize()
    for a, b in zip(_loop_out(off), _loop_out(on)):
        np.testing.assert_array_equal(a, b)
    _, stats, status = _icp_out(on)
    assert status.tolist() == [0, 0] and stats[:, 0, 0].min() > 4 * ir.MIN_POINTS


@pytest.mark.parametrize("per_pair_K", [False, True])
def test_refiner_icp_equals_standalone(loop_setup, per_pair_K):
    cfg, scene, rm, pred, wall = loop_setup
    K = np.stack([_cam(rm.K, 1.05, 1.05, 6.0, -4.0), _cam(rm.K, 0.95, 0.97, -5.0, 3.0)]) if per_pair_K else None
    ref = _refiner(loop_setup, 10)
    _load(ref, loop_setup, K=K)
    ref.refine()
    got = _icp_out(ref)
    last = ref.poses_iter[-1].clone()
    Kd = torch.from_numpy(K.reshape(2, 9)).to(DEV) if per_pair_K else None
    dr, bbox, st = _render(rm, last, K=Kd)
    stats = torch.zeros((2, 10, 2), dtype=torch.float32, device=DEV)
    out = ops().icp_refine(dr, wall, last, rm.K, 10, cfg.TEST.ICP_MAX_DIST, bbox=bbox, K_per_sample=Kd, stats=stats, status=st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got[0], out.cpu().numpy())
    np.testing.assert_array_equal(got[1], stats.cpu().numpy())
    np.testing.assert_array_equal(got[2], st.cpu().numpy())
    assert np.abs(got[0] - last.cpu().numpy()).max() > 1e-5   # the ICP did move the pose


def test_refiner_icp_graph_replay(loop_setup):
    eager = _refiner(loop_setup, 10, graph=False)
    _load(eager, loop_setup)
    eager.refine()
    e1 = _icp_out(eager)
    g = _refiner(loop_setup, 10, graph=True)
    _load(g, loop_setup)
    g.refine()
    assert g.graph is not None
    for a, b in zip(_icp_out(g), e1):
        np.testing.assert_array_equal(a, b)
    # a new batch (the observed depth 4 mm further away) reaches the replayed graph
    moved = loop_setup[4] + 0.004
    _load(g, loop_setup, depth=moved)
    g.refine()
    _load(eager, loop_setup, depth=moved)
    eager.refine()
    e2 = _icp_out(eager)
    for a, b in zip(_icp_out(g), e2):
        np.testing.assert_array_equal(a, b)
    assert np.abs(e2[0] - e1[0]).max() > 1e-3


def test_refiner_icp_needs_depth(loop_setup):
    ref = _refiner(loop_setup, 10)
    bl = loop_setup[1]["blobs"]
    with pytest.raises(ValueError):
        ref.load(*[bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_pred_eval_synthetic_pairs_with_icp(hip_lib):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs

    cfg = make_test_config(test_iter=2)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    B = 4
    data = SyntheticPairs(cfg, 8, B, subdiv=3)
    pred = Predictor(cfg, params, B)
    off = pred_eval(cfg, Refiner(cfg, pred, data.render_machine, B, capture_graph=True), data.test_batches(), data.evaluator())
    cfg.TEST.ICP_ITER = 10
    batches = list(data.test_batches())
    for b in batches:   # the GT render over a wall at 1.5 m
        assert float(b["depth_observed"].max()) == 1.5 and float(b["depth_observed"].min()) > 0.5
    on = pred_eval(cfg, Refiner(cfg, pred, data.render_machine, B, capture_graph=True), batches, data.evaluator())
    assert int(cfg.TEST.test_iter) == 2
    for k in ("pose", "add", "arp_2d"):
        for row_on, row_off in zip(on[k]["overall"], off[k]["overall"]):
            assert row_on == row_off, k
    for k in ("all_rot_err", "all_trans_err"):
        assert on[k] == off[k]
    assert on["icp"]["add"]["overall"][0]["0.02"] >= on["add"]["overall"][-1]["0.02"]
    assert on["icp"]["add"]["overall"][0]["auc"] >= on["add"]["overall"][-1]["auc"]
    cfg.TEST.ICP_ITER = 0


def test_loader_depth_observed_and_pred_eval(hip_lib, tmp_path):
    from PIL import Image

    from test_gpu_loader import _write_pairs
    from deepim.core.loader import TestDataLoader
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.evaluation import PoseEvaluator
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "can", "cat"]
    cfg.TEST.MASK_DILATE = False
    cfg.TEST.ICP_ITER = 5
    db = _write_pairs(str(tmp_path), 4)
    for rec in db:
        rec["depth_observed"] = rec["depth_gt_observed"]
    B = 2
    loader = TestDataLoader(db, cfg, batch_size=B, device=DEV, workers=2)
    assert "depth_observed" not in loader.data_name   # not a network input: INPUT_DEPTH stays off
    for k, batch in enumerate(loader):
        want = np.stack([np.asarray(Image.open(db[k * B + j]["depth_observed"]), np.uint16) for j in range(B)])
        want = (want.astype(np.float32) / np.float32(cfg.dataset.DEPTH_FACTOR))[:, None]
        got = batch["depth_observed"].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
    loader.close()
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    models = syn.make_models(seed=2333, n_models=3, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32), meshes=models)
    ref = Refiner(cfg, Predictor(cfg, params, B), rm, B, capture_graph=True)
    pts = {c: models[i][0].astype(np.float64) for i, c in enumerate(cfg.dataset.class_name)}
    diam = {c: float(np.linalg.norm(p.max(0) - p.min(0))) for c, p in pts.items()}
    loader = TestDataLoader(db, cfg, batch_size=B, device=DEV, workers=2)
    out = pred_eval(cfg, ref, loader, PoseEvaluator(cfg.dataset.class_name, pts, diam))
    loader.close()
    assert len(out["icp"]["add"]["overall"]) == 1
    assert sum(len(out["icp"]["all_rot_err"][c][0]) for c in range(3)) == 4
    cfg.TEST.ICP_ITER = 0
