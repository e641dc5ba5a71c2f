"""Pose from predicted flow on the device (csrc/flow_pnp.hip, dim_flow_pnp / ops.flow_pnp): against the float64 restatement
tests/flow_pnp_reference.py on the small-frame inputs that tests/test_flow_pnp_host.py proves sound, flagging, determinism under graph
replay, argument errors, the Refiner stage inside the captured full-graph loop and pred_eval's out["flow_pnp"]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_pnp_reference as fr  # noqa: E402
import guard_arena  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402
from test_flow_pnp_host import GATE, HUBER, ITERS, WARM, gpu_batches  # noqa: E402

DEV = "cuda:0"


def ops():
    from lib.hip import ops as o

    return o


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _within_bar(got, want, what):
    """the kernel is float64 throughout, so it differs from the restatement by the order of its sums (~1e-13) and its float32 outputs
    by at most a rounding: the bar is 10 x the float32 output rounding, 1e-6 max(1, |x|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff = np.abs(got - want)
    bar = 1e-6 * np.maximum(1.0, np.abs(want))
    print("{}: max |hip - restatement| = {:.3e} (largest ratio to the bar {:.3e})".format(what, diff.max(), (diff / bar).max()))
    assert np.all(diff <= bar), (what, float(diff.max()))


@pytest.fixture(scope="module")
def batches(hip_lib):
    return gpu_batches()


def _stack(cases, clip_last=False):
    depth = np.stack([c["depth"] for c in cases])[:, None]
    flow = np.stack([c["flow"] for c in cases])
    valid = np.stack([c["visible"] for c in cases])[:, None]
    bbox = np.stack([c["bbox"] for c in cases]).astype(np.int32)
    if clip_last:   # a box that reaches over the frame on three sides: the stage clips it
        bbox[-1] += np.array([-70, 200, -3, 100], np.int32)
    pose = np.stack([c["pose_src"] for c in cases])
    Ks = np.stack([c["K"] for c in cases]).reshape(len(cases), 9)
    return depth, flow, valid, bbox, pose, Ks


def _hip(depth, flow, valid, bbox, pose, K, Ks, iters, rep, warm=WARM, huber=HUBER, gate=GATE):
    B = pose.shape[0]
    stats = torch.zeros((B, max(iters, 1), 2), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    out, q = ops().flow_pnp(_dev(depth), _dev(flow), _dev(pose), K, iters, warm, huber, gate, standard_rep=rep,
                            valid=None if valid is None else _dev(valid), bbox=None if bbox is None else _dev(bbox, torch.int32),
                            K_per_sample=None if Ks is None else _dev(Ks), stats=stats, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), q.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("iters", [1, ITERS])
@pytest.mark.parametrize("use_bbox", [True, False])
def test_hip_matches_restatement(batches, iters, use_bbox):
    """B = 3 at 48x64 (16-byte loads) and B = 2 at 37x50 (scalar path, odd row stride), both flow orders, every pair but the first
    with its own K, one box clipped by the frame or no box at all; 30 % of the correspondences displaced by 20-60 px"""
    for name, H, W, cases, rep in batches:
        depth, flow, valid, bbox, pose, Ks = _stack(cases, clip_last=True)
        assert not np.array_equal(Ks[0], Ks[1])   # the second pair has a camera of its own
        bb = bbox if use_bbox else None
        got = _hip(depth, flow, valid, bb, pose, Ks[0].reshape(3, 3), Ks, iters, rep)
        want = fr.flow_pnp(depth, flow, pose, Ks, iters, WARM, HUBER, GATE, standard_rep=rep, valid=valid, bbox=bb)
        what = "{} rep={} iters={} bbox={}".format(name, rep, iters, use_bbox)
        assert got[3].tolist() == want[3].tolist() == [0] * len(cases), what
        np.testing.assert_array_equal(got[2][:, :, 0], want[2][:, :, 0], err_msg=what)   # the counts, at every iteration
        if iters == ITERS:
            assert got[2][:, -1, 0].tolist() == [float(c["n_inliers"]) for c in cases], what
        _within_bar(got[0], want[0], what + " pose_out")
        _within_bar(got[1], want[1], what + " se3_q")
        np.testing.assert_allclose(got[2][:, :, 1], want[2][:, :, 1], rtol=1e-5, atol=1e-7, err_msg=what)   # rms: a float32 output


def test_host_K_and_no_valid(batches):
    """K_per_sample = NULL uses the host K for every pair; valid = NULL takes every drawn pixel"""
    name, H, W, cases, rep = batches[0]
    depth, flow, valid, bbox, pose, Ks = _stack(cases)
    K0 = Ks[0].reshape(3, 3)
    got = _hip(depth, flow, None, bbox, pose, K0, None, ITERS, rep)
    want = fr.flow_pnp(depth, flow, pose, K0, ITERS, WARM, HUBER, GATE, standard_rep=rep, valid=None, bbox=bbox)
    np.testing.assert_array_equal(got[2][:, :, 0], want[2][:, :, 0])
    assert got[3].tolist() == want[3].tolist()
    _within_bar(got[0], want[0], "host K pose_out")


def test_flagging_leaves_the_neighbours_alone(batches):
    name, H, W, cases, rep = batches[0]
    depth, flow, valid, bbox, pose, Ks = _stack(cases)
    full = _hip(depth, flow, valid, bbox, pose, Ks[0].reshape(3, 3), Ks, ITERS, rep)
    depth2 = depth.copy()
    depth2[1] = 0.0
    got = _hip(depth2, flow, valid, bbox, pose, Ks[0].reshape(3, 3), Ks, ITERS, rep)
    assert got[3].tolist() == [0, fr.STATUS_FLOW_PNP_FEW_POINTS, 0]
    assert np.array_equal(got[0][1].view(np.uint32), pose[1].view(np.uint32))
    assert got[1][1].tolist() == [1, 0, 0, 0, 0, 0, 0] and got[2][1, :, 0].max() == 0
    for b in (0, 2):
        for k in range(3):
            assert np.array_equal(got[k][b].view(np.uint32), full[k][b].view(np.uint32)), (b, k)
    # a bad focal length and an all-NaN flow are flagged the same way
    Kbad = Ks.copy()
    Kbad[2, 0] = -Kbad[2, 0]
    flow2 = flow.copy()
    flow2[0] = np.nan
    got = _hip(depth, flow2, valid, bbox, pose, Ks[0].reshape(3, 3), Kbad, ITERS, rep)
    assert got[3].tolist() == [fr.STATUS_FLOW_PNP_FEW_POINTS, 0, fr.STATUS_FLOW_PNP_FEW_POINTS]
    assert np.array_equal(got[0][[0, 2]].view(np.uint32), pose[[0, 2]].view(np.uint32))
    assert np.array_equal(got[0][1].view(np.uint32), full[0][1].view(np.uint32))
    # iters == 0: a copy and the identity
    got = _hip(depth, flow, valid, bbox, pose, Ks[0].reshape(3, 3), Ks, 0, rep)
    assert np.array_equal(got[0].view(np.uint32), pose.view(np.uint32)) and got[3].tolist() == [0, 0, 0]
    assert got[1].tolist() == [[1, 0, 0, 0, 0, 0, 0]] * 3


def test_eager_and_graph_replays_are_bit_identical(batches):
    name, H, W, cases, rep = batches[1]   # the scalar path
    depth, flow, valid, bbox, pose, Ks = _stack(cases)
    B = pose.shape[0]
    args = (_dev(depth), _dev(flow), _dev(pose), Ks[0].reshape(3, 3), ITERS, WARM, HUBER, GATE)
    o = ops()
    bufs = dict(pose_out=torch.zeros((B, 3, 4), device=DEV), se3_q=torch.zeros((B, 7), device=DEV), stats=torch.zeros((B, ITERS, 2), device=DEV),
                status=torch.zeros((B,), dtype=torch.int32, device=DEV))
    # the workspace: exactly dim_flow_pnp_workspace_bytes between guards, at the documented minimum alignment (8 mod 16), NaN bits
    work = guard_arena.workspace(o.lib().dim_flow_pnp_workspace_bytes(B, H, W), 8, DEV)
    bufs["workspace"] = work.view()
    kw = dict(standard_rep=rep, valid=_dev(valid), bbox=_dev(bbox, torch.int32), K_per_sample=_dev(Ks), **bufs)

    def snapshot():
        torch.cuda.synchronize()
        out = [bufs[k].cpu().numpy().copy() for k in ("pose_out", "se3_q", "stats")]
        for k in ("pose_out", "se3_q", "stats"):
            bufs[k].fill_(-7.0)
        work.check("dim_flow_pnp workspace")
        bufs["workspace"].fill_(float("nan"))   # the workspace needs no initialisation
        torch.cuda.synchronize()
        return out

    o.flow_pnp(*args, **kw)
    first = snapshot()
    o.flow_pnp(*args, **kw)
    runs = [snapshot()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o.flow_pnp(*args, **kw)
    torch.cuda.current_stream().wait_stream(s)
    snapshot()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o.flow_pnp(*args, **kw)
    for _ in range(2):
        g.replay()
        runs.append(snapshot())
    assert np.abs(first[0] - pose).max() > 1e-3
    for r in runs:
        for a, b in zip(first, r):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_argument_errors_leave_pose_out_unwritten(batches):
    from lib.hip.capi import DeepIMHipError

    name, H, W, cases, rep = batches[0]
    depth, flow, valid, bbox, pose, Ks = _stack(cases)
    d, f, p = _dev(depth), _dev(flow), _dev(pose)
    out = torch.full((3, 3, 4), -7.0, device=DEV)
    K0 = Ks[0].reshape(3, 3)
    for kw in (dict(iters=-1), dict(warm=-1), dict(huber_px=0.0), dict(huber_px=-2.0), dict(huber_px=4.0, max_px=3.0)):
        a = dict(iters=ITERS, warm=WARM, huber_px=HUBER, max_px=GATE)
        a.update(kw)
        with pytest.raises(DeepIMHipError, match="flow_pnp"):
            ops().flow_pnp(d, f, p, K0, a["iters"], a["warm"], a["huber_px"], a["max_px"], pose_out=out)
    L, o = ops().lib(), ops()
    ws = o.flow_pnp_workspace(3, H, W, DEV)
    k9 = np.ascontiguousarray(K0, np.float32)

    def raw(B=3, dp=d.data_ptr(), fp=f.data_ptr(), pp=p.data_ptr(), kp=k9.ctypes.data, wp=ws.data_ptr(), op=out.data_ptr()):
        return L.dim_flow_pnp(dp, fp, None, None, pp, kp, None, B, H, W, 0, ITERS, WARM, HUBER, GATE, wp, op, None, None, None, None)

    for kw in (dict(B=0), dict(B=-3), dict(dp=None), dict(fp=None), dict(pp=None), dict(kp=None), dict(wp=None), dict(op=None)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------------------------ the Refiner stage
def _cam(K, sx, sy, dx, dy):
    K = np.array(K, dtype=np.float32).copy()
    K[0, 0] *= sx
    K[1, 1] *= sy
    K[0, 2] += dx
    K[1, 2] += dy
    return K


@pytest.fixture(scope="module")
def loop_setup(hip_lib):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.render_hip.render_py_multi import Render_Py
    from loop_parity import moving_head

    cfg = make_test_config(test_iter=3)
    cfg.TEST.FAST_TEST = False   # the full graph: decoder, mask and flow heads at every iteration
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1, rot_scale=1e-4, trans_scale=1e-4)
    rng = np.random.RandomState(5)
    params["Convolution3_weight"] = (rng.randn(*params["Convolution3_weight"].shape) * 0.05).astype(np.float32)   # a flow head that says something
    B = 2
    scene = make_scene(B=B, seed=2333, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    yield cfg, scene, rm, pred
    cfg.TEST.FAST_TEST = True


def _refiner(setup, flow_iter, graph=False):
    from deepim.core.tester import Refiner

    cfg, scene, rm, pred = setup
    cfg.TEST.FLOW_PNP_ITER = flow_iter
    try:
        return Refiner(cfg, pred, rm, 2, capture_graph=graph)
    finally:
        cfg.TEST.FLOW_PNP_ITER = 0


def _load(ref, setup, K=None, shift=0.0):
    bl = setup[1]["blobs"]
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    if shift:
        args[4] = args[4].copy()
        args[4][:, 2, 3] += shift
    ref.load(*args, K=K)


def _loop_out(ref):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (ref.poses_iter, ref.se3_iter, ref.status_iter, ref.flow_est_iter, ref.batch["image_rendered"],
                                              ref.batch["mask_rendered"], ref.batch["mask_observed"])]


def _flow_out(ref):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in (ref.pose_flow_iter, ref.se3_flow_iter, ref.flow_pnp_stats, ref.status_flow)]


@pytest.mark.parametrize("graph", [False, True])
def test_refiner_flow_pnp_leaves_the_loop_alone(loop_setup, graph):
    off = _refiner(loop_setup, 0, graph)
    assert "flow_pnp" not in off.stages
    assert off.pose_flow_iter is None and off.se3_flow_iter is None and off.flow_pnp_stats is None and off.status_flow is None
    _load(off, loop_setup)
    off.refine()
    want = _loop_out(off)
    on = _refiner(loop_setup, ITERS, graph)
    _load(on, loop_setup)
    on.refine()
    assert (on.graph is not None) == graph
    for a, b in zip(want, _loop_out(on)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pose_flow, se3_flow, stats, status = _flow_out(on)
    assert pose_flow.shape == (3, 2, 3, 4) and se3_flow.shape == (3, 2, 7) and stats.shape == (3, 2, ITERS, 2) and status.shape == (3, 2)
    assert np.all(np.isfinite(pose_flow)) and stats[:, :, 0, 0].min() > 4 * fr.MIN_POINTS   # the stage saw the object at every iteration


@pytest.mark.parametrize("per_pair_K", [False, True])
def test_refiner_flow_pnp_equals_standalone(loop_setup, per_pair_K):
    cfg, scene, rm, pred = loop_setup
    K = np.stack([_cam(rm.K, 1.05, 1.05, 6.0, -4.0), _cam(rm.K, 0.95, 0.97, -5.0, 3.0)]) if per_pair_K else None
    ref = _refiner(loop_setup, ITERS)
    _load(ref, loop_setup, K=K)
    ref.refine()
    got = _flow_out(ref)
    Kd = _dev(K.reshape(2, 9)) if per_pair_K else None
    cls = torch.zeros((2,), dtype=torch.int32, device=DEV)
    valid = _dev(scene["blobs"]["mask_observed"])   # the first forward reads the loaded mask, the later ones the box of the render
    for it in range(3):
        src = ref.pose_init if it == 0 else ref.poses_iter[it - 1]
        depth = torch.zeros((2, 1, 480, 640), dtype=torch.float32, device=DEV)
        bbox = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
        status = torch.zeros((2,), dtype=torch.int32, device=DEV)
        rm.render_batch(cls, src.contiguous(), K=Kd, depth=depth, bbox=bbox, mask_thr=0.0 if it == 0 else 0.2, status=status)
        if it > 0:
            ops().box_mask(bbox, valid)
        stats = torch.zeros((2, ITERS, 2), dtype=torch.float32, device=DEV)
        out, q = ops().flow_pnp(depth, ref.flow_est_iter[it], src.contiguous(), rm.K, ITERS, WARM, HUBER, GATE,
                                standard_rep=bool(cfg.network.STANDARD_FLOW_REP), valid=valid, bbox=bbox, K_per_sample=Kd, stats=stats,
                                status=status)
        torch.cuda.synchronize()
        for a, b in zip((out, q, stats, status), got):
            assert np.array_equal(a.cpu().numpy(), b[it]), it
    assert np.abs(got[0] - ref.poses_iter.cpu().numpy()).max() > 1e-5   # not the head's poses


def test_refiner_flow_pnp_graph_replays_match_eager(loop_setup):
    eager, g = _refiner(loop_setup, ITERS, graph=False), _refiner(loop_setup, ITERS, graph=True)
    outs = []
    for shift in (0.0, 0.03):   # two different loads
        _load(eager, loop_setup, shift=shift)
        eager.refine()
        want = _loop_out(eager) + _flow_out(eager)
        _load(g, loop_setup, shift=shift)
        g.refine()
        assert g.graph is not None
        for a, b in zip(want, _loop_out(g) + _flow_out(g)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        outs.append(want[7])
    assert np.abs(outs[0] - outs[1]).max() > 1e-3


def test_refiner_refuses_what_the_stage_cannot_do(loop_setup):
    from deepim.core.tester import Refiner

    cfg, scene, rm, pred = loop_setup
    cfg.TEST.FLOW_PNP_ITER = ITERS
    try:
        cfg.network.PRED_FLOW = False
        with pytest.raises(ValueError, match="FLOW_PNP_ITER.*PRED_FLOW"):
            Refiner(cfg, pred, rm, 2)
        cfg.network.PRED_FLOW = True
        cfg.TEST.FAST_TEST = True
        with pytest.raises(ValueError, match="FLOW_PNP_ITER.*FAST_TEST"):
            Refiner(cfg, pred, rm, 2)
        cfg.TEST.FAST_TEST = False
        cfg.TEST.HYP_NUM = 2
        with pytest.raises(ValueError, match="FLOW_PNP_ITER.*HYP_NUM"):
            Refiner(cfg, pred, rm, 1)
    finally:
        cfg.network.PRED_FLOW = True
        cfg.TEST.FAST_TEST = False
        cfg.TEST.HYP_NUM = 1
        cfg.TEST.FLOW_PNP_ITER = 0


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_pred_eval_scores_the_flow_poses(hip_lib):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs
    from test_gpu_pose_errors import _within_bar as errors_within_bar

    cfg = make_test_config(test_iter=2)
    cfg.TEST.FAST_TEST = False
    cfg.TEST.FLOW_PNP_ITER = ITERS
    try:
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = sym.init_weights(cfg, {}, {}, seed=0)
        B = 2
        data = SyntheticPairs(cfg, 4, B, subdiv=3)
        ref = Refiner(cfg, Predictor(cfg, params, B), data.render_machine, B, capture_graph=True)
        batches = list(data.test_batches())
        off = pred_eval(cfg, ref, batches, data.evaluator())
        cfg.TEST.DEVICE_EVAL = True
        on = pred_eval(cfg, ref, batches, data.evaluator())
        for out in (off, on):
            f = out["flow_pnp"]
            assert len(f["pose"]["overall"]) == len(out["pose"]["overall"]) and len(f["add"]["overall"]) == len(out["add"]["overall"]) == 2
            assert len(f["inliers"]) == len(f["rms"]) == len(f["flagged"]) == 2
            assert np.all(np.isfinite(f["inliers"])) and np.all(np.isfinite(f["rms"])) and min(f["inliers"]) > fr.MIN_POINTS
            assert sum(len(f["all_rot_err"][0][it]) for it in range(2)) == 8
            assert np.all(np.isfinite(np.asarray(f["all_rot_err"][0], np.float64)))
            assert np.all(np.isfinite(np.asarray(f["all_trans_err"][0], np.float64)))
        assert off["flow_pnp"]["all_rot_err"] == on["flow_pnp"]["all_rot_err"]   # the same poses were scored (host numbers in both)
        assert off["flow_pnp"]["inliers"] == on["flow_pnp"]["inliers"] and off["flow_pnp"]["flagged"] == on["flow_pnp"]["flagged"]
        a, b = off["flow_pnp"]["add"], on["flow_pnp"]["add"]
        assert set(a["errors"]) == set(b["errors"]) and len(a["errors"]) > 0
        for k in a["errors"]:
            errors_within_bar(b["errors"][k], a["errors"][k], "flow_pnp add {}".format(k))
        # the main tables are those of the stage off
        cfg.TEST.FLOW_PNP_ITER = 0
        cfg.TEST.DEVICE_EVAL = False
        plain = pred_eval(cfg, Refiner(cfg, Predictor(cfg, params, B), data.render_machine, B, capture_graph=True), batches, data.evaluator())
        assert "flow_pnp" not in plain
        assert plain["all_rot_err"] == off["all_rot_err"] and plain["all_trans_err"] == off["all_trans_err"]
        # a batch without the ground truth cannot be scored
        cfg.TEST.FLOW_PNP_ITER = ITERS
        bad = {k: v for k, v in batches[0].items() if k != "pose_observed"}
        with pytest.raises(KeyError, match="pose_observed"):
            pred_eval(cfg, ref, [bad], data.evaluator())
    finally:
        cfg.TEST.FLOW_PNP_ITER = 0
        cfg.TEST.DEVICE_EVAL = False
        cfg.TEST.FAST_TEST = True
