"""Photometric pose polish after the refinement loop on the device (csrc/photo.hip, dim_photo_refine / ops.photo_refine): the kernels
against the restatement tests/photo_reference.py on the small frames of tests/test_photo_host.py::gpu_batches (planes bit for bit, the
gain sums, the counts, the pose and the rms), the behaviour of the entry point, convergence at full size on GPU renders, the Refiner
stage inside the captured loop and pred_eval's out["photo"] table.

Parity bars: pose_out within 1e-6 * max(1, |x|) and the rms column with rtol 1e-5 (tests/test_gpu_flow_pnp.py's, the arithmetic being
the same: float64 per point, float32 outputs); the five gain sums to 1e-12 relative; planes and counts equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import photo_reference as pr  # noqa: E402
import test_photo_host as host  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402
from test_photo_host import GATE, GPU_ITERS, GPU_LEVELS, HUBER, ITERS, LEVELS  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
FEW = pr.STATUS_PHOTO_FEW_POINTS


def ops():
    from lib.hip import ops as o

    return o


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def _photo(obs, ren, dep, pose_in, K, levels, iters, bbox=None, Kps=None, huber=HUBER, gate=GATE, gain=True, views=False):
    """one call on device tensors -> pose, stats, status (numpy) [, planes, sums]"""
    B, _, h, w = dep.shape
    stats = torch.zeros((B, max(levels * iters, 1), 2), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    # the workspace: exactly dim_photo_workspace_bytes between guards, at the alignment the fast path documents and no better (16 mod
    # 32), full of NaN bits
    arena = guard_arena.workspace(ops().lib().dim_photo_workspace_bytes(B, h, w, levels), 16, DEV)
    work = arena.view()
    out = ops().photo_refine(obs, ren, dep, pose_in, K, levels, iters, huber, gate, gain=gain, bbox=bbox, K_per_sample=Kps, stats=stats,
                             status=status, workspace=work)
    arena.check("dim_photo_refine workspace, B = {}, {} x {}, {} levels".format(B, h, w, levels))
    torch.cuda.synchronize()
    res = (out.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy())
    if views:
        planes, sums = ops().photo_workspace_views(work, B, h, w, levels)
        res += ({k: [p.cpu().numpy() for p in v] for k, v in planes.items()}, sums.cpu().numpy())
    return res


def _batch(which):
    g = host.gpu_batches()[which]
    t = {k: _dev(g[k]) for k in ("image_observed", "image_rendered", "depth_rendered", "pose_in", "K_per_sample")}
    t["bbox"] = _dev(g["bbox"], torch.int32)
    return g, t


def _call(g, t, iters, with_bbox=True, **kw):
    return _photo(t["image_observed"], t["image_rendered"], t["depth_rendered"], t["pose_in"], g["K"], GPU_LEVELS, iters,
                  bbox=t["bbox"] if with_bbox else None, Kps=t["K_per_sample"], **kw)


def _assert_pose(got, want, what):
    want = np.asarray(want, np.float64)
    bound = 1e-6 * np.maximum(1.0, np.abs(want))
    err = np.abs(np.asarray(got, np.float64) - want)
    print(what, "max pose error / bound", float((err / bound).max()))
    assert np.all(err <= bound), (what, float((err / bound).max()))


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("iters", [1, GPU_ITERS])
@pytest.mark.parametrize("which", [0, 1])
def test_hip_matches_restatement(hip_lib, which, iters, with_bbox):
    g, t = _batch(which)
    B = g["pose_in"].shape[0]
    pose, stats, status, planes, sums = _call(g, t, iters, with_bbox, views=True)
    r_pose, r_stats, r_status, extra = host.gpu_reference(which, iters, with_bbox)
    for b in range(B):
        pl = extra[b]["planes"]
        for lv in range(GPU_LEVELS):
            for kind in ("obs", "ren", "depth"):
                assert np.array_equal(planes[kind][lv][b].view(np.uint32), pl[kind][lv].view(np.uint32)), (b, kind, lv)
            assert np.array_equal(planes["valid"][lv][b].view(np.uint32), pl["valid"][lv].astype(np.float32).view(np.uint32)), (b, lv)
        want = extra[b]["sums"]
        assert sums[b, 0] == want[0]
        rel = np.abs(sums[b, :5] - want) / np.abs(want)
        print(which, iters, with_bbox, b, "gain sums rel", rel.max())
        assert np.all(rel <= 1e-12), (b, sums[b, :5], want)
        a, bias, ok = extra[b]["gain"]
        # a and b: the variances cancel a few digits of the sums' 1e-12
        assert sums[b, 7] == float(ok) and abs(sums[b, 5] - a) <= 1e-9 * abs(a) and abs(sums[b, 6] - bias) <= 1e-9 * max(1.0, abs(bias))
    np.testing.assert_array_equal(status, r_status)
    np.testing.assert_array_equal(stats[:, :, 0], r_stats[:, :, 0])
    np.testing.assert_allclose(stats[:, :, 1], r_stats[:, :, 1], rtol=1e-5, atol=0)
    _assert_pose(pose, r_pose, (which, iters, with_bbox))
    if which == 0 and with_bbox:   # the small window: flagged at the coarsest level, moved at level 0 (when it gets there)
        assert status[2] == FEW and (iters == 1 or not np.array_equal(pose[2], g["pose_in"][2]))


def test_host_K_without_per_sample_K(hip_lib):
    """pair 0's camera as the call's K9 for every pair, against the restatement given that one K"""
    g, t = _batch(0)
    pose, stats, status = _photo(t["image_observed"], t["image_rendered"], t["depth_rendered"], t["pose_in"], g["K"], GPU_LEVELS, GPU_ITERS,
                                 bbox=t["bbox"])
    r_pose, r_stats, r_status = pr.photo_refine(g["image_observed"], g["image_rendered"], g["depth_rendered"], g["pose_in"], g["K"],
                                                GPU_LEVELS, GPU_ITERS, HUBER, GATE, bbox=g["bbox"])
    np.testing.assert_array_equal(status, r_status)
    np.testing.assert_array_equal(stats[:, :, 0], r_stats[:, :, 0])
    np.testing.assert_allclose(stats[:, :, 1], r_stats[:, :, 1], rtol=1e-5, atol=0)
    _assert_pose(pose, r_pose, "host K")
    with_K = _call(g, t, GPU_ITERS)[0]
    assert np.array_equal(pose[0], with_K[0]) and not np.array_equal(pose[1], with_K[1])   # pair 0's camera is the same either way


@pytest.mark.parametrize("trigger", ["empty depth", "negative fx", "constant observed"])
def test_flagging_leaves_the_neighbours_alone(hip_lib, trigger):
    g, t = _batch(0)
    base = _call(g, t, GPU_ITERS)
    t = dict(t)
    if trigger == "empty depth":
        t["depth_rendered"] = t["depth_rendered"].clone()
        t["depth_rendered"][1].zero_()
    elif trigger == "negative fx":
        t["K_per_sample"] = t["K_per_sample"].clone()
        t["K_per_sample"][1, 0] = -t["K_per_sample"][1, 0]
    else:
        t["image_observed"] = t["image_observed"].clone()
        t["image_observed"][1] = 7.0
    pose, stats, status = _call(g, t, GPU_ITERS)
    assert status[1] == FEW and stats[1, :, 0].max() == 0
    assert np.array_equal(pose[1].view(np.uint32), g["pose_in"][1].view(np.uint32))
    for b in (0, 2):
        assert np.array_equal(pose[b].view(np.uint32), base[0][b].view(np.uint32)), b
        np.testing.assert_array_equal(stats[b], base[1][b])
        assert status[b] == base[2][b]


def test_zero_iterations_is_a_copy(hip_lib):
    g, t = _batch(1)
    pose, _, status = _call(g, t, 0)
    assert np.array_equal(pose.view(np.uint32), g["pose_in"].view(np.uint32)) and status.tolist() == [0, 0]


def test_eager_and_graph_replay_are_bit_identical(hip_lib):
    g, t = _batch(0)
    B = g["pose_in"].shape[0]
    o = ops()
    work = o.photo_workspace(B, g["H"], g["W"], GPU_LEVELS, DEV)
    pose = torch.zeros((B, 3, 4), device=DEV)
    stats = torch.zeros((B, GPU_LEVELS * GPU_ITERS, 2), device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def run():
        o.fill(status, 0)
        o.photo_refine(t["image_observed"], t["image_rendered"], t["depth_rendered"], t["pose_in"], g["K"], GPU_LEVELS, GPU_ITERS, HUBER, GATE,
                       bbox=t["bbox"], K_per_sample=t["K_per_sample"], pose_out=pose, stats=stats, status=status, workspace=work)

    def read():
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (pose, stats, status)]

    run()
    eager = read()
    run()
    for a, b in zip(read(), eager):
        np.testing.assert_array_equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        pose.zero_()
        stats.zero_()
        work.zero_()
        graph.replay()
        for a, b in zip(read(), eager):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ full size
def _render(rm, poses, K=None):
    """-> image (B,3,H,W) blob, depth (B,1,H,W), bbox (B,4), status: the stage's render"""
    from lib.utils import synthetic as syn

    B = poses.shape[0]
    image = torch.zeros((B, 3, H, W), dtype=torch.float32, device=DEV)
    depth = torch.zeros((B, 1, H, W), dtype=torch.float32, device=DEV)
    bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    rm.render_batch(torch.zeros((B,), dtype=torch.int32, device=DEV), torch.as_tensor(poses).to(DEV), K=K, image=image, depth=depth,
                    bbox=bbox, plane_means=syn.plane_means(), mask_thr=0.0, status=status)
    return image, depth, bbox, status


def test_convergence_16_pairs_full_size(hip_lib):
    """the bars of tests/test_photo_host.py (set there on the restatement) on GPU renders: one pair fewer than the restatement's N may
    end above 2 mm (the HIP rasteriser differs from the oracle's by edge pixels), none above 1.25 x its starting ADD"""
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn
    from test_icp_host import icp_pairs

    models, cls, gt, init = icp_pairs(16)
    rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
    pts = models[0][0].astype(np.float64)
    img_gt, d_gt, _, st_o = _render(rm, gt)
    ren, dep, bbox, st_r = _render(rm, init)
    assert int(st_o.abs().sum()) == 0 and int(st_r.abs().sum()) == 0
    img_h, d_h, pm = img_gt.cpu().numpy(), d_gt.cpu().numpy(), syn.plane_means()
    obs = _dev(np.stack([host.observed_recipe(img_h[b], d_h[b], 100 + b, pm) for b in range(16)]))
    pose, stats, status = _photo(obs, ren, dep, _dev(init), rm.K, LEVELS, ITERS, bbox=bbox)
    before, after = host.add_errors(init, gt, pts), host.add_errors(pose, gt, pts)
    n_ref = host.restatement_N()
    assert n_ref >= 14
    host.check_convergence(before, after, n_ref - 1)
    for b in np.nonzero(after <= host.ADD_OK)[0]:
        assert status[b] == 0 and stats[b, ITERS - 1, 1] < stats[b, 0, 1], b


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
    from lib.utils import synthetic as syn

    cfg = make_test_config(test_iter=2)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1, rot_scale=1e-4, trans_scale=1e-4)   # a head that barely moves: the loop ends near the initial pose
    B = 2
    scene = make_scene(B=B, seed=2333, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    # the observed image: the object a degree and a few millimetres from the initial pose, over noise, with another gain and bias
    rng = np.random.default_rng(9)
    at = np.stack([syn.perturb_pose(rng, p, angle_std=1.0, angle_max=3.0, xy_std=0.002, z_std=0.004) for p in scene["pose_init"]])
    img, d, _, _ = _render(rm, torch.from_numpy(at))
    img_h, d_h = img.cpu().numpy(), d.cpu().numpy()
    obs = _dev(np.stack([host.observed_recipe(img_h[b], d_h[b], 40 + b, syn.plane_means()) for b in range(B)]))
    yield cfg, scene, rm, pred, obs
    from deepim.config.config import reset_config

    reset_config()


def _refiner(setup, photo_iter, graph=False, **keys):
    from deepim.core.tester import Refiner

    cfg, scene, rm, pred, obs = setup
    old = {k: cfg.TEST.get(k) for k in keys}
    cfg.TEST.PHOTO_ITER = photo_iter
    cfg.TEST.update(keys)
    try:
        return Refiner(cfg, pred, rm, 2, capture_graph=graph)
    finally:
        cfg.TEST.PHOTO_ITER = 0
        cfg.TEST.update(old)


def _load(ref, setup, K=None, image=None):
    bl = setup[1]["blobs"]
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    args[0] = setup[4] if image is None else image
    ref.load(*args, K=K)


def _loop_out(ref):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (ref.poses_iter, ref.se3_iter, ref.status_iter)]


def _photo_out(ref):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (ref.pose_photo, ref.photo_stats, ref.status_photo)]


@pytest.mark.parametrize("graph", [False, True])
def test_refiner_photo_leaves_the_loop_alone(loop_setup, graph):
    off = _refiner(loop_setup, 0, graph)
    assert "photo" not in off.stages and off.pose_photo is None and off.photo_stats is None and off.status_photo is None
    _load(off, loop_setup)
    off.refine()
    want = _loop_out(off)
    on = _refiner(loop_setup, ITERS, graph)
    _load(on, loop_setup)
    on.refine()
    for a, b in zip(want, _loop_out(on)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    pose, stats, status = _photo_out(on)
    assert stats.shape == (2, LEVELS * ITERS, 2) and status.tolist() == [0, 0] and stats[:, :, 0].min() >= pr.MIN_POINTS
    assert np.abs(pose - want[0][-1]).max() > 1e-5   # the stage did move the pose


@pytest.mark.parametrize("per_pair_K", [False, True])
def test_refiner_photo_equals_standalone(loop_setup, per_pair_K):
    cfg, scene, rm, pred, obs = loop_setup
    K = np.stack([_cam(rm.K, 1.05, 1.05, 6.0, -4.0), _cam(rm.K, 0.95, 0.97, -5.0, 3.0)]) if per_pair_K else None
    ref = _refiner(loop_setup, ITERS)
    _load(ref, loop_setup, K=K)
    ref.refine()
    got = _photo_out(ref)
    last = ref.poses_iter[-1].clone()
    Kd = torch.from_numpy(K.reshape(2, 9)).to(DEV) if per_pair_K else None
    ren, dep, bbox, st = _render(rm, last, K=Kd)
    stats = torch.zeros((2, LEVELS * ITERS, 2), dtype=torch.float32, device=DEV)
    out = ops().photo_refine(obs, ren, dep, last, rm.K, LEVELS, ITERS, cfg.TEST.PHOTO_HUBER, cfg.TEST.PHOTO_MAX, gain=cfg.TEST.PHOTO_GAIN,
                             bbox=bbox, K_per_sample=Kd, stats=stats, status=st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got[0].view(np.uint32), out.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got[1], stats.cpu().numpy())
    np.testing.assert_array_equal(got[2], st.cpu().numpy())


def test_refiner_photo_graph_replay(loop_setup):
    eager = _refiner(loop_setup, ITERS, graph=False)
    _load(eager, loop_setup)
    eager.refine()
    e1 = _photo_out(eager)
    g = _refiner(loop_setup, ITERS, graph=True)
    _load(g, loop_setup)
    g.refine()
    assert g.graph is not None
    for a, b in zip(_photo_out(g), e1):
        np.testing.assert_array_equal(a, b)
    g.refine()    # a second replay
    for a, b in zip(_photo_out(g), e1):
        np.testing.assert_array_equal(a, b)
    # a new batch (a brighter observed image) reaches the replayed graph
    brighter = (loop_setup[4] * 1.1 + 3.0).contiguous()
    _load(g, loop_setup, image=brighter)
    g.refine()
    _load(eager, loop_setup, image=brighter)
    eager.refine()
    e2 = _photo_out(eager)
    for a, b in zip(_photo_out(g), e2):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(e2[1], e1[1])


def test_refiner_refusals(loop_setup):
    from types import SimpleNamespace

    from deepim.core.tester import Refiner

    cfg, scene, rm, pred, obs = loop_setup
    with pytest.raises(ValueError, match="TEST.PHOTO_ITER.*TEST.HYP_NUM"):
        _refiner(loop_setup, ITERS, HYP_NUM=2)
    with pytest.raises(ValueError, match="TEST.PHOTO_ITER.*TEST.COARSE_VIEWS"):
        _refiner(loop_setup, ITERS, COARSE_VIEWS=42)
    with pytest.raises(ValueError, match="TEST.PHOTO_LEVELS"):
        _refiner(loop_setup, ITERS, PHOTO_LEVELS=6)
    cfg.TEST.PHOTO_ITER = ITERS
    try:
        with pytest.raises(ValueError, match="TEST.PHOTO_ITER.*lit ModelNet renderer"):
            Refiner(cfg, pred, SimpleNamespace(normals=None, height=H, width=W), 2)
        scales = cfg.SCALES
        cfg.SCALES = [(540, 720)]
        try:
            with pytest.raises(ValueError, match="TEST.PHOTO_ITER.*SCALES"):
                Refiner(cfg, pred, rm, 2)
        finally:
            cfg.SCALES = scales
    finally:
        cfg.TEST.PHOTO_ITER = 0


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("device_eval", [False, True])
def test_pred_eval_synthetic_pairs_with_photo(hip_lib, device_eval):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs

    cfg = make_test_config(test_iter=2)
    cfg.TEST.DEVICE_EVAL = device_eval
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    B = 4
    data = SyntheticPairs(cfg, 8, B, subdiv=3)
    pred = Predictor(cfg, params, B)
    try:
        off = pred_eval(cfg, Refiner(cfg, pred, data.render_machine, B, capture_graph=True), data.test_batches(), data.evaluator())
        cfg.TEST.PHOTO_ITER = ITERS
        on = pred_eval(cfg, Refiner(cfg, pred, data.render_machine, B, capture_graph=True), data.test_batches(), data.evaluator())
        assert int(cfg.TEST.test_iter) == 2 and "photo" not in off
        for k in ("pose", "add", "arp_2d"):
            for row_on, row_off in zip(on[k]["overall"], off[k]["overall"]):
                assert row_on == row_off, k
        for k in ("all_rot_err", "all_trans_err"):
            assert on[k] == off[k]
        ph = on["photo"]
        assert set(ph) >= {"pose", "add", "arp_2d"} and len(ph["add"]["overall"]) == 1 and len(ph["pose"]["overall"]) == 1
        assert sum(len(ph["all_rot_err"][c][0]) for c in range(len(ph["all_rot_err"]))) == 8
        assert all(np.isfinite(r) for c in ph["all_rot_err"] for r in c[0])
    finally:
        from deepim.config.config import reset_config

        reset_config()
