"""Silhouette pose polish after the refinement loop on the device (csrc/sil.hip, dim_sil_edge_field and dim_sil_refine /
ops.sil_edge_field and ops.sil_refine): the kernels against the restatement tests/sil_reference.py on the hand-built masks and the
small frames of tests/test_sil_host.py (the field equal, the counts and status equal, the pose and the rms within the bars below),
the behaviour of the entry points, the full size on GPU renders, the Refiner stage inside the captured loop and pred_eval's
out["sil"] table.

Parity bars: the field equal; status and counts equal; pose_out within 1e-6 * max(1, |x|) and the rms column with rtol 1e-5
(tests/test_gpu_flow_pnp.py's and test_gpu_photo.py's, the arithmetic being the same: float64 per point, float32 outputs)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import sil_reference as sr  # noqa: E402
import test_sil_host as host  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402
from test_sil_host import GATE, GPU_ITERS, HUBER, RADIUS  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
FEW = sr.STATUS_SIL_FEW_POINTS
SIL_ITER, SIL_ROUNDS = 6, 2     # what the shipped test YAML sets


def ops():
    from lib.hip import ops as o

    return o


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def _refine(depth, field, pose_in, K, iters, bbox=None, Kps=None, huber=HUBER, gate=GATE):
    """one call on device tensors -> pose, stats, status (numpy)"""
    B = depth.shape[0]
    stats = torch.zeros((B, max(iters, 1), 2), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    # the workspace: exactly dim_sil_workspace_bytes between guards, at the documented minimum alignment (8 mod 16), full of NaN bits
    _, _, h, w = depth.shape
    work = guard_arena.workspace(ops().lib().dim_sil_workspace_bytes(B, h, w), 8, DEV)
    out = ops().sil_refine(depth, field, pose_in, K, iters, huber, gate, bbox=bbox, K_per_sample=Kps, stats=stats, status=status,
                           workspace=work.view())
    work.check("dim_sil_refine workspace, B = {}".format(B))
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()


def _batch(which):
    g = host.gpu_batches()[which]
    t = {k: _dev(g[k]) for k in ("depth_rendered", "mask", "pose_in", "K_per_sample")}
    t["bbox"] = _dev(g["bbox"], torch.int32)
    t["field"] = ops().sil_edge_field(t["mask"], RADIUS)
    return g, t


def _call(g, t, iters, with_bbox=True, per_sample=True):
    return _refine(t["depth_rendered"], t["field"], t["pose_in"], g["K"], iters, bbox=t["bbox"] if with_bbox else None,
                   Kps=t["K_per_sample"] if per_sample else None)


def _assert_pose(got, want, what):
    want = np.asarray(want, np.float64)
    bound = 1e-6 * np.maximum(1.0, np.abs(want))
    err = np.abs(np.asarray(got, np.float64) - want)
    print(what, "max pose error / bound", float((err / bound).max()))
    assert np.all(err <= bound), (what, float((err / bound).max()))


def _assert_matches(got, want, what):
    pose, stats, status = got
    r_pose, r_stats, r_status = want[:3]
    print(what, "counts", stats[:, :, 0].tolist(), "rms", np.round(stats[:, :, 1], 4).tolist(), "status", status.tolist())
    np.testing.assert_array_equal(status, r_status)
    np.testing.assert_array_equal(stats[:, :, 0], r_stats[:, :, 0])
    np.testing.assert_allclose(stats[:, :, 1], r_stats[:, :, 1], rtol=1e-5, atol=0)
    _assert_pose(pose, r_pose, what)


# ------------------------------------------------------------------------------------------------------------------ the field
@pytest.mark.parametrize("radius", host.FIELD_RADII)
@pytest.mark.parametrize("size", host.FIELD_SIZES)
def test_field_equals_restatement_on_hand_built_masks(hip_lib, size, radius):
    h, w = size
    masks = host.hand_masks(h, w)
    want = host.field_reference(h, w, radius)
    names = list(masks)
    for i in range(0, len(names), 3):
        trio = [names[(i + k) % len(names)] for k in range(3)]      # B = 3 in every call
        got = ops().sil_edge_field(_dev(np.stack([masks[n][None] for n in trio])), radius)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for k, n in enumerate(trio):
            assert np.array_equal(got[k], want[n]), (n, size, radius, int((got[k] != want[n]).sum()))


def _render(rm, poses, K=None):
    """-> depth (B,1,H,W), bbox (B,4), status: the stage's render"""
    B = poses.shape[0]
    depth = torch.zeros((B, 1, H, W), dtype=torch.float32, device=DEV)
    bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    extra = {"K": K} if K is not None else {}
    rm.render_batch(torch.zeros((B,), dtype=torch.int32, device=DEV), torch.as_tensor(poses).to(DEV), depth=depth, bbox=bbox, mask_thr=0.0,
                    status=status, **extra)
    return depth, bbox, status


@functools.lru_cache(maxsize=None)
def full_scene():
    """16 pairs at 480x640 on GPU renders of the models of tests/scene.py: the mask = the render at the ground truth, the depth and
    box = the render at the input pose; the device planes, their host copies, and the restatement's field and result, computed once"""
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn
    from test_icp_host import ICP_NOISE

    models = syn.make_models(seed=2333, n_models=1, subdiv=3)
    cls, gt, init = syn.sample_pairs(7, 16, **ICP_NOISE)
    rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
    d_gt, _, st_o = _render(rm, gt)
    depth, bbox, st_r = _render(rm, init)
    assert int(st_o.abs().sum()) == 0 and int(st_r.abs().sum()) == 0
    mask = (d_gt > 0).to(torch.float32).contiguous()
    torch.cuda.synchronize()
    mask_h, depth_h, bbox_h = mask.cpu().numpy(), depth.cpu().numpy(), bbox.cpu().numpy()
    field_h = sr.edge_field(mask_h, RADIUS)
    ref = sr.sil_refine(depth_h, field_h, init, rm.K, SIL_ITER, HUBER, GATE, bbox=bbox_h, with_extra=True)
    return {"rm": rm, "pts": models[0][0].astype(np.float64), "gt": gt, "init": init, "mask": mask, "depth": depth, "bbox": bbox,
            "field_ref": field_h, "ref": ref}


def test_field_equals_restatement_full_size(hip_lib):
    s = full_scene()
    got = ops().sil_edge_field(s["mask"], RADIUS)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (16, H, W) and int((s["field_ref"] >= 0).sum()) > 16 * 1000
    assert np.array_equal(got, s["field_ref"]), int((got != s["field_ref"]).sum())


# ------------------------------------------------------------------------------------------------------------------ the refinement
@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("iters", GPU_ITERS)
@pytest.mark.parametrize("which", [0, 1])
def test_hip_matches_restatement(hip_lib, which, iters, with_bbox):
    g, t = _batch(which)
    torch.cuda.synchronize()
    assert np.array_equal(t["field"].cpu().numpy(), g["field"])
    got = _call(g, t, iters, with_bbox)
    _assert_matches(got, host.gpu_reference(which, iters, with_bbox), (which, iters, with_bbox))
    if which == 0 and with_bbox:   # the small window: flagged, the input pose bit for bit
        assert got[2][2] == FEW and np.array_equal(got[0][2].view(np.uint32), g["pose_in"][2].view(np.uint32))


@pytest.mark.parametrize("which", [0, 1])
def test_host_K_without_per_sample_K(hip_lib, which):
    """pair 0's camera as the call's K9 for every pair, against the restatement given that one K"""
    g, t = _batch(which)
    got = _call(g, t, GPU_ITERS[-1], per_sample=False)
    _assert_matches(got, host.gpu_reference(which, GPU_ITERS[-1], True, False), (which, "host K"))
    with_K = _call(g, t, GPU_ITERS[-1])[0]
    assert np.array_equal(got[0][0], with_K[0]) and not np.array_equal(got[0][1], with_K[1])   # pair 0's camera is the same either way


@pytest.mark.parametrize("trigger", ["empty depth", "negative fx", "empty mask"])
def test_flagging_leaves_the_neighbours_alone(hip_lib, trigger):
    g, t = _batch(0)
    iters = GPU_ITERS[-1]
    base = _call(g, t, iters, with_bbox=False)
    assert base[2].tolist() == [0, 0, 0]
    t = dict(t)
    if trigger == "empty depth":
        t["depth_rendered"] = t["depth_rendered"].clone()
        t["depth_rendered"][1].zero_()
    elif trigger == "negative fx":
        t["K_per_sample"] = t["K_per_sample"].clone()
        t["K_per_sample"][1, 0] = -t["K_per_sample"][1, 0]
    else:
        mask = t["mask"].clone()
        mask[1].zero_()
        t["field"] = ops().sil_edge_field(mask, RADIUS)
        torch.cuda.synchronize()
        assert int((t["field"][1] != -1).sum()) == 0
    pose, stats, status = _call(g, t, iters, with_bbox=False)
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
    B, iters = g["pose_in"].shape[0], GPU_ITERS[-1]
    o = ops()
    work = o.sil_workspace(B, g["H"], g["W"], DEV)
    field = torch.zeros((B, g["H"], g["W"]), dtype=torch.int32, device=DEV)
    pose = torch.zeros((B, 3, 4), device=DEV)
    stats = torch.zeros((B, iters, 2), device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)

    def run():
        o.fill(status, 0)
        o.sil_edge_field(t["mask"], RADIUS, field=field)
        o.sil_refine(t["depth_rendered"], field, t["pose_in"], g["K"], iters, HUBER, GATE, bbox=t["bbox"], K_per_sample=t["K_per_sample"],
                     pose_out=pose, stats=stats, status=status, workspace=work)

    def read():
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (field, pose, stats, status)]

    run()
    eager = read()
    assert np.array_equal(eager[0], g["field"])
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
        field.zero_()
        pose.zero_()
        stats.zero_()
        work.zero_()
        graph.replay()
        for a, b in zip(read(), eager):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ full size
def test_full_size_16_pairs(hip_lib):
    """the device equals the restatement run on the same planes copied to the host; for every unflagged pair the last rms is below
    the first; ADD improves on every pair on which the restatement's does"""
    s = full_scene()
    field = ops().sil_edge_field(s["mask"], RADIUS)
    got = _refine(s["depth"], field, _dev(s["init"]), s["rm"].K, SIL_ITER, bbox=s["bbox"])
    _assert_matches(got, s["ref"], "full size")
    pose, stats, status = got
    add = lambda poses: np.array([sr.add_error(p, g, s["pts"]) for p, g in zip(poses, s["gt"])])  # noqa: E731
    before, after, after_ref = add(s["init"]), add(pose), add(s["ref"][0])
    print("ADD before (mm)", np.round(before * 1e3, 2), "after (mm)", np.round(after * 1e3, 2), "restatement (mm)", np.round(after_ref * 1e3, 2))
    print("least decision margins of the restatement", {k: min(e["margin"][k] for e in s["ref"][3]) for k in ("round", "huber", "gate")})
    print("rms first / last (px)", np.round(stats[:, 0, 1], 3), np.round(stats[:, -1, 1], 3), "contour points", [e["points"] for e in s["ref"][3]])
    assert int((status == 0).sum()) >= 8
    for b in range(16):
        if status[b] == 0:
            assert stats[b, -1, 1] < stats[b, 0, 1], (b, stats[b, :, 1])
        if after_ref[b] < before[b]:
            assert after[b] < before[b], (b, before[b], after[b])


# ------------------------------------------------------------------------------------------------------------------ the Refiner stage
def _cam(K, sx, sy, dx, dy):
    K = np.array(K, dtype=np.float32).copy()
    K[0, 0] *= sx
    K[1, 1] *= sy
    K[0, 2] += dx
    K[1, 2] += dy
    return K


def _setup(full_graph):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    cfg = make_test_config(test_iter=2)
    cfg.TEST.FAST_TEST = not full_graph
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1, rot_scale=1e-4, trans_scale=1e-4)   # a head that barely moves: the loop ends near the initial pose
    B = 2
    scene = make_scene(B=B, seed=2333, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    # the segmentation: the object a degree and a few millimetres from the initial pose
    rng = np.random.default_rng(9)
    at = np.stack([syn.perturb_pose(rng, p, angle_std=1.0, angle_max=3.0, xy_std=0.002, z_std=0.004) for p in scene["pose_init"]])
    mask = (_render(rm, torch.from_numpy(at))[0] > 0).to(torch.float32).contiguous()
    return cfg, scene, rm, pred, mask


@pytest.fixture(scope="module")
def loop_setup(hip_lib):
    yield _setup(False)
    from deepim.config.config import reset_config

    reset_config()


def _refiner(setup, sil_iter, graph=False, **keys):
    from deepim.core.tester import Refiner

    cfg, scene, rm, pred, mask = setup
    old = {k: cfg.TEST.get(k) for k in keys}
    cfg.TEST.SIL_ITER = sil_iter
    cfg.TEST.update(keys)
    try:
        return Refiner(cfg, pred, rm, 2, capture_graph=graph)
    finally:
        cfg.TEST.SIL_ITER = 0
        cfg.TEST.update(old)


def _load(ref, setup, K=None, mask=None):
    bl = setup[1]["blobs"]
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    args[2] = setup[4] if mask is None else mask
    ref.load(*args, K=K)


def _loop_out(ref):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (ref.poses_iter, ref.se3_iter, ref.status_iter)]


def _sil_out(ref):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (ref.pose_sil, ref.sil_stats, ref.status_sil)]


def _standalone(cfg, rm, mask, last, Kd, rounds=SIL_ROUNDS, iters=SIL_ITER):
    """the stage by hand: the field once, then render and refine per round -> pose, stats (B, rounds*iters, 2), status"""
    o = ops()
    field = o.sil_edge_field(mask, int(np.ceil(cfg.TEST.SIL_MAX_PX)))
    status = torch.zeros((2,), dtype=torch.int32, device=DEV)
    pose, stats = last, []
    for _ in range(rounds):
        depth, bbox, st = _render(rm, pose, K=Kd)
        status |= st
        stats.append(torch.zeros((2, iters, 2), dtype=torch.float32, device=DEV))
        pose = o.sil_refine(depth, field, pose, rm.K, iters, cfg.TEST.SIL_HUBER_PX, cfg.TEST.SIL_MAX_PX, bbox=bbox, K_per_sample=Kd,
                            stats=stats[-1], status=status)
    torch.cuda.synchronize()
    return pose.cpu().numpy(), torch.cat(stats, dim=1).cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("graph", [False, True])
def test_refiner_sil_leaves_the_loop_alone(loop_setup, graph):
    off = _refiner(loop_setup, 0, graph)
    assert "sil" not in off.stages and off.pose_sil is None and off.sil_stats is None and off.status_sil is None
    assert not hasattr(off, "mask_sil") and not hasattr(off, "field_sil") and not hasattr(off, "depth_sil")
    _load(off, loop_setup)
    off.refine()
    want = _loop_out(off)
    on = _refiner(loop_setup, SIL_ITER, graph)
    _load(on, loop_setup)
    on.refine()
    for a, b in zip(want, _loop_out(on)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    pose, stats, status = _sil_out(on)
    print("counts", stats[:, :, 0].tolist(), "rms", np.round(stats[:, :, 1], 3).tolist())
    assert stats.shape == (2, SIL_ROUNDS * SIL_ITER, 2) and status.tolist() == [0, 0] and stats[:, :, 0].min() >= sr.MIN_POINTS
    assert np.abs(pose - want[0][-1]).max() > 1e-5   # the stage did move the pose
    assert np.all(stats[:, -1, 1] < stats[:, 0, 1])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("per_pair_K", [False, True])
def test_refiner_sil_equals_standalone(loop_setup, per_pair_K, graph):
    cfg, scene, rm, pred, mask = loop_setup
    K = np.stack([_cam(rm.K, 1.05, 1.05, 6.0, -4.0), _cam(rm.K, 0.95, 0.97, -5.0, 3.0)]) if per_pair_K else None
    ref = _refiner(loop_setup, SIL_ITER, graph)
    _load(ref, loop_setup, K=K)
    ref.refine()
    if graph:
        assert ref.graph is not None
        ref.refine()    # a replay
    got = _sil_out(ref)
    last = ref.poses_iter[-1].clone()
    Kd = torch.from_numpy(K.reshape(2, 9)).to(DEV) if per_pair_K else None
    want = _standalone(cfg, rm, mask, last, Kd)
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    # the stage reads its own copy of the loaded segmentation, not the box the loop has written over mask_observed since
    assert np.array_equal(ref.mask_sil.cpu().numpy(), mask.cpu().numpy())
    assert not np.array_equal(ref.batch["mask_observed"].cpu().numpy(), mask.cpu().numpy())


def test_refiner_sil_graph_takes_a_new_mask(loop_setup):
    g = _refiner(loop_setup, SIL_ITER, graph=True)
    _load(g, loop_setup)
    g.refine()
    first = _sil_out(g)
    shifted = torch.roll(loop_setup[4], shifts=2, dims=3).contiguous()    # the segmentation two pixels to the right
    _load(g, loop_setup, mask=shifted)
    g.refine()
    eager = _refiner(loop_setup, SIL_ITER, graph=False)
    _load(eager, loop_setup, mask=shifted)
    eager.refine()
    for a, b in zip(_sil_out(g), _sil_out(eager)):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(_sil_out(g)[0], first[0])


def test_refiner_sil_mask_pred_on_the_full_graph(loop_setup):
    """(after loop_setup, whose config object this one shares: FAST_TEST is put back at the end)"""
    full_graph_setup = _setup(True)
    try:
        _mask_pred_on_the_full_graph(full_graph_setup)
    finally:
        full_graph_setup[0].TEST.FAST_TEST = True


def _mask_pred_on_the_full_graph(full_graph_setup):
    cfg, scene, rm, pred, mask = full_graph_setup
    ref = _refiner(full_graph_setup, SIL_ITER, SIL_MASK="pred")
    assert not hasattr(ref, "mask_sil") and ref.mask_pred_iter is not None
    bl = scene["blobs"]
    ref.load(*[bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
    ref.refine()
    got = _sil_out(ref)
    want = _standalone(cfg, rm, ref.mask_pred_iter[-1].clone(), ref.poses_iter[-1].clone(), None)
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    off = _refiner(full_graph_setup, 0)
    off.load(*[bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
    off.refine()
    for a, b in zip(_loop_out(off), _loop_out(ref)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refiner_refusals(loop_setup):
    from types import SimpleNamespace

    from deepim.core.tester import Refiner

    cfg, scene, rm, pred, mask = loop_setup
    with pytest.raises(ValueError, match="TEST.SIL_ITER.*TEST.HYP_NUM"):
        _refiner(loop_setup, SIL_ITER, HYP_NUM=2)
    with pytest.raises(ValueError, match="TEST.SIL_ITER.*TEST.COARSE_VIEWS"):
        _refiner(loop_setup, SIL_ITER, COARSE_VIEWS=42)
    with pytest.raises(ValueError, match="TEST.SIL_ROUNDS"):
        _refiner(loop_setup, SIL_ITER, SIL_ROUNDS=9)
    with pytest.raises(ValueError, match="TEST.SIL_ITER.*TEST.SIL_MASK"):
        _refiner(loop_setup, SIL_ITER, SIL_MASK="pred")       # the FAST_TEST graph has no mask head
    ref = _refiner(loop_setup, SIL_ITER)
    bl = scene["blobs"]
    with pytest.raises(ValueError, match="TEST.SIL_ITER"):
        ref.load(bl["image_observed"], bl["image_rendered"], None, bl["mask_rendered"], bl["src_pose"], bl["class_index"])
    cfg.TEST.SIL_ITER = SIL_ITER
    try:
        with pytest.raises(ValueError, match="TEST.SIL_ITER.*lit ModelNet renderer"):
            Refiner(cfg, pred, SimpleNamespace(normals=None, height=H, width=W), 2)
        scales = cfg.SCALES
        cfg.SCALES = [(540, 720)]
        try:
            with pytest.raises(ValueError, match="TEST.SIL_ITER.*SCALES"):
                Refiner(cfg, pred, rm, 2)
        finally:
            cfg.SCALES = scales
    finally:
        cfg.TEST.SIL_ITER = 0


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("device_eval", [False, True])
def test_pred_eval_synthetic_pairs_with_sil(hip_lib, device_eval):
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
        cfg.TEST.SIL_ITER = SIL_ITER
        on = pred_eval(cfg, Refiner(cfg, pred, data.render_machine, B, capture_graph=True), data.test_batches(), data.evaluator())
        assert int(cfg.TEST.test_iter) == 2 and "sil" not in off
        for k in ("pose", "add", "arp_2d"):
            for row_on, row_off in zip(on[k]["overall"], off[k]["overall"]):
                assert row_on == row_off, k
        for k in ("all_rot_err", "all_trans_err"):
            assert on[k] == off[k]
        sl = on["sil"]
        assert set(sl) >= {"pose", "add", "arp_2d"} and len(sl["add"]["overall"]) == 1 and len(sl["pose"]["overall"]) == 1
        assert sum(len(sl["all_rot_err"][c][0]) for c in range(len(sl["all_rot_err"]))) == 8
        assert all(np.isfinite(r) for c in sl["all_rot_err"] for r in c[0])
    finally:
        from deepim.config.config import reset_config

        reset_config()
