"""The refinement loop from camera images of another size than the 480x640 network input (config.SCALES = [[540, 720]], K the camera of
that image): every image-like buffer, the renders, the boxes and the zoom window at the source size; X and the encoder at 480x640.

The oracle step is assembled here from UNCHANGED oracle pieces -- oracle.zoom.zoom_factor_from_valid at the source size,
_grid_from_factor at 480x640, bilinear_sampler, oracle.flownet.network_input / encoder and the heads, zoom_trans, oracle.se3.RT_transform,
oracle.native.render(..., H=540, W=720) -- teacher-forced with the HIP poses and checked by tests/loop_parity.check_loop with that
function's own default bars."""
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flownet as oflow, native, se3 as ose3, zoom as ozoom  # noqa: E402
from oracle.refine import image_transform, update_mask_observed_box_rendered  # noqa: E402
from scene import make_test_config  # noqa: E402
from loop_parity import check_loop, moving_head  # noqa: E402
import source_size_reference as R  # noqa: E402

DEV = "cuda:0"
HS, WS, HN, WN = 540, 720, 480, 640
SCALE = HS / float(HN)          # 1.125
B, T = 2, 2
BLOBS = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
f32 = np.float32


def source_K():
    from lib.utils import synthetic as syn

    K = np.array(syn.LINEMOD_K, np.float64) * SCALE
    K[2, 2] = 1.0
    return K.astype(f32)


def source_config(test_iter=T):
    cfg = make_test_config(test_iter=test_iter)
    cfg.SCALES = [(HS, WS)]
    cfg.dataset.INTRINSIC_MATRIX = source_K()
    return cfg


def make_source_scene(seed=2333, subdiv=3):
    """tests/scene.py make_scene with the frame of the source camera: the same models and draws, rendered by the CPU oracle at 540x720"""
    from lib.utils import synthetic as syn

    K = source_K()
    models = syn.make_models(seed=seed, n_models=1, subdiv=subdiv)
    cls, gt, init = syn.sample_pairs(seed + 1, B, n_classes=1, frame=(K, WS, HS))
    rng = np.random.default_rng(seed + 2)
    io, ir, mo, mr, dobs, dren = [], [], [], [], [], []
    for b in range(B):
        v, t, f, tex = models[cls[b]]
        bgr_gt, d_gt = native.render(v, t, f, tex, gt[b][:, :3], gt[b][:, 3], K, H=HS, W=WS)
        obs = syn.compose_observed(bgr_gt, d_gt, rng)
        bgr_r, d_r = native.render(v, t, f, tex, init[b][:, :3], init[b][:, 3], K, H=HS, W=WS)
        assert obs.shape == (HS, WS, 3)
        io.append(syn.bgr_to_blob(obs))
        ir.append(syn.bgr_to_blob(bgr_r.astype(np.uint8)))
        m_r = (d_r > 0.2).astype(f32)
        mr.append(m_r[None, None])
        mo.append(syn.box_from_mask(m_r)[None, None])
        dobs.append(np.where(d_gt > 0, d_gt, 1.5).astype(f32)[None, None])
        dren.append(d_r.astype(f32)[None, None])
    blobs = {"image_observed": np.concatenate(io).astype(f32), "image_rendered": np.concatenate(ir).astype(f32),
             "mask_observed": np.concatenate(mo).astype(f32), "mask_rendered": np.concatenate(mr).astype(f32),
             "src_pose": init.astype(f32), "class_index": cls, "depth_observed": np.concatenate(dobs), "depth_rendered": np.concatenate(dren)}
    return {"models": models, "K": K, "blobs": blobs, "pose_gt": gt}


def oracle_forward(params, batch, K, pixel_means, window_size=(HS, WS)):
    """one forward from source-size blobs: the window at `window_size` (the source size; the negative control passes 480x640), the
    grid at 480x640, the unchanged sampler, Concat, encoder, heads and inverse ZoomTrans"""
    mo, mr = np.asarray(batch["mask_observed"], f32), np.asarray(batch["mask_rendered"], f32)
    mr_bin = np.where(mr > 0.2, f32(1), f32(0)).astype(f32)
    zf, _ = ozoom.zoom_factor_from_valid(np.sum(mo, axis=1) > 0.3, np.sum(mr_bin, axis=1) > 0.3, batch["src_pose"], K, *window_size)
    grid = ozoom._grid_from_factor(zf, HN, WN)
    pm = np.asarray(pixel_means, f32).reshape(3)[::-1].reshape(1, 3, 1, 1)
    zio = (ozoom.bilinear_sampler(np.asarray(batch["image_observed"], f32) + pm, grid) - pm).astype(f32)
    zir = (ozoom.bilinear_sampler(np.asarray(batch["image_rendered"], f32) + pm, grid) - pm).astype(f32)
    zmo, zmr = ozoom.mx_round(ozoom.bilinear_sampler(mo, grid)), ozoom.mx_round(ozoom.bilinear_sampler(mr_bin, grid))
    data = oflow.network_input(zio, zir, zmo, zmr)
    assert data.shape[2:] == (HN, WN)
    with torch.no_grad():
        fc7 = oflow.encoder(params, torch.from_numpy(data))
        rot = torch.nn.functional.linear(fc7, oflow._t(params, "rot_weight", torch.float32), oflow._t(params, "rot_bias", torch.float32))
        tz = torch.nn.functional.linear(fc7, oflow._t(params, "trans_weight", torch.float32), oflow._t(params, "trans_bias", torch.float32))
    trans = ozoom.zoom_trans(zf, tz.numpy(), b_inv_zoom=True)
    return np.concatenate([rot.numpy(), trans], axis=1).astype(f32)[0]


def oracle_loop(params, mesh, blobs_b, K, pixel_means, forced_poses=None, window_size=(HS, WS), update_mask="box_rendered", K_render=None):
    """oracle.refine.refine_pair's loop on source-size blobs (one pair): -> (poses, se3s)"""
    verts, uvs, faces, tex = mesh
    z3, o3 = np.zeros(3), np.ones(3)
    batch = {k: np.array(v, dtype=f32) for k, v in blobs_b.items()}
    pose_rendered = np.array(batch["src_pose"][0], dtype=np.float64)
    poses, se3s = [], []
    for it in range(T):
        se3 = oracle_forward(params, batch, K, pixel_means, window_size)
        se3s.append(se3)
        pose_new = ose3.RT_transform(pose_rendered, se3[:-3], se3[-3:], z3, o3, "CAMERA")
        poses.append(pose_new)
        if forced_poses is not None:
            pose_new = np.array(forced_poses[it], dtype=np.float64)
        if it < T - 1:
            bgr, depth = native.render(verts, uvs, faces, tex, pose_new[:3, :3], pose_new[:, 3], K if K_render is None else K_render, H=HS, W=WS)
            mask_r = np.zeros(depth.shape)
            mask_r[depth > 0.2] = 1
            batch["image_rendered"] = image_transform(bgr.astype("uint8").astype(np.float64), pixel_means).astype(f32)
            batch["mask_rendered"] = mask_r[None, None].astype(f32)
            if update_mask == "box_rendered":
                batch["mask_observed"] = update_mask_observed_box_rendered(mask_r)[None, None].astype(f32)
            batch["src_pose"] = pose_new[None].astype(f32)
            pose_rendered = pose_new
    return poses, se3s


@pytest.fixture(scope="module")
def setup(hip_lib):
    assert torch.cuda.is_available()
    from deepim.config.config import reset_config
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.render_hip.render_py_multi import Render_Py

    cfg = source_config()
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
    scene = make_source_scene()
    pred = Predictor(cfg, params, B)
    assert (pred.net.Hs, pred.net.Ws, pred.net.H, pred.net.W) == (HS, WS, HN, WN) and tuple(pred.net.X.shape) == (B, HN, WN, 8)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], width=WS, height=HS, meshes=scene["models"])
    pts = scene["models"][0][0].astype(np.float64)
    st = {"cfg": cfg, "params": params, "scene": scene, "pred": pred, "rm": rm, "pts": pts, "diam": float(np.linalg.norm(pts.max(0) - pts.min(0))),
          "free": {}}
    yield st
    reset_config()


def _pair_blobs(scene, b):
    return {k: scene["blobs"][k][b:b + 1] for k in BLOBS[:5]}


def _free(st, b):
    """the free-running oracle loop of pair b, computed once"""
    if b not in st["free"]:
        st["free"][b] = oracle_loop(st["params"], st["scene"]["models"][0], _pair_blobs(st["scene"], b), st["scene"]["K"], st["cfg"].network.PIXEL_MEANS)
    return st["free"][b]


def _run(st, graph=False, K=None, cfg=None):
    from deepim.core.tester import Refiner

    bl = st["scene"]["blobs"]
    ref = Refiner(cfg or st["cfg"], st["pred"], st["rm"], B, capture_graph=graph)
    for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered"):
        assert tuple(ref.batch[k].shape[2:]) == (HS, WS), k
    ref.load(*[bl[k] for k in BLOBS], K=K)
    poses = ref.refine().cpu().numpy().copy()
    return ref, poses, ref.se3_iter.cpu().numpy().copy()


@pytest.fixture(scope="module")
def eager(setup):
    ref, poses, se3 = _run(setup)
    assert int(ref.status_iter.abs().sum()) == 0
    return poses, se3


def test_step_parity_with_the_oracle_pieces(setup, eager):
    st, (poses, se3) = setup, eager
    bl = st["scene"]["blobs"]
    for b in range(B):
        forced = oracle_loop(st["params"], st["scene"]["models"][0], _pair_blobs(st["scene"], b), st["scene"]["K"], st["cfg"].network.PIXEL_MEANS,
                             forced_poses=poses[:, b])
        check_loop(bl["src_pose"][b], poses[:, b], se3[:, b], _free(st, b), forced, st["pts"], st["diam"], tag="540x720 pair {}".format(b))


def test_negative_control_window_at_the_network_size(setup, monkeypatch):
    """the bars must go RED when the loop finds the zoom window at 480x640 instead of the source size (the fault is injected from
    outside: ops.zoom_factor is replaced by one that ignores the size it is given); same scene, same checks, eager mode"""
    from lib.hip import ops

    st = setup
    real = ops.zoom_factor
    monkeypatch.setattr(ops, "zoom_factor", lambda bo, br, pose, K, H, W, **kw: real(bo, br, pose, K, HN, WN, **kw))
    _, poses, se3 = _run(st)
    monkeypatch.undo()
    bl, red = st["scene"]["blobs"], 0
    for b in range(B):
        forced = oracle_loop(st["params"], st["scene"]["models"][0], _pair_blobs(st["scene"], b), st["scene"]["K"], st["cfg"].network.PIXEL_MEANS,
                             forced_poses=poses[:, b])
        try:
            check_loop(bl["src_pose"][b], poses[:, b], se3[:, b], _free(st, b), forced, st["pts"], st["diam"], tag="window at 480x640, pair {}".format(b))
        except AssertionError as e:
            red += 1
            print("pair {}: red as required: {}".format(b, str(e)[:200]))
    assert red == B, "the loop checks did not notice a window computed at the network size"


def test_graph_capture_gives_the_same_bits(setup, eager):
    ref, poses, se3 = _run(setup, graph=True)
    assert ref.graph is not None
    np.testing.assert_array_equal(poses, eager[0])
    np.testing.assert_array_equal(se3, eager[1])
    np.testing.assert_array_equal(ref.refine().cpu().numpy(), eager[0])      # a replay


def test_c_refiner_gives_the_same_bits_and_leaves_its_inputs(setup, eager):
    """dim_refiner_create_src: bit-equal poses_iter / se3_iter to the Python Refiner (tests/test_gpu_refiner_capi.py asserts this at
    480x640); the six input blobs are read, never written; the same-size create functions keep refusing another size"""
    import ctypes

    from lib.hip import capi
    from lib.hip.refiner_capi import CRefiner, RefinerDesc

    st = setup
    bl = st["scene"]["blobs"]
    dev = {k: torch.as_tensor(np.ascontiguousarray(bl[k])).to(DEV) for k in BLOBS}
    keep = {k: v.clone() for k, v in dev.items()}
    cref = CRefiner(st["cfg"], st["params"], st["rm"], B)
    poses_c = cref.refine(*[dev[k] for k in BLOBS]).cpu().numpy().copy()
    np.testing.assert_array_equal(poses_c, eager[0])
    np.testing.assert_array_equal(cref.se3_iter.cpu().numpy(), eager[1])
    assert int(cref.status_iter.abs().sum()) == 0
    for k in dev:
        assert torch.equal(dev[k], keep[k]), k
    cref.close()
    d = RefinerDesc()
    d.B, d.H, d.W, d.test_iter, d.n_classes = B, HS, WS, T, 1
    names, ptrs, h = (ctypes.c_char_p * 1)(b"x"), (ctypes.c_void_p * 1)(None), ctypes.c_void_p()
    assert capi.lib().dim_refiner_create_cls(ctypes.byref(h), ctypes.byref(d), 1, names, ptrs, 0, None) != 0
    assert b"480 x 640" in capi.lib().dim_last_error()
    d.W = WS + 4
    assert capi.lib().dim_refiner_create_src(ctypes.byref(h), ctypes.byref(d), 1, names, ptrs, 0, None) != 0
    assert b"4:3" in capi.lib().dim_last_error()


def test_update_mask_init(setup):
    """UPDATE_MASK 'init': mask_observed stays the loaded one; the step parity of pair 0 against the oracle loop that does the same"""
    st = setup
    cfg = st["cfg"]
    cfg.TEST.UPDATE_MASK = "init"
    try:
        ref, poses, se3 = _run(st)
        np.testing.assert_array_equal(ref.batch["mask_observed"].cpu().numpy(), st["scene"]["blobs"]["mask_observed"])
    finally:
        cfg.TEST.UPDATE_MASK = "box_rendered"
    args = (st["params"], st["scene"]["models"][0], _pair_blobs(st["scene"], 0), st["scene"]["K"], cfg.network.PIXEL_MEANS)
    free = oracle_loop(*args, update_mask="init")
    forced = oracle_loop(*args, update_mask="init", forced_poses=poses[:, 0])
    check_loop(st["scene"]["blobs"]["src_pose"][0], poses[:, 0], se3[:, 0], free, forced, st["pts"], st["diam"], tag="UPDATE_MASK init")


def test_per_pair_K(setup, eager):
    """a camera per pair: the re-render uses it, the zoom window keeps the config K (as at 480x640); pair 0 against the oracle loop that
    renders with that camera, and the uniform run is not what comes out"""
    st = setup
    K0 = np.asarray(st["scene"]["K"], np.float64)
    Ks = np.stack([K0 * np.array([[1.0 + 0.04 * (j + 1), 1, 1], [1, 1.0 + 0.04 * (j + 1), 1], [1, 1, 1]]) for j in range(B)]).astype(f32)
    ref, poses, se3 = _run(st, K=Ks)
    assert ref.per_pair_K and not np.array_equal(poses[1], eager[0][1])
    np.testing.assert_array_equal(poses[0], eager[0][0])            # the first iteration sees the loaded blobs only
    args = (st["params"], st["scene"]["models"][0], _pair_blobs(st["scene"], 0), st["scene"]["K"], st["cfg"].network.PIXEL_MEANS)
    free = oracle_loop(*args, K_render=Ks[0])
    forced = oracle_loop(*args, K_render=Ks[0], forced_poses=poses[:, 0])
    check_loop(st["scene"]["blobs"]["src_pose"][0], poses[:, 0], se3[:, 0], free, forced, st["pts"], st["diam"], tag="per-pair K")


@pytest.mark.parametrize("input_mask,input_depth,mode", [(False, False, 1), (False, True, 2), (True, True, 3)])
def test_the_other_input_graphs(setup, input_mask, input_depth, mode):
    """the other first-layer arities (no masks: the ZoomImage window; INPUT_DEPTH without and with masks) from source-size blobs: X
    (and X2) equal the restatement's lanes for the window the device found, and a two-iteration loop runs and re-renders its planes
    (the depth plane too) at the source size"""
    from deepim.core.tester import Predictor, Refiner
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    st = setup
    cfg, bl = st["cfg"], st["scene"]["blobs"]
    cfg.network.INPUT_MASK, cfg.network.PRED_MASK, cfg.network.INPUT_DEPTH = input_mask, input_mask, input_depth
    try:
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
        pred = Predictor(cfg, params, B)
        assert pred.net.input_mode == mode
        batch = {k: torch.as_tensor(np.ascontiguousarray(v)).to(DEV) for k, v in bl.items()}
        pred.net.forward_test(batch)
        zf = pred.net.zoom_factor.cpu().numpy()
        means = pred.net.plane_means
        if mode == 1:
            pm = means.reshape(1, 3, 1, 1)
            valid = lambda im: np.sum(im + pm, axis=1) > 0.01  # noqa: E731
            want_zf, _ = ozoom.zoom_factor_from_valid(valid(bl["image_observed"]), valid(bl["image_rendered"]), bl["src_pose"], st["scene"]["K"], HS, WS)
            np.testing.assert_allclose(zf, want_zf, rtol=2e-6, atol=2e-6)
            want = R.net_input_src(bl["image_observed"], bl["image_rendered"], None, None, zf, means, 1, HN, WN)["X"]
        else:
            want = R.net_input_src(bl["image_observed"], bl["image_rendered"], bl["depth_observed"], bl["depth_rendered"], zf, means, 2, HN, WN)["X"]
        np.testing.assert_array_equal(pred.net.X.cpu().numpy(), want)
        if mode == 3:
            want2 = R.net_input_src(bl["image_observed"], bl["image_rendered"], bl["mask_observed"], bl["mask_rendered"], zf, means, 3, HN, WN)["X"]
            np.testing.assert_array_equal(pred.net.X2.cpu().numpy(), want2)
        ref = Refiner(cfg, pred, st["rm"], B, capture_graph=True)
        ref.load(*[bl[k] for k in BLOBS], depth_observed=bl["depth_observed"] if input_depth else None,
                 depth_rendered=bl["depth_rendered"] if input_depth else None)
        poses = ref.refine().cpu().numpy()
        assert np.isfinite(poses).all() and int(ref.status_iter.abs().sum()) == 0
        assert not np.array_equal(ref.batch["image_rendered"].cpu().numpy(), bl["image_rendered"])
        if input_depth:
            d = ref.batch["depth_rendered"].cpu().numpy()
            assert d.shape == (B, 1, HS, WS) and not np.array_equal(d, bl["depth_rendered"]) and (d > 0.2).any()
    finally:
        cfg.network.INPUT_MASK, cfg.network.PRED_MASK, cfg.network.INPUT_DEPTH = True, True, False


def test_device_eval_and_bop_without_the_vsd_grid(setup):
    """TEST.DEVICE_EVAL and TEST.BOP (pose-only kernels, the source camera from the config) through pred_eval on synthetic 540x720
    pairs: the tables of the plain run, the device errors behind them, finite BOP errors for every pose"""
    from deepim.core.tester import Refiner, pred_eval
    from lib.dataset.synthetic_pairs import SyntheticPairs

    st = setup
    cfg = st["cfg"]
    data = SyntheticPairs(cfg, 2 * B, B, seed=2333, subdiv=3)
    assert (data.render_machine.height, data.render_machine.width) == (HS, WS)
    batches = list(data.test_batches())
    assert tuple(batches[0]["image_observed"].shape) == (B, 3, HS, WS)
    ref = Refiner(cfg, st["pred"], data.render_machine, B)
    plain = pred_eval(cfg, ref, batches, data.evaluator())
    cfg.TEST.DEVICE_EVAL, cfg.TEST.BOP, cfg.TEST.BOP_SYM_STEP = True, True, 0.2
    try:
        on = pred_eval(cfg, ref, batches, data.evaluator())
    finally:
        cfg.TEST.DEVICE_EVAL, cfg.TEST.BOP, cfg.TEST.BOP_SYM_STEP = False, False, 0.01
    assert on["device_eval"] is True and "bop" in on and "bop" not in plain
    for c in range(len(plain["all_rot_err"])):
        for it in range(T):
            np.testing.assert_allclose(on["all_rot_err"][c][it], plain["all_rot_err"][c][it], rtol=0, atol=0)
            assert len(on["bop"]["errors"]["mssd"][c][it]) == 2 * B
            assert np.isfinite(on["bop"]["errors"]["mssd"][c][it]).all() and np.isfinite(on["bop"]["errors"]["mspd"][c][it]).all()
    # the refinement moves the synthetic pairs' poses somewhere finite and the reprojection errors are in source pixels
    assert max(on["bop"]["errors"]["mspd"][0][0]) > 0


@pytest.mark.parametrize("key,value", [("ICP_ITER", 2), ("HYP_NUM", 2), ("COARSE_VIEWS", 8), ("VSD", True), ("BOP_VSD", True), ("FLOW_PNP_ITER", 2)])
def test_stages_of_the_network_size_raise_at_construction(setup, key, value):
    from deepim.core.tester import Refiner

    st = setup
    cfg = st["cfg"]
    old = cfg.TEST.get(key)
    cfg.TEST[key] = value
    try:
        with pytest.raises(ValueError, match="TEST.{}.*SCALES".format(key)):
            Refiner(cfg, st["pred"], st["rm"], B)
    finally:
        cfg.TEST[key] = old
    Refiner(cfg, st["pred"], st["rm"], B)


def test_full_graph_flow_error_and_lit_renderer_raise(setup):
    from deepim.core.tester import FlowEPE, Predictor, Refiner
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    st = setup
    cfg = st["cfg"]

    class Lit(object):
        normals = None
        height, width = HS, WS

    with pytest.raises(ValueError, match="lit ModelNet renderer.*SCALES"):
        Refiner(cfg, st["pred"], Lit(), B)
    cfg.TEST.FAST_TEST = False
    try:
        with pytest.raises(ValueError, match="PRED_FLOW.*FAST_TEST.*SCALES"):
            Refiner(cfg, st["pred"], st["rm"], B)
        with pytest.raises(ValueError, match="SCALES"):
            FlowEPE(cfg, B, DEV)
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        with pytest.raises(ValueError, match="TEST.FAST_TEST.*SCALES"):
            Predictor(cfg, sym.init_weights(cfg, {}, {}, seed=0), 1)
    finally:
        cfg.TEST.FAST_TEST = True
    # a render machine or a network of another size than SCALES is refused too
    from lib.render_hip.render_py_multi import Render_Py

    with pytest.raises(ValueError, match="render machine"):
        Refiner(cfg, st["pred"], Render_Py(None, cfg.dataset.class_name, st["scene"]["K"], meshes=st["scene"]["models"]), B)


def test_pred_eval_through_the_test_entry_point(hip_lib, tmp_path):
    """deepim/test.py with a 540x720 config of the new style (SCALES and the camera of that image; otherwise the shipped ape test
    config with a small batch) on synthetic pairs, as a child process: it runs and fills the score lists"""
    with open(os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test_960x1280.yaml")) as f:
        text = f.read()
    K = source_K().reshape(-1)
    for old, new in (("- 960\n- 1280\n", "- {}\n- {}\n".format(HS, WS)), ("BATCH_PAIRS: 16\n  test_epoch", "BATCH_PAIRS: 2\n  test_epoch"),
                     ("test_iter: 4", "test_iter: 2")):
        assert old in text, old
        text = text.replace(old, new)
    lines = [("  INTRINSIC_MATRIX: [{}]".format(", ".join(repr(float(v)) for v in K)) if ln.startswith("  INTRINSIC_MATRIX:") else ln)
             for ln in text.split("\n")]
    cfg_file = str(tmp_path / "ape_540x720.yaml")
    with open(cfg_file, "w") as f:
        f.write("\n".join(lines))
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(PKG, "deepim", "test.py"), "--cfg", cfg_file, "--gpus", "0", "--num_pairs", "4"],
                       cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "evaluating pose" in r.stdout and "refined 4 pairs x 2 iterations" in r.stdout
    files = glob.glob(os.path.join(str(tmp_path), "output", "deepim_hip", "*", "synthetic_val_ape", "*_results.pkl"))
    assert len(files) == 1, files
    rot_err, trans_err, poses_est, poses_gt = pickle.load(open(files[0], "rb"))
    assert len(poses_est[0][1]) == 4 and len(poses_gt[0][0]) == 4 and len(rot_err[0][1]) == 4
    assert np.isfinite(np.asarray(poses_est[0][1], np.float64)).all()
