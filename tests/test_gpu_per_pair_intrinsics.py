"""Per-pair camera intrinsics in the test-time loop (reference deepim/core/tester.py:165, :560-562: each pair is re-rendered with its
own -K.txt when the dataset ships one; ZoomMask and the flow error keep the config K).  dim_raster_render_k / Render_Py.render_batch
with a (B,3,3) K, Refiner.load(K=...), dim_refiner_run_k, and TestDataLoader's "K" blob."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flownet as oflow, native, se3 as ose3  # noqa: E402
from oracle.refine import image_transform, update_mask_observed_box_rendered  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402
from loop_parity import check_loop, moving_head  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640


def _cam(K, sx, sy, dx, dy):
    K = np.array(K, dtype=np.float32).copy()
    K[0, 0] *= sx
    K[1, 1] *= sy
    K[0, 2] += dx
    K[1, 2] += dy
    return K


def _four_cameras():
    from lib.utils import synthetic as syn

    return np.stack([_cam(syn.LINEMOD_K, 1.2, 1.2, 30.0, -20.0), syn.LINEMOD_K, _cam(syn.LINEMOD_K, 0.8, 0.8, -25.0, 35.0),
                     _cam(syn.LINEMOD_K, 1.1, 0.9, 15.0, 12.0)])


def _poses():
    """four poses in view; the last one puts the near plane (0.25 m) through the middle of the 0.2 m object"""
    from lib.utils import synthetic as syn

    cls, gt, init = syn.sample_pairs(4, 4, n_classes=2)
    init = init.astype(np.float32).copy()
    init[3, :, 3] = [0.0, 0.0, 0.27]
    return cls.astype(np.int32), init


def _outputs(B, aligned):
    """image / depth / mask / bgr planes; aligned=False shifts every plane by one float, which forces the one-thread-per-pixel resolve"""
    def plane(*shape):
        n = int(np.prod(shape))
        if aligned:
            return torch.zeros(shape, dtype=torch.float32, device=DEV)
        return torch.zeros((n + 1,), dtype=torch.float32, device=DEV)[1:].view(*shape)

    return {"image": plane(B, 3, H, W), "depth": plane(B, 1, H, W), "mask": plane(B, 1, H, W), "bgr": plane(B, H, W, 3),
            "bbox": torch.zeros((B, 4), dtype=torch.int32, device=DEV), "status": torch.zeros((B,), dtype=torch.int32, device=DEV)}


@pytest.fixture(scope="module")
def machines(hip_lib):
    from lib.render_hip.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi, vertex_normals
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    models = syn.make_models(seed=3, n_models=2, subdiv=3)
    out = {}
    for bil in (False, True):
        out[(False, bil)] = Render_Py(None, ["a", "b"], syn.LINEMOD_K, meshes=models, tex_bilinear=bil)
        lit_meshes = [(v, vertex_normals(v, f), t, f) for v, t, f, tex in models]
        out[(True, bil)] = Render_Py_Light_ModelNet_Multi(None, models[0][3], syn.LINEMOD_K, meshes=lit_meshes, tex_bilinear=bil)
    return models, out


def _render(rm, lit, cls, poses, K, o, pm, clean_bbox=None, bbox=None):
    kw = {}
    if lit:   # fixed lights: the same for the batch and for the solo render of one sample
        B = poses.shape[0]
        kw["light_position"] = torch.tensor(np.tile([[0.3, -0.2, 0.1]], (B, 1)), dtype=torch.float32, device=DEV)
        kw["light_intensity"] = torch.tensor(np.tile([[1.0, 0.95, 1.05]], (B, 1)), dtype=torch.float32, device=DEV)
    rm.render_batch(cls, poses, K=K, image=o["image"], depth=o["depth"], mask=o["mask"], bgr=o["bgr"], bbox=o["bbox"] if bbox is None else bbox,
                    plane_means=pm, mask_thr=0.2, status=o["status"], clean_bbox=clean_bbox, **kw)


def _solo(rm, lit, cls, poses, Ks, b, aligned, pm):
    o = _outputs(1, aligned)
    _render(rm, lit, cls[b:b + 1], poses[b:b + 1], Ks[b], o, pm)
    return o


def _assert_sample_equal(o, b, solo, tag):
    for k in ("image", "depth", "mask", "bgr", "bbox", "status"):
        assert torch.equal(o[k][b], solo[k][0]), (tag, b, k)


# ------------------------------------------------------------------------------------------------------------------ the rasteriser
@pytest.mark.parametrize("lit", [False, True])
@pytest.mark.parametrize("bil", [False, True])
@pytest.mark.parametrize("aligned", [True, False])
def test_mixed_batch_equals_solo_renders(machines, lit, bil, aligned):
    from lib.utils import synthetic as syn

    models, rms = machines
    rm = rms[(lit, bil)]
    Ks = _four_cameras()
    cls_np, poses_np = _poses()
    cls, poses = torch.from_numpy(cls_np).to(DEV), torch.from_numpy(poses_np).to(DEV)
    pm = syn.plane_means()
    o = _outputs(4, aligned)
    _render(rm, lit, cls, poses, Ks, o, pm)                         # host (B,3,3)
    o2 = _outputs(4, aligned)
    _render(rm, lit, cls, poses, torch.from_numpy(Ks.reshape(4, 9)).to(DEV), o2, pm)   # device (B,9)
    torch.cuda.synchronize()
    for k in o:
        assert torch.equal(o[k], o2[k]), k
    assert int(o["status"].abs().sum()) == 0
    for b in range(4):
        assert float(o["mask"][b].sum()) > 500, b    # every sample is in view
        _assert_sample_equal(o, b, _solo(rm, lit, cls, poses, Ks, b, aligned, pm), "lit={} bil={} aligned={}".format(lit, bil, aligned))
    # the cameras do matter: sample 0 rendered with the config K is another picture
    other = _outputs(1, aligned)
    _render(rm, lit, cls[:1], poses[:1], syn.LINEMOD_K, other, pm)
    assert not torch.equal(other["mask"][0], o["mask"][0])


@pytest.mark.parametrize("lit", [False, True])
def test_dirty_box_render_with_per_sample_K(machines, lit):
    """the loop's 2nd render: the planes hold the previous render, clean_bbox names its box"""
    from lib.utils import synthetic as syn

    models, rms = machines
    rm = rms[(lit, False)]
    Ks = _four_cameras()
    cls_np, poses_np = _poses()
    cls = torch.from_numpy(cls_np).to(DEV)
    moved = poses_np.copy()
    moved[:, 0, 3] += 0.012
    moved[:, 1, 3] -= 0.007
    pm = syn.plane_means()
    o = _outputs(4, True)
    bb_prev = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    _render(rm, lit, cls, torch.from_numpy(poses_np).to(DEV), Ks, o, pm, bbox=bb_prev)
    _render(rm, lit, cls, torch.from_numpy(moved).to(DEV), Ks, o, pm, clean_bbox=bb_prev)
    poses2 = torch.from_numpy(moved).to(DEV)
    for b in range(4):
        _assert_sample_equal(o, b, _solo(rm, lit, cls, poses2, Ks, b, True, pm), "dirty lit={}".format(lit))


def test_per_sample_K_vs_oracle(machines):
    """one sample of a mixed batch against oracle.native.render with that sample's K (bars of test_gpu_ops.test_rasteriser_vs_oracle)"""
    from lib.utils import synthetic as syn

    models, rms = machines
    rm = rms[(False, False)]
    Ks = _four_cameras()
    cls_np, poses_np = _poses()
    o = _outputs(4, True)
    _render(rm, False, torch.from_numpy(cls_np).to(DEV), torch.from_numpy(poses_np).to(DEV), Ks, o, syn.plane_means())
    for b in (0, 2):
        v, t, f, tex = models[cls_np[b]]
        rb, rd = native.render(v, t, f, tex, poses_np[b][:, :3], poses_np[b][:, 3], Ks[b])
        gd = o["depth"][b, 0].cpu().numpy()
        assert ((gd > 0) != (rd > 0)).sum() <= 4
        both = (gd > 0) & (rd > 0)
        assert both.sum() > 500
        np.testing.assert_allclose(gd[both], rd[both], rtol=2e-6)
        gb = o["bgr"][b].cpu().numpy()
        assert ((np.abs(gb - rb).max(axis=-1) > 0.0) & both).sum() <= 8
        ys, xs = np.nonzero(gd > 0.2)
        assert o["bbox"][b].tolist() == [xs.min(), xs.max(), ys.min(), ys.max()]


@pytest.mark.parametrize("aligned", [True, False])
def test_bad_K_renders_background_and_flags(machines, aligned):
    from lib.hip import ops
    from lib.utils import synthetic as syn

    models, rms = machines
    rm = rms[(False, False)]
    Ks = _four_cameras()
    Ks[1, 0, 0] = 0.0
    Ks[2, 0, 0] = np.nan
    cls_np, poses_np = _poses()
    cls, poses = torch.from_numpy(cls_np).to(DEV), torch.from_numpy(poses_np).to(DEV)
    pm = syn.plane_means()
    o = _outputs(4, aligned)
    _render(rm, False, cls, poses, Ks, o, pm)
    torch.cuda.synchronize()
    assert o["status"].tolist() == [0, ops.STATUS_BAD_K, ops.STATUS_BAD_K, 0]
    for b in (1, 2):
        assert float(o["depth"][b].abs().sum()) == 0 and float(o["mask"][b].sum()) == 0 and float(o["bgr"][b].abs().sum()) == 0
        for c in range(3):
            assert bool((o["image"][b, c] == -float(pm[c])).all())
        assert o["bbox"][b].tolist() == [W, -1, H, -1]
    for b in (0, 3):
        _assert_sample_equal(o, b, _solo(rm, False, cls, poses, Ks, b, aligned, pm), "bad-K neighbour")


def test_wrong_K_shape_raises_before_launch(machines):
    models, rms = machines
    cls_np, poses_np = _poses()
    o = _outputs(4, True)
    o["status"].fill_(7)
    for lit in (False, True):
        with pytest.raises(ValueError):
            _render(rms[(lit, False)], lit, torch.from_numpy(cls_np).to(DEV), torch.from_numpy(poses_np).to(DEV), np.zeros((3, 3, 3)), o, None)
    torch.cuda.synchronize()
    assert o["status"].tolist() == [7, 7, 7, 7]


# ------------------------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def loop_setup(hip_lib):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.render_hip.render_py_multi import Render_Py

    cfg = make_test_config(test_iter=4)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1)
    B = 2
    scene = make_scene(B=B, seed=2333, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    K_cfg = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32)
    K_pairs = np.stack([_cam(K_cfg, 1.15, 1.12, 18.0, -10.0), _cam(K_cfg, 0.85, 0.88, -14.0, 16.0)])
    return cfg, params, scene, rm, pred, K_pairs


def _refine(setup, K=None, graph=False, K_then=None):
    """-> (poses_iter, se3_iter, status_iter) as numpy.  K_then: load that K after a first refine and replay (graph re-use)."""
    from deepim.core.tester import Refiner

    cfg, params, scene, rm, pred, _ = setup
    bl = scene["blobs"]
    ref = Refiner(cfg, pred, rm, 2, capture_graph=graph)
    args = [bl[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    ref.load(*args, K=K)
    ref.refine()
    if K_then is not None:
        ref.load(*args, K=K_then)
        ref.refine()
    return ref.poses_iter.cpu().numpy().copy(), ref.se3_iter.cpu().numpy().copy(), ref.status_iter.cpu().numpy().copy()


def _forced_oracle(params, mesh, blobs_b, K_cfg, K_b, pixel_means, poses_hip_b, test_iter):
    """oracle.refine.refine_pair's teacher-forced loop, restated with the reference's two cameras: the network (zoom) sees the config K,
    the re-render the pair's K (tester.py:560-562).  -> (poses, se3s)"""
    verts, uvs, faces, tex = mesh
    batch = {k: np.array(v, dtype=np.float32) for k, v in blobs_b.items()}
    pose_rendered = np.array(batch["src_pose"][0], dtype=np.float64)
    out = oflow.forward_test(params, batch, K_cfg, pixel_means, fast_test=True)
    poses, se3s = [], []
    for it in range(test_iter):
        se3 = np.squeeze(out["se3"]).astype("float32")
        se3s.append(se3)
        poses.append(ose3.RT_transform(pose_rendered, se3[:-3], se3[-3:], np.zeros(3), np.ones(3), "CAMERA"))
        pose_new = np.array(poses_hip_b[it], dtype=np.float64)
        if it < test_iter - 1:
            bgr, depth = native.render(verts, uvs, faces, tex, pose_new[:3, :3], pose_new[:, 3], K_b)
            mask_r = (depth > 0.2).astype(np.float64)
            batch["image_rendered"] = image_transform(bgr.astype("uint8").astype(np.float64), pixel_means).astype(np.float32)
            batch["mask_rendered"] = mask_r[np.newaxis, np.newaxis].astype(np.float32)
            batch["mask_observed"] = update_mask_observed_box_rendered(mask_r)[np.newaxis, np.newaxis].astype(np.float32)
            batch["src_pose"] = pose_new[np.newaxis].astype(np.float32)
            pose_rendered = pose_new
            out = oflow.forward_test(params, batch, K_cfg, pixel_means, fast_test=True)
    return poses, se3s


def _check_vs_oracle(setup, poses, se3, test_iter=4, verbose=True):
    cfg, params, scene, rm, pred, K_pairs = setup
    bl = scene["blobs"]
    pts = scene["models"][0][0].astype(np.float64)
    diam = np.linalg.norm(pts.max(0) - pts.min(0))
    for b in range(2):
        blobs_b = {k: bl[k][b:b + 1] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose")}
        forced = _forced_oracle(params, scene["models"][int(bl["class_index"][b])], blobs_b, cfg.dataset.INTRINSIC_MATRIX, K_pairs[b],
                                cfg.network.PIXEL_MEANS, poses[:test_iter, b], test_iter)
        # free = forced: the free-running loop is only reported by check_loop; the step bar is on the teacher-forced one
        check_loop(bl["src_pose"][b], poses[:test_iter, b], se3[:test_iter, b], forced, forced, pts, diam, tag="per-pair K pair {}".format(b),
                   step_tol=2e-5, verbose=verbose, min_rot_deg=0.0, min_trans_m=0.0, mean_rot_deg=0.0)


@pytest.mark.parametrize("graph", [False, True])
def test_loop_with_uniform_per_pair_K_is_bit_identical(loop_setup, graph):
    cfg = loop_setup[0]
    K_cfg = np.tile(np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32)[None], (2, 1, 1))
    base = _refine(loop_setup, K=None, graph=graph)
    same = _refine(loop_setup, K=K_cfg, graph=graph)
    for a, b in zip(base, same):
        np.testing.assert_array_equal(a, b)


def test_loop_with_distinct_K_vs_oracle(loop_setup):
    poses, se3, status = _refine(loop_setup, K=loop_setup[5])
    assert int(np.abs(status).sum()) == 0
    _check_vs_oracle(loop_setup, poses, se3)
    # the cameras move the result: iteration 0 is the same forward, the later ones differ measurably from the config-K loop
    base = _refine(loop_setup, K=None)[0]
    np.testing.assert_array_equal(poses[0], base[0])
    assert np.abs(poses[1:] - base[1:]).max() > 1e-3


def test_loop_check_bites_when_the_K_buffer_holds_the_config_K(loop_setup, monkeypatch):
    """negative control: a loop that loads the per-pair K but renders with the config K fails the oracle check from iteration 1 on"""
    from deepim.core.tester import Refiner

    cfg = loop_setup[0]
    K_cfg = np.tile(np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(1, 9), (2, 1))
    real = Refiner._load_K

    def load_config_K(self, K):
        real(self, K)
        self.K_pair.copy_(torch.from_numpy(K_cfg))

    monkeypatch.setattr(Refiner, "_load_K", load_config_K)
    poses, se3, _ = _refine(loop_setup, K=loop_setup[5])
    monkeypatch.undo()
    with pytest.raises(AssertionError):
        _check_vs_oracle(loop_setup, poses, se3, test_iter=2, verbose=False)


def test_graph_replay_picks_up_newly_loaded_K(loop_setup):
    K_a = loop_setup[5]
    K_b = K_a[::-1].copy()
    replayed = _refine(loop_setup, K=K_a, graph=True, K_then=K_b)
    eager = _refine(loop_setup, K=K_b, graph=False)
    for a, b in zip(replayed, eager):
        np.testing.assert_array_equal(a, b)
    assert np.abs(replayed[0] - _refine(loop_setup, K=K_a)[0]).max() > 1e-3


def test_c_resident_loop_with_per_pair_K_matches_python(loop_setup):
    from lib.hip.refiner_capi import CRefiner

    cfg, params, scene, rm, pred, K_pairs = loop_setup
    bl = scene["blobs"]
    dev = [torch.as_tensor(np.ascontiguousarray(bl[k])).to(DEV)
           for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")]
    cref = CRefiner(cfg, params, rm, 2)
    poses_c = cref.refine(*dev, K_per_pair=torch.from_numpy(K_pairs.reshape(2, 9)).to(DEV)).cpu().numpy().copy()
    se3_c = cref.se3_iter.cpu().numpy().copy()
    poses, se3, _ = _refine(loop_setup, K=K_pairs)
    np.testing.assert_array_equal(poses_c, poses)
    np.testing.assert_array_equal(se3_c, se3)
    poses_plain = cref.refine(*dev).cpu().numpy()   # NULL: the desc's K9
    np.testing.assert_array_equal(poses_plain, _refine(loop_setup, K=None)[0])
    cref.close()


# ------------------------------------------------------------------------------------------------------------------ files end to end
def test_loader_K_blob_and_pred_eval(hip_lib, tmp_path):
    import pickle

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
    root = str(tmp_path)
    db = _write_pairs(root, 4)
    K_cfg = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32)
    Ka, Kb = _cam(K_cfg, 1.1, 1.1, 12.0, -8.0), _cam(K_cfg, 0.9, 0.92, -10.0, 6.0)
    for i, K in ((1, Ka), (3, Kb)):
        path = db[i]["image_observed"][:-10] + "-K.txt"
        assert path == os.path.join(root, "{:03d}-K.txt".format(i))
        np.savetxt(path, K)
    want = np.stack([K_cfg, Ka, Ka, Kb])   # pair 2 has no file: it keeps pair 1's camera
    B = 2
    loader = TestDataLoader(db, cfg, batch_size=B, device=DEV, workers=2)
    batches = []
    for k, batch in enumerate(loader):
        np.testing.assert_array_equal(batch["K"].cpu().numpy(), want[k * B:(k + 1) * B])
        batches.append({n: v.clone() for n, v in batch.items()})
    loader.close()
    # no file anywhere: no "K" blob
    plain = TestDataLoader(_write_pairs(os.path.join(root, "plain"), 2), cfg, batch_size=B, device=DEV, workers=2)
    assert "K" not in plain.next()
    plain.close()

    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    moving_head(params, seed=1)
    models = syn.make_models(seed=2333, n_models=3, subdiv=3)
    rm = Render_Py(None, cfg.dataset.class_name, K_cfg, meshes=models)
    ref = Refiner(cfg, Predictor(cfg, params, B), rm, B, capture_graph=True)
    pts = {c: models[i][0].astype(np.float64) for i, c in enumerate(cfg.dataset.class_name)}
    diam = {c: float(np.linalg.norm(p.max(0) - p.min(0))) for c, p in pts.items()}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, diam)
    f = str(tmp_path / "results.pkl")
    loader = TestDataLoader(db, cfg, batch_size=B, device=DEV, workers=2)
    pred_eval(cfg, ref, loader, ev, result_file=f)
    loader.close()
    with open(f, "rb") as fh:
        est = pickle.load(fh)[2]
    names = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")
    explicit, without = [], []
    for k, bt in enumerate(batches):
        ref.load(*[bt[n] for n in names], K=want[k * B:(k + 1) * B])
        explicit.append(ref.refine().cpu().numpy().astype(np.float64).copy())
        ref.load(*[bt[n] for n in names])
        without.append(ref.refine().cpu().numpy().astype(np.float64).copy())
    order = {}
    for k, bt in enumerate(batches):
        for j, c in enumerate(bt["class_index"].cpu().numpy()):
            order.setdefault(int(c), []).append((k, j))
    moved = 0.0
    for c, slots in order.items():
        for it in range(2):
            for n, (k, j) in enumerate(slots):
                np.testing.assert_array_equal(est[c][it][n], explicit[k][it, j])
                moved = max(moved, float(np.abs(explicit[k][it, j] - without[k][it, j]).max()))
    assert moved > 0.0   # the per-pair cameras reached the loop
