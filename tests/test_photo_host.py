"""CPU: the photometric pose polish after the refinement loop -- the restatement (tests/photo_reference.py) converges on seeded
synthetic pairs whose observed image has another gain and bias, its controls (no gain fit, a gate below the noise), the pyramid
rules, the new TEST keys and their refusals, the host side of the C ABI (dim_photo_workspace_bytes, argument checks before any
device call), the out["photo"] table of pred_eval with a fake refiner on CPU tensors, and gpu_batches(): the small-frame inputs
tests/test_gpu_photo.py compares the kernels on, proven sound here.

Convergence bars (set from the restatement, 16 pairs of ICP_NOISE, 3 levels x 4 iterations, Huber 30, gate 180): N = 15 pairs end with
ADD <= 2 mm, the worst of them at 1.31 mm; pair 15 starts at 18.3 mm and ends at 13.0 mm.  Asserted: N >= 14 and no pair above 1.25 x
its starting ADD.  The rms of an iteration is compared within one pyramid level only: a finer level sees the pixel noise the coarser
one has averaged away, so the last rms (level 0) of a pair that starts almost converged lies above its first (level 2)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import photo_reference as pr
from conftest import ROOT
from test_icp_host import icp_pairs

LEVELS, ITERS, HUBER, GATE = 3, 4, 30.0, 180.0     # the config defaults (PHOTO_ITER: what the test YAML sets)
ADD_OK = 2e-3
HEADER = os.path.join(ROOT, "include", "deepim_hip.h")


def observed_recipe(image, depth, seed, plane_means):
    """the observed blob of a render blob (3,H,W) at the ground truth: the render over a seeded uniform-noise background, then
    another gain and bias, round(0.8 I + 20) on the 0..255 values"""
    pm = np.asarray(plane_means, np.float32).reshape(3, 1, 1)
    vals = np.clip(np.round(np.asarray(image, np.float32) + pm), 0, 255)
    bg = np.random.default_rng(seed).integers(0, 256, size=vals.shape).astype(np.float32)
    o = np.where(np.asarray(depth).reshape(1, *vals.shape[1:]) > 0, vals, bg)
    return (np.round(0.8 * o + 20.0) - pm).astype(np.float32)


@functools.lru_cache(maxsize=None)
def full_scene(n=16):
    """-> pts, K, gt, init, image_observed, image_rendered, depth_rendered of icp_pairs(n), rendered by the oracle"""
    from lib.utils import synthetic as syn
    from oracle import native

    models, cls, gt, init = icp_pairs(n)
    v, t, f, tex = models[0]
    K, pm = syn.LINEMOD_K, syn.plane_means()
    obs, ren, dep = [], [], []
    for b in range(n):
        bgr, d = native.render(v, t, f, tex, gt[b][:, :3], gt[b][:, 3], K)
        obs.append(observed_recipe(syn.bgr_to_blob(bgr)[0], d, 100 + b, pm))
        bgr, d = native.render(v, t, f, tex, init[b][:, :3], init[b][:, 3], K)
        ren.append(syn.bgr_to_blob(bgr)[0])
        dep.append(d[None])
    return v.astype(np.float64), K, gt, init, np.stack(obs), np.stack(ren), np.stack(dep)


@functools.lru_cache(maxsize=None)
def full_result(gain=True):
    pts, K, gt, init, obs, ren, dep = full_scene()
    return pr.photo_refine(obs, ren, dep, init, K, LEVELS, ITERS, HUBER, GATE, gain=gain)


def add_errors(poses, gt, pts):
    return np.array([pr.add_error(p, g, pts) for p, g in zip(poses, gt)])


def check_convergence(before, after, n_min):
    """the bars of the issue: at least n_min pairs end with ADD <= 2 mm and none ends above 1.25 x its starting ADD"""
    n = int(np.sum(after <= ADD_OK))
    print("ADD before (mm)", np.round(before * 1e3, 2), "after (mm)", np.round(after * 1e3, 2), "N", n)
    assert n >= n_min, (n, after)
    assert np.all(after <= 1.25 * before), (before, after)
    return n


def restatement_N():
    """N of the committed restatement, the number the GPU test's bar is taken from"""
    pts, K, gt, init = full_scene()[:4]
    return int(np.sum(add_errors(full_result()[0], gt, pts) <= ADD_OK))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_converges():
    pts, K, gt, init = full_scene()[:4]
    pose, stats, status = full_result()
    before, after = add_errors(init, gt, pts), add_errors(pose, gt, pts)
    assert before.min() > ADD_OK    # every input is off by more than the bar
    n = check_convergence(before, after, 14)
    print("N", n, "worst converged (mm)", 1e3 * after[after <= ADD_OK].max())
    lv0 = (LEVELS - 1) * ITERS     # the first iteration of level 0
    for b in np.nonzero(after <= ADD_OK)[0]:
        assert status[b] == 0, b
        assert stats[b, ITERS - 1, 1] < stats[b, 0, 1], (b, stats[b, :, 1])   # the level the polish starts at: its rms falls
    assert stats[:, -1, 1].mean() < stats[:, 0, 1].mean() and stats[:, -1, 1].mean() < stats[:, lv0, 1].mean()


def test_gain_control():
    """without the gain and bias fit the brightness difference is read as a residual: a larger final rms on every pair and a worse pose
    on average over the pairs that converge with the fit"""
    pts, K, gt, init = full_scene()[:4]
    pose1, stats1, _ = full_result(True)
    pose0, stats0, _ = full_result(False)
    a1, a0 = add_errors(pose1, gt, pts), add_errors(pose0, gt, pts)
    ok = a1 <= ADD_OK
    print("ADD with gain (mm)", np.round(a1 * 1e3, 2), "without (mm)", np.round(a0 * 1e3, 2))
    assert np.all(stats0[:, -1, 1] > stats1[:, -1, 1])
    assert a0[ok].mean() > a1[ok].mean()
    assert int(np.sum(a0[ok] > a1[ok])) >= int(ok.sum()) - 2


def test_negative_control_gate_below_the_noise():
    pts, K, gt, init, obs, ren, dep = full_scene()
    one = slice(0, 1)
    pose, stats, status = pr.photo_refine(obs[one], ren[one], dep[one], init[one], K, LEVELS, ITERS, 1e-3, 1e-3)
    assert status.tolist() == [pr.STATUS_PHOTO_FEW_POINTS]
    assert np.array_equal(pose.view(np.uint32), init[one].view(np.uint32))
    assert stats[0, :, 0].max() < pr.MIN_POINTS
    moved = full_result()[0][0]
    assert full_result()[2][0] == 0 and pr.add_error(moved, gt[0], pts) < ADD_OK < pr.add_error(init[0], gt[0], pts)


def test_pyramid_sizes_and_dropped_row_and_column():
    assert pr.level_sizes(37, 50, 3) == [(37, 50), (18, 25), (9, 12)]
    rng = np.random.default_rng(3)
    p = rng.normal(0, 100, (37, 50)).astype(np.float32)
    lv = pr.pyramid(p, 3)
    assert [x.shape for x in lv] == [(37, 50), (18, 25), (9, 12)] and all(x.dtype == np.float32 for x in lv)
    q = p.copy()
    q[36, :] = 1e6     # the leftover row of level 0
    q1 = pr.half(q)
    np.testing.assert_array_equal(q1, lv[1])
    q1[:, 24] = -1e6   # the leftover column of level 1
    np.testing.assert_array_equal(pr.half(q1), lv[2])
    a, b, c, d = p[0, 0], p[0, 1], p[1, 0], p[1, 1]
    assert lv[1][0, 0] == np.float32(np.float32(np.float32(a + b) + np.float32(c + d)) * np.float32(0.25))
    v = np.ones((37, 50), bool)
    v[5, 7] = False
    v1 = pr.half_valid(v)
    assert v1.shape == (18, 25) and not v1[2, 3] and int(v1.sum()) == 18 * 25 - 1
    assert int(pr.half_valid(v1).sum()) == 9 * 12 - 1


def test_bbox_restricts_the_template():
    pts, K, gt, init, obs, ren, dep = full_scene()
    d = dep[0, 0]
    ys, xs = np.nonzero(d > 0)
    tight = [xs.min(), xs.max(), ys.min(), ys.max()]
    np.testing.assert_array_equal(pr.template_valid(d), pr.template_valid(d, tight))
    np.testing.assert_array_equal(pr.template_valid(d), pr.template_valid(d, [-7, 900, -2, 480]))   # clamped like clamp_bbox
    assert int(pr.template_valid(d, [640, -1, 480, -1]).sum()) == 0                                 # the render's empty box
    half = pr.template_valid(d, [xs.min(), (xs.min() + xs.max()) // 2, ys.min(), ys.max()])
    assert 0 < int(half.sum()) < int((d > 0).sum())
    pl = pr.planes(obs[0], ren[0], d, [xs.min(), (xs.min() + xs.max()) // 2, ys.min(), ys.max()], 2)
    assert int(pl["valid"][1].sum()) < int(pr.planes(obs[0], ren[0], d, tight, 2)["valid"][1].sum())
    assert pr.gain_sums(pl)[0] == half.sum()


# ------------------------------------------------------------------------------------------------------------------ config
def test_config_defaults_and_yaml_merge(tmp_path):
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    T = config.TEST
    assert (T.PHOTO_ITER, T.PHOTO_LEVELS, T.PHOTO_HUBER, T.PHOTO_MAX, T.PHOTO_GAIN) == (0, 3, 30.0, 180.0, True)
    p = tmp_path / "photo.yaml"
    p.write_text("TEST:\n  PHOTO_ITER: 5\n  PHOTO_LEVELS: 2\n  PHOTO_MAX: 120.0\n  PHOTO_GAIN: False\n  test_iter: 4\n")
    update_config(str(p))
    assert (T.PHOTO_ITER, T.PHOTO_LEVELS, T.PHOTO_HUBER, T.PHOTO_MAX, T.PHOTO_GAIN, T.test_iter) == (5, 2, 30.0, 120.0, False, 4)
    reset_config()
    assert config.TEST.PHOTO_ITER == 0


def test_shipped_yamls():
    from deepim.config.config import config, reset_config, update_config
    from deepim.core.tester import photo_settings

    cfgs = os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs")
    reset_config()
    update_config(os.path.join(cfgs, "deepim_hip_LM_ape_test.yaml"))
    assert config.TEST.PHOTO_ITER == 0 and photo_settings(config)[0] == 0
    base = {k: v for k, v in config.TEST.items() if not k.startswith("PHOTO_")}
    reset_config()
    update_config(os.path.join(cfgs, "deepim_hip_LM_ape_test_photo.yaml"))
    assert photo_settings(config) == (4, 3, 30.0, 180.0, True)
    assert {k: v for k, v in config.TEST.items() if not k.startswith("PHOTO_")} == base   # the ape test config plus the new keys
    reset_config()


def test_photo_settings_refusals():
    from deepim.config.config import config, reset_config
    from deepim.core.tester import photo_settings, refuse_at_source_size

    reset_config()
    assert photo_settings(config) == (0, 3, 30.0, 180.0, True)
    bad = {"PHOTO_ITER": [-1, 2.5, True], "PHOTO_LEVELS": [0, 6, 1.5, True], "PHOTO_HUBER": [0.0, -1.0, float("nan"), float("inf")],
           "PHOTO_MAX": [29.0, float("nan"), float("inf")], "PHOTO_GAIN": [1, "yes", None]}
    for key, values in bad.items():
        for v in values:
            reset_config()
            config.TEST[key] = v
            with pytest.raises(ValueError, match="TEST." + key):
                photo_settings(config)
    for key, v in (("HYP_NUM", 4), ("COARSE_VIEWS", 42)):
        reset_config()
        config.TEST[key] = v
        assert photo_settings(config)[0] == 0           # fine while the stage is off
        config.TEST.PHOTO_ITER = 4
        with pytest.raises(ValueError, match="TEST." + key):
            photo_settings(config)
    reset_config()
    config.TEST.PHOTO_ITER = 4
    assert photo_settings(config) == (4, 3, 30.0, 180.0, True)
    refuse_at_source_size(config, (480, 640))
    with pytest.raises(ValueError, match="TEST.PHOTO_ITER"):
        refuse_at_source_size(config, (960, 1280))
    reset_config()


# ------------------------------------------------------------------------------------------------------------------ C ABI, host side
def test_header_defines_the_status_bit():
    text = open(HEADER).read()
    assert "#define DIM_STATUS_PHOTO_FEW_POINTS 1024" in text
    assert pr.STATUS_PHOTO_FEW_POINTS == 1024
    from lib.hip import ops

    assert ops.STATUS_PHOTO_FEW_POINTS == 1024


def _plane_bytes(B, H, W, levels):
    return 4 * sum(4 * ((B * h * w + 3) // 4) * 4 for h, w in pr.level_sizes(H, W, levels))


def test_workspace_bytes(hip_lib):
    gn = (16 + 16 * 32) * 8     # T_delta state + 16 workgroup partials of 32 doubles, as the ICP's
    for B, H, W, levels in ((1, 480, 640, 3), (16, 480, 640, 3), (3, 48, 64, 2), (2, 37, 50, 2), (2, 37, 50, 1), (1, 48, 48, 5)):
        assert hip_lib.dim_photo_workspace_bytes(B, H, W, levels) == B * (gn + 8 * 8) + _plane_bytes(B, H, W, levels), (B, H, W, levels)
        assert hip_lib.dim_photo_workspace_offset(B, H, W, levels, 4, 0) == B * gn
        assert hip_lib.dim_photo_workspace_offset(B, H, W, levels, 0, 0) == B * (gn + 64)
        assert hip_lib.dim_photo_workspace_offset(B, H, W, levels, 3, levels - 1) % 16 == 0
        assert hip_lib.dim_photo_workspace_offset(B, H, W, levels, 0, levels) == -1
    # refused shapes: no bytes
    for B, H, W, levels in ((0, 480, 640, 3), (2, 480, 640, 0), (2, 480, 640, 6), (2, 11, 64, 3), (2, 48, 5, 2)):
        assert hip_lib.dim_photo_workspace_bytes(B, H, W, levels) == 0, (B, H, W, levels)


def test_bad_arguments_return_err_arg_without_a_device(hip_lib):
    K9 = (ctypes.c_float * 9)(572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is enqueued

    def call(B=2, H=480, W=640, levels=3, iters=4, huber=30.0, gate=180.0, io=fake, ir=fake, dr=fake, pose=fake, k9=K9, ws=fake, out=fake):
        return hip_lib.dim_photo_refine(io, ir, dr, None, pose, k9, None, B, H, W, levels, iters, huber, gate, 1, ws, out, None, None, None)

    cases = {"B=0": dict(B=0), "B<0": dict(B=-3), "levels=0": dict(levels=0), "levels=6": dict(levels=6), "iters<0": dict(iters=-1),
             "huber=0": dict(huber=0.0), "huber<0": dict(huber=-1.0), "huber=nan": dict(huber=float("nan")),
             "gate<huber": dict(gate=29.0), "gate=nan": dict(gate=float("nan")), "coarsest 2 rows": dict(H=11),
             "coarsest 2 columns": dict(W=11), "coarsest 2x2 at 5 levels": dict(H=47, W=47, levels=5),
             "image_observed": dict(io=None), "image_rendered": dict(ir=None), "depth_rendered": dict(dr=None), "pose_in": dict(pose=None),
             "K9": dict(k9=None), "workspace": dict(ws=None), "pose_out": dict(out=None)}
    for name, kw in cases.items():
        assert call(**kw) == -1, name
        assert hip_lib.dim_last_error().decode().startswith("photo_refine"), name


# ------------------------------------------------------------------------------------------------------------------ pred_eval
class _FakeNet(object):
    device = "cpu"


class _FakeRefiner(object):
    """stands in for deepim.core.tester.Refiner: fixed poses per batch on CPU tensors"""

    def __init__(self, B, poses_iter, poses_photo, photo):
        self.B, self.net = B, _FakeNet()
        self._poses, self._photo = list(poses_iter), list(poses_photo)
        self.photo = photo
        self.pose_photo = None

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None):
        self.pose_photo = torch.from_numpy(self._photo.pop(0)) if self.photo else None
        self._cur = torch.from_numpy(self._poses.pop(0))

    def refine(self):
        return self._cur


def _fake_run(photo, n_batches=2, B=4, test_iter=3, **test_keys):
    from deepim.core.tester import pred_eval
    from lib.dataset.evaluation import PoseEvaluator
    from lib.utils import synthetic as syn
    from scene import make_test_config

    cfg = make_test_config(test_iter=test_iter)
    cfg.dataset.class_name = ["ape", "cat"]
    cfg.TEST.PHOTO_ITER = 4 if photo else 0
    cfg.TEST.update(test_keys)
    rng = np.random.default_rng(5)
    pts = {c: rng.uniform(-0.05, 0.05, size=(200, 3)) for c in cfg.dataset.class_name}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, {c: 0.15 for c in cfg.dataset.class_name})
    batches, iters, polished = [], [], []
    for k in range(n_batches):
        cls, gt, init = syn.sample_pairs(100 + k, B, n_classes=2)
        init = init.copy()
        if k == 1:
            init[2] = -1.0   # undetected
        iters.append(np.stack([gt + rng.normal(0, 0.02 / (it + 1), gt.shape).astype(np.float32) for it in range(test_iter)]).astype(np.float32))
        polished.append((gt + rng.normal(0, 0.001, gt.shape)).astype(np.float32))
        z = torch.zeros((B, 1, 4, 4))
        batches.append({"image_observed": z, "image_rendered": z, "mask_observed": z, "mask_rendered": z, "src_pose": torch.from_numpy(init),
                        "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt)})
    out = pred_eval(cfg, _FakeRefiner(B, iters, polished, photo), batches, ev)
    return cfg, out


def test_pred_eval_scores_photo_as_one_row_table():
    from test_icp_host import _same

    _, off = _fake_run(False)
    assert "photo" not in off
    cfg, on = _fake_run(True)
    assert int(cfg.TEST.test_iter) == 3   # the one-row scoring does not touch the config
    _same({k: v for k, v in on.items() if k != "photo"}, off)
    ph = on["photo"]
    assert set(ph) >= {"pose", "add", "arp_2d"}
    assert ph["pose"]["rot_acc"].shape == (2, 1, 10) and len(ph["pose"]["overall"]) == 1
    assert len(ph["add"]["overall"]) == 1 and len(ph["arp_2d"]["overall"]) == 1
    rot = [r for c in range(2) for r in ph["all_rot_err"][c][0]]
    assert len(rot) == 8 and sorted(rot)[-1] == 1000 and sorted(rot)[-2] < 10    # one undetected pair, scored as the loop scores it
    assert ph["add"]["overall"][0]["0.02"] >= on["add"]["overall"][2]["0.02"]
    assert ph["add"]["overall"][0]["auc"] > on["add"]["overall"][2]["auc"]
    cfg.TEST.PHOTO_ITER = 0


@pytest.mark.parametrize("key", ["VSD", "BOP"])
def test_pred_eval_refuses_photo_with_vsd_or_bop(key):
    with pytest.raises(ValueError, match="TEST.PHOTO_ITER"):
        _fake_run(True, **{key: True})
    from deepim.config.config import reset_config

    reset_config()


# ------------------------------------------------------------------------------------------------------------------ small frames
def _rot(deg, axis):
    a = np.asarray(axis, np.float64)
    return pr.rodrigues(np.radians(deg) * a / np.linalg.norm(a))


def ellipsoid_render(pose, K, H, W, axes=(0.30, 0.24, 0.20)):
    """an analytic textured ellipsoid by ray casting -> image (3,H,W) float32 0..255 values, depth (H,W) float32 (0 = background).
    The texture is a smooth function of the surface point in the object frame."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R, t = np.asarray(pose, np.float64)[:, :3], np.asarray(pose, np.float64)[:, 3]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)
    inv = 1.0 / np.asarray(axes, np.float64)
    dq, oq = (ray @ R) * inv, (-t @ R) * inv           # the ray in the unit-sphere frame: o + s d
    a, b, c = np.sum(dq * dq, -1), 2.0 * np.sum(dq * oq, -1), float(np.sum(oq * oq)) - 1.0
    disc = b * b - 4.0 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a), 0.0)
    hit &= s > 0
    q = oq + s[..., None] * dq                         # on the unit sphere
    tex = np.stack([128.0 + 90.0 * np.sin(7.0 * q[..., 0] + 1.0) * np.cos(5.0 * q[..., 1]),
                    128.0 + 90.0 * np.sin(6.0 * q[..., 1] + 2.0) * np.cos(4.0 * q[..., 2] + 0.5),
                    128.0 + 90.0 * np.sin(5.0 * q[..., 2] + 3.0) * np.cos(6.0 * q[..., 0] + 1.5)])
    image = np.where(hit[None], tex, 0.0).astype(np.float32)
    return image, np.where(hit, s, 0.0).astype(np.float32)


def _small_batch(H, W, n, seed):
    """n pairs at H x W: the ellipsoid near the frame's middle, the input pose 3-4 degrees and about a centimetre off (a pixel of these frames is some 9 mm at the object), the observed image
    over noise with another gain and bias; every pair but the first has its own K"""
    rng = np.random.default_rng(seed)
    pm = np.array([103.939, 116.779, 123.68], np.float32)
    K0 = np.array([[1.7 * W, 0, 0.5 * W - 0.3], [0, 1.7 * W, 0.5 * H + 0.2], [0, 0, 1]], np.float32)
    Ks, gts, inits, obs, ren, dep = [], [], [], [], [], []
    for b in range(n):
        K = K0.copy()
        if b > 0:
            K[0, 0] *= 1.0 + 0.03 * b
            K[1, 1] *= 1.0 - 0.02 * b
            K[0, 2] += 1.5 * b
            K[1, 2] -= 1.0 * b
        R = _rot(rng.uniform(0, 360), rng.normal(size=3))
        gt = np.concatenate([R, np.array([[rng.uniform(-0.03, 0.03)], [rng.uniform(-0.02, 0.02)], [rng.uniform(0.95, 1.05)]])], axis=1)
        dR = _rot(rng.uniform(3.0, 4.0), rng.normal(size=3))
        init = np.concatenate([dR @ gt[:, :3], gt[:, 3:] + rng.normal(0, [0.008, 0.008, 0.01])[:, None]], axis=1).astype(np.float32)
        gt = gt.astype(np.float32)
        io, do = ellipsoid_render(gt, K, H, W)
        ir, dr = ellipsoid_render(init, K, H, W)
        obs.append(observed_recipe(np.round(io) - pm.reshape(3, 1, 1), do, seed * 10 + b, pm))
        ren.append((np.round(ir) - pm.reshape(3, 1, 1)).astype(np.float32))
        dep.append(dr[None])
        Ks.append(K.reshape(9))
        gts.append(gt)
        inits.append(init)
    return {"H": H, "W": W, "K": K0, "K_per_sample": np.stack(Ks).astype(np.float32), "pose_gt": np.stack(gts), "pose_in": np.stack(inits),
            "image_observed": np.stack(obs), "image_rendered": np.stack(ren), "depth_rendered": np.stack(dep)}


def _tight_boxes(depth):
    out = []
    for d in depth[:, 0]:
        ys, xs = np.nonzero(d > 0)
        out.append([xs.min(), xs.max(), ys.min(), ys.max()])
    return np.asarray(out, np.int32)


GPU_LEVELS, GPU_ITERS = 2, 3


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """the small-frame inputs of tests/test_gpu_photo.py: B = 3 at 48x64 and B = 2 at 37x50, two levels.  Per batch a dict of numpy
    arrays: the three images, pose_in, pose_gt, K (the first pair's, the call's K9), K_per_sample (B,9) and bbox (B,4) int32.
    48x64: pair 1's box reaches past the frame on three sides (clipped like clamp_bbox); pair 2's box is a small window of its render, so
    its coarsest level holds fewer than 64 template pixels (flagged there) while level 0 still updates.  37x50: a leftover row and
    column, W % 4 != 0 (the scalar paths)."""
    a = _small_batch(48, 64, 3, 11)
    box = _tight_boxes(a["depth_rendered"])
    box[1] = [-6, 70, -3, box[1][3]]
    cx, cy = (box[2][0] + box[2][1]) // 2, (box[2][2] + box[2][3]) // 2
    box[2] = [cx - 9, cx + 8, cy - 6, cy + 5]      # 18 x 12 = 216 pixels: 9 x 6 = 54 at level 1
    a["bbox"] = box
    b = _small_batch(37, 50, 2, 12)
    b["bbox"] = _tight_boxes(b["depth_rendered"])
    return a, b


@functools.lru_cache(maxsize=None)
def gpu_reference(which, iters=GPU_ITERS, with_bbox=True):
    """the restatement on gpu_batches()[which]: pose, stats, status, per-pair extras (planes, gain sums); computed once per case"""
    g = gpu_batches()[which]
    return pr.photo_refine(g["image_observed"], g["image_rendered"], g["depth_rendered"], g["pose_in"], g["K_per_sample"], GPU_LEVELS, iters,
                           HUBER, GATE, bbox=g["bbox"] if with_bbox else None, with_extra=True)


def _pose_err(pose, gt):
    """a pose distance without a model: the mean displacement of the ellipsoid's six axis ends"""
    ends = np.concatenate([np.diag([0.30, 0.24, 0.20]), -np.diag([0.30, 0.24, 0.20])])
    return pr.add_error(pose, gt, ends)


def test_gpu_batches_are_sound():
    for which, g in enumerate(gpu_batches()):
        B = g["pose_in"].shape[0]
        assert g["image_observed"].shape == (B, 3, g["H"], g["W"]) and g["depth_rendered"].shape == (B, 1, g["H"], g["W"])
        assert np.array_equal(g["K_per_sample"][0].reshape(3, 3), g["K"]) and not np.array_equal(g["K_per_sample"][1], g["K_per_sample"][0])
        for with_bbox in (True, False):
            pose, stats, status, extra = gpu_reference(which, GPU_ITERS, with_bbox)
            small = [2] if (which == 0 and with_bbox) else []
            for b in range(B):
                n_coarse = int(extra[b]["planes"]["valid"][GPU_LEVELS - 1].sum())
                before, after = _pose_err(g["pose_in"][b], g["pose_gt"][b]), _pose_err(pose[b], g["pose_gt"][b])
                print(which, with_bbox, b, "template", int(extra[b]["sums"][0]), n_coarse, "counts", stats[b, :, 0], "err mm", 1e3 * before,
                      1e3 * after)
                if b in small:   # flagged at the coarsest level, yet level 0 updates
                    assert n_coarse < pr.MIN_POINTS <= extra[b]["sums"][0]
                    assert status[b] == pr.STATUS_PHOTO_FEW_POINTS and stats[b, :GPU_ITERS, 0].max() < pr.MIN_POINTS
                    assert stats[b, GPU_ITERS:, 0].min() >= pr.MIN_POINTS and not np.array_equal(pose[b], g["pose_in"][b])
                else:
                    assert n_coarse >= 256, (which, b, n_coarse)
                    assert status[b] == 0 and stats[b, :, 0].min() >= pr.MIN_POINTS
                    assert after < 0.5 * before, (which, b, before, after)
    a = gpu_batches()[0]
    assert a["bbox"][1][0] < 0 and a["bbox"][1][1] > a["W"] - 1 and a["bbox"][1][2] < 0   # clipped by the frame
    full = gpu_reference(0, GPU_ITERS, False)[3][1]["planes"]["valid"][0]
    np.testing.assert_array_equal(gpu_reference(0, GPU_ITERS, True)[3][1]["planes"]["valid"][0], full)
