"""TEST.VIEWS_CALIB_ITER end to end: the Refiner of tests/test_gpu_views_refiner.py (G = 2 objects, V = 2 ring cameras, 480x640, the
identity pose head) loaded with camera 1's extrinsic off by a seeded rotation and shift.  The bars are those of tests/test_gpu_icp.py,
ADD <= 1e-3 m and |dt| <= 5e-4 m: an extrinsic error in a camera is an object pose error in that camera, so the extrinsic is measured
as the pose X'_1 T_g of every object, at its true rig pose T_g, against X*_1 T_g."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import icp_reference as ir  # noqa: E402
import views_reference as vr  # noqa: E402
from scene import make_test_config  # noqa: E402
from test_gpu_views_refiner import B, DEV, G, V, _bits, _errors, _load, setup  # noqa: E402,F401

CALIB_ITER = ICP_ITER = 10
ADD_BAR, DT_BAR = 1e-3, 5e-4
SEED, ANGLE_DEG, SHIFT_M = 2, 0.3, 3e-3   # the seed chosen on the CPU: 5.4 to 5.6 mm of displacement
CALIB_TENSORS = ("cam_T_rig_calib", "pose_calib", "pose_rig_calib", "calib_stats", "calib_stats_group", "calib_stats_view", "status_calib")
STAGE_TENSORS = ("pose_rig", "pose_views", "pose_icp", "pose_rig_icp", "icp_stats", "icp_stats_group", "status_icp")


def perturbed_rig(X, seed=SEED, angle_deg=ANGLE_DEG, shift=SHIFT_M):
    """X (V,3,4) -> the same rig with cameras 1.. moved by a seeded camera-frame rotation of angle_deg about a random axis and a shift
    of `shift` metres in a random direction (camera 0, the gauge, is exact)"""
    rng = np.random.default_rng(seed)
    out = np.asarray(X, np.float32).copy()
    for v in range(1, len(out)):
        axis, d = rng.normal(size=3), rng.normal(size=3)
        P = vr.mat(ir.rodrigues(np.radians(angle_deg) * axis / np.linalg.norm(axis)), shift * d / np.linalg.norm(d))
        out[v] = vr.mul(P, out[v]).astype(np.float32)
    return out


def extrinsic_errors(X1, X1_true, rig_gt, pts):
    """camera 1's extrinsic as object pose errors in that camera -> [(ADD, |dt|)] per object"""
    return [_errors(vr.mul(X1, T), vr.mul(X1_true, T), pts) for T in np.asarray(rig_gt, np.float64)]


def _refiner(setup, graph=False, drop_keys=False, **keys):
    from deepim.core.tester import Refiner

    cfg, pred, data, _ = setup
    make_test_config(test_iter=2)
    for k, v in keys.items():
        cfg.TEST[k] = v
    if drop_keys:
        for k in ("VIEWS_CALIB_ITER", "VIEWS_CALIB_MAX_DIST"):
            cfg.TEST.pop(k)
    try:
        return Refiner(cfg, pred, data.render_machine, B, capture_graph=graph)
    finally:
        make_test_config(test_iter=2)


def _snapshot(r, names):
    torch.cuda.synchronize()
    return {n: getattr(r, n).cpu().numpy().copy() for n in names}


@pytest.fixture(scope="module")
def runs(setup):
    """every Refiner once: calibration on (eager and graph) and off, on the perturbed and on the true extrinsics"""
    cfg, pred, data, batch = setup
    X_true = batch["cam_T_rig"].cpu().numpy()
    X_off = np.tile(perturbed_rig(X_true[:V]), (G, 1, 1))
    on = dict(VIEWS=V, ICP_ITER=ICP_ITER, VIEWS_CALIB_ITER=CALIB_ITER)
    eager, graph, plain = _refiner(setup, **on), _refiner(setup, graph=True, **on), _refiner(setup, VIEWS=V, ICP_ITER=ICP_ITER, VIEWS_CALIB_ITER=0)
    assert plain.calib is None and not hasattr(plain, "cam_T_rig_calib") and plain.views.cam_T_rig_used is plain.views.cam_T_rig
    out = dict(X_true=X_true, X_off=X_off, gt=batch["pose_gt"].cpu().numpy(), rig_gt=batch["pose_rig_gt"].cpu().numpy(),
               pts=data.models[0][0].astype(np.float64))
    for name, X in (("off", X_off), ("true", X_true)):                    # the second load: other extrinsics reach the replayed graph
        for who, r in (("eager", eager), ("graph", graph), ("plain", plain)):
            _load(r, batch, cam_T_rig=torch.from_numpy(X).to(DEV))
            r.refine()
            out[who, name] = _snapshot(r, STAGE_TENSORS + (CALIB_TENSORS if r.calib is not None else ()))
            assert _bits(r.views.cam_T_rig).tolist() == _bits(X).tolist()  # the loaded extrinsics are never overwritten
    assert graph.graph is not None and eager.graph is None
    return out


def test_the_perturbation_is_visible_and_inside_the_gate(runs):
    from deepim.config.config import config

    worst = [e[0] for e in extrinsic_errors(runs["X_off"][1], runs["X_true"][1], runs["rig_gt"], runs["pts"])]
    print("mean displacement of the model points under the loaded extrinsic of camera 1:", worst)
    assert min(worst) > 2e-3 and max(worst) < 0.5 * float(config.TEST.ICP_MAX_DIST)


def test_calibration_recovers_the_extrinsic_and_the_poses(runs):
    got, plain = runs["eager", "off"], runs["plain", "off"]
    assert got["status_calib"].tolist() == [0] * B and got["status_icp"].tolist() == [0] * B
    before = extrinsic_errors(runs["X_off"][1], runs["X_true"][1], runs["rig_gt"], runs["pts"])
    after = extrinsic_errors(got["cam_T_rig_calib"][1], runs["X_true"][1], runs["rig_gt"], runs["pts"])
    row_dt = np.linalg.norm(got["cam_T_rig_calib"][1][:, 3].astype(np.float64) - runs["X_true"][1][:, 3])
    print("camera 1 extrinsic (ADD, |dt|) per object: loaded", before, "calibrated", after, "; |t' - t*| of the row itself", row_dt)
    for add, dt in after:
        assert add <= ADD_BAR and dt <= DT_BAR
    assert row_dt <= DT_BAR                                                   # ... and the translation of the row itself
    assert np.array_equal(_bits(got["cam_T_rig_calib"][0]), _bits(runs["X_true"][0]))   # the gauge camera keeps its bits
    pose = [_errors(got["pose_rig_icp"][g], runs["rig_gt"][g], runs["pts"]) for g in range(G)]
    cam1 = [_errors(got["pose_icp"][g * V + 1], runs["gt"][g * V + 1], runs["pts"]) for g in range(G)]
    print("joint ICP after the calibration: rig pose (ADD, |dt|)", pose, "in camera 1", cam1)
    for add, dt in pose + cam1:
        assert add <= ADD_BAR and dt <= DT_BAR
    # negative control: the same load without the calibration misses a bar in camera 1
    control = [_errors(plain["pose_icp"][g * V + 1], runs["gt"][g * V + 1], runs["pts"]) for g in range(G)]
    control_rig = [_errors(plain["pose_rig_icp"][g], runs["rig_gt"][g], runs["pts"]) for g in range(G)]
    print("joint ICP without it: in camera 1", control, "rig pose", control_rig)
    assert all(add > ADD_BAR or dt > DT_BAR for add, dt in control)


def test_nothing_to_fix(runs):
    got = runs["eager", "true"]
    assert got["status_calib"].tolist() == [0] * B
    moved = extrinsic_errors(got["cam_T_rig_calib"][1], runs["X_true"][1], runs["rig_gt"], runs["pts"])
    print("true extrinsics loaded: the calibration moves camera 1 by (ADD, |dt|)", moved)
    for add, dt in moved:
        assert add <= ADD_BAR and dt <= DT_BAR
    for g in range(G):
        add, dt = _errors(got["pose_rig_icp"][g], runs["rig_gt"][g], runs["pts"])
        assert add <= ADD_BAR and dt <= DT_BAR


def test_poses_agree_with_the_calibrated_extrinsics(runs):
    for name in ("off", "true"):
        got = runs["eager", name]
        Xc = np.tile(got["cam_T_rig_calib"], (G, 1, 1))
        assert np.all(vr.ulp_close(got["pose_calib"], vr.views_from_rig(got["pose_rig_calib"], Xc, V)))
        assert np.all(vr.ulp_close(got["pose_icp"], vr.views_from_rig(got["pose_rig_icp"], Xc, V)))   # the later stage reads them too
        assert got["calib_stats_view"].shape == (V, CALIB_ITER, 2) and np.all(got["calib_stats_view"][:, :, 0] >= ir.MIN_POINTS)
        assert got["calib_stats_group"][:, 0, 0].tolist() == got["calib_stats"][:, 0, 0].reshape(G, V).sum(1).tolist()
        assert got["calib_stats_view"][:, 0, 0].tolist() == got["calib_stats"][:, 0, 0].reshape(G, V).sum(0).tolist()


def test_graph_replay_equals_eager(runs):
    for name in ("off", "true"):
        for key in STAGE_TENSORS + CALIB_TENSORS:
            assert np.array_equal(_bits(runs["graph", name][key]), _bits(runs["eager", name][key])), (name, key)
    assert np.abs(runs["graph", "off"]["cam_T_rig_calib"][1] - runs["graph", "true"]["cam_T_rig_calib"][1]).max() < 1e-2
    assert not np.array_equal(_bits(runs["graph", "off"]["pose_rig_calib"]), _bits(runs["graph", "true"]["pose_rig_calib"]))


def test_key_off_is_the_refiner_without_the_key(setup, runs):
    cfg, pred, data, batch = setup
    r = _refiner(setup, drop_keys=True, VIEWS=V, ICP_ITER=ICP_ITER)
    assert r.calib is None
    _load(r, batch, cam_T_rig=torch.from_numpy(runs["X_off"]).to(DEV))
    r.refine()
    got = _snapshot(r, STAGE_TENSORS)
    for key in STAGE_TENSORS:
        assert np.array_equal(_bits(got[key]), _bits(runs["plain", "off"][key])), key


def test_load_refuses_groups_that_do_not_repeat_one_rig(setup, runs):
    cfg, pred, data, batch = setup
    r = _refiner(setup, VIEWS=V, VIEWS_CALIB_ITER=2)
    X = runs["X_true"].copy()
    X[V + 1] = runs["X_off"][1]
    with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_ITER.*cam_T_rig\[3\]"):
        _load(r, batch, cam_T_rig=torch.from_numpy(X))
    with pytest.raises(ValueError, match=r"TEST\.VIEWS_CALIB_ITER.*depth_observed"):
        r.load(batch["image_observed"], batch["image_rendered"], batch["mask_segmentation"], batch["mask_rendered"], batch["src_pose"],
               batch["class_index"], K=batch["K"], cam_T_rig=batch["cam_T_rig"])
    _load(r, batch, cam_T_rig=runs["eager", "off"]["cam_T_rig_calib"])    # what a calibration returned is accepted, as (V,3,4)
