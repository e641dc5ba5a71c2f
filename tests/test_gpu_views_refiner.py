"""TEST.VIEWS end to end: a Refiner whose batch holds G = 2 objects seen by V = 2 ring cameras (lib/dataset/synthetic_views.py), at
480x640 with seeded weights.  The pose head is the identity head of tests/test_gpu_hypotheses.py, so the loop leaves every sample at
its starting pose and the tests see the consensus and the joint stages on known inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hyp_reference as hr  # noqa: E402
import icp_reference as ir  # noqa: E402
import views_reference as vr  # noqa: E402
from scene import make_test_config  # noqa: E402

DEV = "cuda:0"
G, V = 2, 2
B = G * V
ICP_ITER = 10
EPS32 = float(np.finfo(np.float32).eps)
NEW_TENSORS = ("views_score", "views_choice", "pose_rig", "pose_views", "status_views", "pose_icp", "pose_rig_icp", "icp_stats",
               "icp_stats_group", "status_icp")


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.uint32)


@pytest.fixture(scope="module")
def setup(hip_lib):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_views import SyntheticViews

    cfg = make_test_config(test_iter=2)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    for k in ("rot_weight", "trans_weight", "trans_bias"):     # the identity head: (1,0,0,0 | 0,0,0) whatever the network sees
        params[k] = np.zeros_like(params[k])
    params["rot_bias"] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    data = SyntheticViews(cfg, G, V, seed=2333, device=DEV)
    return cfg, Predictor(cfg, params, B), data, data.batch()


def _refiner(setup, graph=False, drop_keys=False, **keys):
    """a Refiner under TEST keys that are put back afterwards (the config is global); drop_keys: a config that has never heard of VIEWS"""
    from deepim.core.tester import Refiner

    cfg, pred, data, _ = setup
    make_test_config(test_iter=2)
    for k, v in keys.items():
        cfg.TEST[k] = v
    if drop_keys:
        for k in ("VIEWS", "VIEWS_SCORE"):
            cfg.TEST.pop(k)
    try:
        return Refiner(cfg, pred, data.render_machine, B, capture_graph=graph)
    finally:
        make_test_config(test_iter=2)


def _load(ref, batch, **over):
    b = dict(batch, **over)
    extra = {"cam_T_rig": b["cam_T_rig"]} if ref.V > 1 else {}
    ref.load(b["image_observed"], b["image_rendered"], b["mask_segmentation"], b["mask_rendered"], b["src_pose"], b["class_index"],
             depth_observed=b["depth_observed"] if ref.depth_observed is not None else None, K=b["K"], **extra)


def _seen_from(X, rig):
    """X (B,3,4), rig (G,3,4) -> (B,3,4) float64: the rig poses seen from every camera"""
    return vr.views_from_rig(np.asarray(rig, np.float64), np.asarray(X, np.float64), V)


def _errors(pose, gt, pts):
    return ir.add_error(pose, gt, pts), float(np.linalg.norm(np.asarray(pose, np.float64)[:, 3] - np.asarray(gt, np.float64)[:, 3]))


# ------------------------------------------------------------------------------------------------------------------ consistency
def test_joint_icp_poses_agree_with_the_extrinsics(setup):
    """pose_icp[b] is X_b pose_rig_icp[g] within one float32 ulp per entry; the same samples refined one by one are not.
    The entry's own per-sample output (the stage's pose_step) is the same pose up to float32 roundings on the way -- of pose_views,
    of the extrinsics (rigid to a rounding only) and of the two results: within 16 eps32 of the pose's scale."""
    cfg, pred, data, batch = setup
    X = batch["cam_T_rig"].cpu().numpy()
    joint = _refiner(setup, VIEWS=2, ICP_ITER=ICP_ITER)
    _load(joint, batch)
    joint.refine()
    torch.cuda.synchronize()
    assert joint.status_icp.cpu().tolist() == [0] * B and joint.views_choice.cpu().min() >= 0
    pose, rig = joint.pose_icp.cpu().numpy(), joint.pose_rig_icp.cpu().numpy()
    want = _seen_from(X, rig)
    assert np.all(vr.ulp_close(pose, want))
    step = joint.stages["icp"].pose_step.cpu().numpy()
    scale = np.maximum(1.0, np.abs(want).max(axis=(1, 2), keepdims=True))
    print("entry's own pose_out against X pose_rig: worst", float((np.abs(step - want) / (EPS32 * scale)).max()), "eps32 of the scale")
    assert np.all(np.abs(step - want) <= 16 * EPS32 * scale)
    assert np.abs(pose - joint.pose_views.cpu().numpy()).max() > 1e-4             # the stage moved the poses
    assert joint.icp_stats_group.cpu().numpy()[:, 0, 0].tolist() == joint.icp_stats.cpu().numpy()[:, 0, 0].reshape(G, V).sum(1).tolist()
    # negative control: VIEWS 1 on the same samples
    single = _refiner(setup, VIEWS=1, ICP_ITER=ICP_ITER)
    assert single.views is None and single.pose_rig_icp is None
    _load(single, batch)
    single.refine()
    torch.cuda.synchronize()
    alone = single.pose_icp.cpu().numpy()
    for g in range(G):
        rig_g = vr.mul(vr.inverse(X[g * V]), alone[g * V])                         # the rig pose view 0 implies
        other = vr.mul(X[g * V + 1], rig_g)
        gap = np.abs(alone[g * V + 1] - other).max()
        print("group", g, "independent views disagree by", gap)
        assert not np.all(vr.ulp_close(alone[g * V + 1], other)) and gap > 100 * EPS32


# ------------------------------------------------------------------------------------------------------------------ a blinded camera
def test_blinded_camera_is_carried_by_the_other(setup):
    cfg, pred, data, batch = setup
    pts = data.models[0][0].astype(np.float64)
    depth = batch["depth_observed"].clone()
    depth[1::V].zero_()                                                            # view 1 of every group sees no depth
    gt = batch["pose_gt"].cpu().numpy()
    single = _refiner(setup, VIEWS=1, ICP_ITER=ICP_ITER)
    _load(single, batch, depth_observed=depth)
    single.refine()
    torch.cuda.synchronize()
    st, alone, start = single.status_icp.cpu().numpy(), single.pose_icp.cpu().numpy(), single.poses_iter[-1].cpu().numpy()
    joint = _refiner(setup, VIEWS=2, ICP_ITER=ICP_ITER)
    _load(joint, batch, depth_observed=depth)
    joint.refine()
    torch.cuda.synchronize()
    together = joint.pose_icp.cpu().numpy()
    assert joint.status_icp.cpu().tolist() == [0] * B
    assert np.all(joint.icp_stats.cpu().numpy()[1::V, :, 0] == 0)                  # the blind view contributes nothing
    for g in range(G):
        seeing, blind = g * V, g * V + 1
        assert st[blind] & ir.STATUS_ICP_FEW_POINTS and st[seeing] == 0
        assert np.array_equal(_bits(alone[blind]), _bits(start[blind]))            # alone it returns its start
        e_alone, e_seeing, e_joint = _errors(alone[blind], gt[blind], pts), _errors(alone[seeing], gt[seeing], pts), _errors(
            together[blind], gt[blind], pts)
        print("group {}: blind view alone ADD {:.2e} |dt| {:.2e}; seeing view alone {:.2e} {:.2e}; blind view in the group {:.2e} {:.2e}".format(
            g, *(e_alone + e_seeing + e_joint)))
        assert e_seeing[0] <= 1e-3 and e_seeing[1] <= 5e-4                         # the bars of tests/test_gpu_icp.py, met by the seeing view alone
        assert e_joint[0] <= 1e-3 and e_joint[1] <= 5e-4
        assert e_alone[0] > 1e-3


# ------------------------------------------------------------------------------------------------------------------ consensus
def test_consensus_picks_the_view_that_is_right(setup):
    cfg, pred, data, batch = setup
    init = data.samples["pose_init"].copy()
    far = [1, 2]                                                                   # view 1 of group 0, view 0 of group 1
    turn = hr.rodrigues(hr.fibonacci_axes(4)[1], np.radians(30.0))                 # a losing hypothesis of tests/test_gpu_hypotheses.py
    for b in far:
        init[b, :, :3] = (turn @ init[b, :, :3].astype(np.float64)).astype(np.float32)
    moved = data.batch(pose_init=init)
    ref = _refiner(setup, VIEWS=2)
    _load(ref, moved)
    ref.refine()
    torch.cuda.synchronize()
    assert ref.views_choice.cpu().tolist() == [0, 1]
    vc = ref.views
    want = hr.scores("rgb", moved["image_observed"].cpu().numpy(), vc.image.cpu().numpy(), vc.depth.cpu().numpy(), vc.bbox.cpu().numpy())
    score = ref.views_score.cpu().numpy()
    print("scores", score.tolist(), "restatement", want.tolist())
    assert np.all(np.abs(score.astype(np.float64) - want) <= 1e-5)
    for b in far:
        assert score[b] < score[b ^ 1] - 0.05
    last = ref.poses_iter[-1].cpu().numpy()
    status = ref.status_iter[-1].cpu().numpy()
    X = moved["cam_T_rig"].cpu().numpy()
    from deepim.core.views import FATAL_MASK
    r_choice, r_rig, r_views, r_bits = vr.consensus(score, status, FATAL_MASK, last, X, V)
    assert r_choice.tolist() == [0, 1] and not r_bits.any()
    assert np.all(vr.ulp_close(ref.pose_rig.cpu().numpy(), r_rig)) and np.all(vr.ulp_close(ref.pose_views.cpu().numpy(), r_views))
    for b in (0, 3):
        assert np.array_equal(_bits(ref.pose_views[b]), _bits(last[b]))            # the chosen views keep their pose
    assert ref.status_views.cpu().tolist() == [0] * B
    gt = moved["pose_gt"].cpu().numpy()
    for b in far:                                                                  # the far view is brought back by its group
        assert np.abs(ref.pose_views[b].cpu().numpy() - gt[b]).max() < 0.1 < np.abs(last[b] - gt[b]).max()


# ------------------------------------------------------------------------------------------------------------------ graph capture
def test_graph_replay_equals_eager_and_takes_new_extrinsics(setup):
    from lib.dataset.synthetic_views import ring_rig

    cfg, pred, data, batch = setup
    keys = dict(VIEWS=2, ICP_ITER=4, PHOTO_ITER=2, SIL_ITER=2)
    names = NEW_TENSORS + ("pose_photo", "pose_rig_photo", "photo_stats_group", "pose_sil", "pose_rig_sil", "sil_stats_group")
    eager, graph = _refiner(setup, **keys), _refiner(setup, graph=True, **keys)
    other = torch.from_numpy(np.tile(ring_rig(V, radius=0.8, span_deg=60.0, seed=5)[0], (G, 1, 1))).to(DEV)
    first = None
    for X in (batch["cam_T_rig"], other):
        for r in (eager, graph):
            _load(r, batch, cam_T_rig=X)
            r.refine()
        torch.cuda.synchronize()
        assert graph.graph is not None and eager.graph is None
        for name in names:
            assert getattr(graph, name) is not None, name
            assert np.array_equal(_bits(getattr(graph, name)), _bits(getattr(eager, name))), name
        for name in ("pose_photo", "pose_sil"):                                    # every joint stage publishes X pose_rig
            stage_rig = getattr(graph, name.replace("pose_", "pose_rig_")).cpu().numpy()
            assert np.all(vr.ulp_close(getattr(graph, name).cpu().numpy(), _seen_from(X.cpu().numpy(), stage_rig))), name
        now = graph.pose_rig_icp.cpu().numpy().copy()
        if first is not None:
            assert np.abs(now - first).max() > 1e-3                                # the second load's extrinsics reached the replay
        first = now


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_views_1_is_the_refiner_without_the_key(setup):
    cfg, pred, data, batch = setup
    out = []
    for drop in (True, False):
        r = _refiner(setup, drop_keys=drop, ICP_ITER=4, **({} if drop else {"VIEWS": 1}))
        assert r.V == 1 and r.views is None and r.views_score is None and r.pose_rig_icp is None and r.icp_stats_group is None
        _load(r, batch)
        poses = r.refine()
        torch.cuda.synchronize()
        out.append([_bits(t) for t in (poses, r.se3_iter, r.status_iter, r.pose_icp, r.icp_stats, r.status_icp)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_load_checks(setup):
    cfg, pred, data, batch = setup
    joint = _refiner(setup, VIEWS=2)
    with pytest.raises(ValueError, match="cam_T_rig"):
        _load(joint, batch, cam_T_rig=None)
    bad = batch["cam_T_rig"].clone()
    bad[2, :, :3] *= 1.01
    with pytest.raises(ValueError, match=r"cam_T_rig\[2\]"):
        _load(joint, batch, cam_T_rig=bad)
    _load(joint, batch, cam_T_rig=batch["cam_T_rig"][:V].cpu())                    # (V,3,4), from the host
    assert np.array_equal(_bits(joint.views.cam_T_rig), _bits(batch["cam_T_rig"]))
    with pytest.raises(ValueError, match=r"TEST\.VIEWS.*load_staged"):
        joint.load_staged(None, None)
    single = _refiner(setup, VIEWS=1)
    with pytest.raises(ValueError, match="TEST.VIEWS"):
        single.load(batch["image_observed"], batch["image_rendered"], batch["mask_segmentation"], batch["mask_rendered"], batch["src_pose"],
                    batch["class_index"], cam_T_rig=batch["cam_T_rig"])
    with pytest.raises(ValueError, match="TEST.VIEWS"):
        _refiner(setup, VIEWS=3)                                                   # 4 samples are not groups of 3
