"""Visible surface discrepancy on the device (csrc/vsd.hip, ops.vsd_errors, pred_eval with TEST.VSD) against the reference's masks
(tests/golden/vsd_golden.npz) and the numpy restatement lib/utils/pose_error.py vsd.

Bars: the counts and the `step` errors are integers and one division: equal exactly.  The `tlinear` errors differ from numpy's only
in the order of a float64 sum of at most a few thousand terms in [0, 1]: |dev - ref| <= 1e-12 * max(1, |ref|)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_test_config  # noqa: E402

DEV = "cuda:0"
COSTS = ("step", "tlinear")
T_SETS, ROWS = 2, 3


def ops():
    from lib.hip import ops as o

    return o


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _box(depth):
    """the rasteriser's box of the drawn pixels: {min_x, max_x, min_y, max_y}, empty = {W, -1, H, -1}"""
    H, W = depth.shape
    ys, xs = np.nonzero(depth > 0)
    return [xs.min(), xs.max(), ys.min(), ys.max()] if len(xs) else [W, -1, H, -1]


def _tlinear_bar(dev, ref, what):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    diff = np.abs(dev - ref)
    print("{}: max |dev - ref| = {:.3e} (bar 1e-12 * max(1, |ref|))".format(what, diff.max()))
    assert np.all(diff <= 1e-12 * np.maximum(1.0, np.abs(ref))), (what, float(diff.max()))


# ------------------------------------------------------------------------------------------------------------------ golden layouts
_LAYOUTS = {}


def layout(name):
    """per golden case: three pairs (the case; the case mirrored; the case with the two renders in each other's role) x two estimates
    (the pair's own; the same moved two rows down), two cameras, and the host's numbers for all of it -- computed once"""
    if name in _LAYOUTS:
        return _LAYOUTS[name]
    from lib.utils.pose_error import vsd

    g = np.load(os.path.join(GOLDEN, "vsd_golden.npz"))
    c = {k[2:]: g[k] for k in g.files if k.startswith(name + "_")}
    taus, delta = [float(t) for t in g["taus"]], float(c["delta"])
    other = g[("b" if name == "a" else "a") + "_K"]
    obs = [c["depth_test"], c["depth_test"][:, ::-1].copy(), c["depth_test"]]
    gt = [c["depth_gt"], c["depth_gt"][:, ::-1].copy(), c["depth_est"]]
    est0 = [c["depth_est"], c["depth_est"][:, ::-1].copy(), c["depth_gt"]]
    est = [est0, [np.roll(e, 2, axis=0) for e in est0]]
    cams = [c["K"], other, c["K"]]
    ref = {}
    for mode, Ks in (("one", [c["K"]] * ROWS), ("per_pair", cams)):
        for cost in COSTS:
            e = np.zeros((T_SETS, ROWS, len(taus)))
            n = np.zeros((T_SETS, ROWS, 3), dtype=np.int64)
            for t in range(T_SETS):
                for b in range(ROWS):
                    for k, tau in enumerate(taus):
                        e[t, b, k], n[t, b] = vsd(est[t][b], gt[b], obs[b], Ks[b], delta, tau, cost)
            ref[(mode, cost)] = (e, n)
    # row 0, estimate 0 is the golden case: the host's counts there are the reference's own masks'
    vg, ve = c["visib_gt"], c["visib_est"]
    assert ref[("one", "step")][1][0, 0].tolist() == [int(vg.sum()), int((vg | ve).sum()), int((vg & ve).sum())]
    _LAYOUTS[name] = dict(obs=obs, gt=gt, est=est, cams=cams, K=c["K"], taus=taus, delta=delta, ref=ref)
    return _LAYOUTS[name]


def run_layout(L, perm, cost, taus, per_pair, boxes, workspace=None):
    obs = _dev(np.stack([L["obs"][b] for b in perm]))
    gt = _dev(np.stack([L["gt"][b] for b in perm]))
    est = _dev(np.stack([np.stack([L["est"][t][b] for b in perm]) for t in range(T_SETS)]))
    extra = {}
    if per_pair:
        extra["K_per_sample"] = np.stack([L["cams"][b] for b in perm])
    if boxes:
        extra["bbox_gt"] = _dev(np.array([_box(L["gt"][b]) for b in perm], np.int32))
        extra["bbox_est"] = _dev(np.array([[_box(L["est"][t][b]) for b in perm] for t in range(T_SETS)], np.int32))
    e, n = ops().vsd_errors(obs, gt, est, L["K"], L["delta"], taus, cost, workspace=workspace, **extra)
    return e.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("per_pair", [False, True], ids=["one_K", "per_pair_K"])
@pytest.mark.parametrize("name", ["a", "b"], ids=["48x64", "50x63"])
def test_kernel_equals_the_host_on_the_golden_planes(hip_lib, name, per_pair):
    L = layout(name)
    for cost in COSTS:
        ref_e, ref_n = L["ref"][("per_pair" if per_pair else "one", cost)]
        for perm in ((0, 1, 2), (2, 0, 1)):
            got = {}
            for boxes in (False, True):
                e, n = run_layout(L, perm, cost, L["taus"], per_pair, boxes)
                got[boxes] = (e, n)
                want_e, want_n = ref_e[:, list(perm)], ref_n[:, list(perm)]
                assert np.array_equal(n[:, :, :3], want_n), (name, cost, perm, boxes, n[:, :, :3].tolist(), want_n.tolist())
                drawn = np.array([[(L["gt"][b] > 0).sum() for b in perm]] * T_SETS)
                assert np.array_equal(n[:, :, 3], drawn)
                if cost == "step":
                    assert np.array_equal(e, want_e), (name, perm, boxes, np.abs(e - want_e).max())
                else:
                    _tlinear_bar(e, want_e, "{} tlinear perm {} boxes {}".format(name, perm, boxes))
            # boxes only skip pixels that add nothing: the same bits
            assert np.array_equal(got[False][0].view(np.uint64), got[True][0].view(np.uint64))
            assert np.array_equal(got[False][1], got[True][1])


@pytest.mark.parametrize("name", ["a", "b"], ids=["48x64", "50x63"])
def test_several_taus_in_one_call_equal_single_calls_and_a_dirty_workspace_changes_nothing(hip_lib, name):
    L = layout(name)
    # exactly dim_vsd_workspace_bytes between guards, at the documented minimum alignment (8 mod 16)
    arena = guard_arena.workspace(ops().lib().dim_vsd_workspace_bytes(T_SETS, ROWS), 8, DEV)
    work = arena.view()
    for cost in COSTS:
        work.fill_(float("nan"))
        all8, n8 = run_layout(L, (0, 1, 2), cost, L["taus"], True, True, workspace=work)
        arena.check("dim_vsd_errors workspace, NaN before the call, " + cost)
        work.copy_(torch.randn(work.shape, dtype=torch.float64, device=DEV) * 1e6)
        again, n_again = run_layout(L, (0, 1, 2), cost, L["taus"], True, True, workspace=work)
        arena.check("dim_vsd_errors workspace, noise before the call, " + cost)
        assert np.array_equal(all8.view(np.uint64), again.view(np.uint64)) and np.array_equal(n8, n_again)
        single = [run_layout(L, (0, 1, 2), cost, [tau], True, True)[0][:, :, 0] for tau in L["taus"]]
        for k in range(8):
            assert np.array_equal(all8[:, :, k].view(np.uint64), single[k].view(np.uint64)), (cost, k)
        three, n3 = run_layout(L, (0, 1, 2), cost, L["taus"][2:5], True, True)
        assert np.array_equal(three.view(np.uint64), all8[:, :, 2:5].copy().view(np.uint64)) and np.array_equal(n3, n8)


def test_empty_planes_and_a_nan_pixel(hip_lib):
    from lib.utils.pose_error import vsd

    L = layout("b")
    obs, gt, est = L["obs"][0], L["gt"][0], L["est"][0][0]
    zero = np.zeros_like(gt)
    for planes in ((zero, zero, zero), (zero, gt, est)):      # everything empty; no observed depth at all
        for cost in COSTS:
            e, n = ops().vsd_errors(_dev(planes[0][None]), _dev(planes[1][None]), _dev(planes[2][None]), L["K"], L["delta"], [0.02, 0.03], cost)
            assert e.cpu().tolist() == [[1.0, 1.0]] and n.cpu()[0, :3].tolist() == [0, 0, 0]
    # one NaN in the observed depth, on a pixel of the intersection: it drops out of every set, as on the host
    e0, n0 = vsd(est, gt, obs, L["K"], L["delta"], 0.02, "step")
    from lib.utils.misc import depth_im_to_dist_im
    from lib.utils.visibility import estimate_visib_mask_est, estimate_visib_mask_gt
    s = [depth_im_to_dist_im(d, L["K"]) for d in (obs, gt, est)]
    vg = estimate_visib_mask_gt(s[0], s[1], L["delta"])
    y, x = np.argwhere(vg & estimate_visib_mask_est(s[0], s[2], vg, L["delta"]))[7]
    holed = obs.copy()
    holed[y, x] = np.nan
    e1, n1 = vsd(est, gt, holed, L["K"], L["delta"], 0.02, "step")
    assert n1 == (n0[0] - 1, n0[1] - 1, n0[2] - 1)
    e, n = ops().vsd_errors(_dev(holed[None]), _dev(gt[None]), _dev(est[None]), L["K"], L["delta"], [0.02], "step")
    assert n.cpu()[0, :3].tolist() == list(n1) and e.cpu().item() == e1


def test_bad_arguments_raise(hip_lib):
    z = torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV)
    K = np.eye(3)
    with pytest.raises(ValueError):
        ops().vsd_errors(z, z, z, K, 0.015, [0.01] * 9)
    with pytest.raises(ValueError):
        ops().vsd_errors(z, z, z, K, 0.015, [0.02], "linear")
    with pytest.raises(ValueError):
        ops().vsd_errors(z, z, z, K, 0.015, [0.0])


# ------------------------------------------------------------------------------------------------------------------ a rendered scene
SCENE_H, SCENE_W, SCENE_B = 120, 160, 4
_SCENE = {}


def scene():
    """four poses of the synthetic mesh rendered at 120 x 160 with the LINEMOD camera scaled by 1/4 -- once"""
    if _SCENE:
        return _SCENE
    from lib.render_hip.render_py_multi import Render_Py
    from lib.utils import synthetic as syn

    K = np.asarray(syn.LINEMOD_K, np.float32).copy()
    K[:2] *= SCENE_W / 640.0
    rm = Render_Py(None, ["ape"], K, width=SCENE_W, height=SCENE_H, device=DEV, meshes=syn.make_models(seed=2333, n_models=1, subdiv=3))
    cls, gt, _ = syn.sample_pairs(77, SCENE_B, n_classes=1)
    _SCENE.update(rm=rm, K=K.astype(np.float64), cls=_dev(np.asarray(cls, np.int32)), gt=np.asarray(gt, np.float32))
    _SCENE["d_gt"], _SCENE["box_gt"] = render(_SCENE["gt"])
    return _SCENE


def render(poses):
    s = _SCENE
    depth = torch.zeros((SCENE_B, 1, SCENE_H, SCENE_W), dtype=torch.float32, device=DEV)
    bbox = torch.zeros((SCENE_B, 4), dtype=torch.int32, device=DEV)
    s["rm"].render_batch(s["cls"], _dev(np.asarray(poses, np.float32)), depth=depth, bbox=bbox, mask_thr=0.0)
    return depth, bbox


def score(obs, d_est, box_est, delta, tau, cost):
    s = scene()
    e, n = ops().vsd_errors(obs, s["d_gt"], d_est, s["K"], delta, [tau], cost, bbox_gt=s["box_gt"], bbox_est=box_est)
    return e.cpu().numpy()[:, 0], n.cpu().numpy()


def test_scene_equal_poses_with_and_without_an_occluder(hip_lib):
    s = scene()
    drawn = (s["d_gt"] > 0).sum(dim=(1, 2, 3)).cpu().numpy()
    assert np.all(drawn > 100)
    e, n = score(s["d_gt"], s["d_gt"], s["box_gt"], 0.015, 0.02, "tlinear")
    assert np.all(e == 0.0) and np.array_equal(n[:, 0], drawn) and np.array_equal(n[:, 1], drawn) and np.array_equal(n[:, 3], drawn)
    # a fronto-parallel plate 30 cm from the camera over the left half of every box
    obs = s["d_gt"].clone()
    left = []
    for b, (x0, x1, y0, y1) in enumerate(s["box_gt"].cpu().tolist()):
        xm = (x0 + x1) // 2
        obs[b, 0, y0:y1 + 1, x0:xm + 1] = 0.3
        left.append(int((s["d_gt"][b, 0, :, xm + 1:] > 0).sum()))
    e, n = score(obs, s["d_gt"], s["box_gt"], 0.015, 0.02, "tlinear")
    assert np.all(e == 0.0) and n[:, 0].tolist() == left and n[:, 1].tolist() == left and np.all(np.array(left) < drawn)


def test_scene_shifted_estimates(hip_lib):
    s = scene()
    box = s["box_gt"].cpu().numpy()
    # sideways by two box widths: no pixel of the estimate lands on the ground truth's
    far = s["gt"].copy()
    far[:, 0, 3] += 2.0 * (box[:, 1] - box[:, 0] + 1) * far[:, 2, 3] / s["K"][0, 0]
    d_est, box_est = render(far)
    for cost in COSTS:
        e, n = score(s["d_gt"], d_est, box_est, 0.015, 0.02, cost)
        assert np.all(e == 1.0) and np.all(n[:, 2] == 0), (cost, e)
    # tau / 2 along the optical axis, tau = 4 delta: half the linear cost, under the step
    delta, tau = 0.005, 0.02
    near = s["gt"].copy()
    near[:, 2, 3] += tau / 2
    d_est, box_est = render(near)
    e_lin, _ = score(s["d_gt"], d_est, box_est, delta, tau, "tlinear")
    e_step, _ = score(s["d_gt"], d_est, box_est, delta, tau, "step")
    print("tau/2 along z: tlinear", e_lin, "step", e_step)
    assert np.all((e_lin > 0.3) & (e_lin < 0.7)), e_lin
    assert np.all(e_step < 0.1), e_step


# ------------------------------------------------------------------------------------------------------------------ pred_eval
PAIRS, BATCH = 4, 2


def _same(a, b, path="out"):
    """exact equality of two nested results (dicts, lists, arrays, numbers; NaN equals NaN)"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "{}[{!r}]".format(path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "{}[{}]".format(path, i))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f"), path


@pytest.mark.parametrize("variant", ["plain", "device_eval", "icp", "hyp"])
def test_pred_eval_vsd_equals_the_host_on_single_renders(hip_lib, variant, tmp_path):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs
    from lib.utils.pose_error import vsd

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "glue"]
    n_hyp = 2 if variant == "hyp" else 1
    with_icp = variant == "icp"
    try:
        cfg.TEST.ICP_ITER = 2 if with_icp else 0
        cfg.TEST.HYP_NUM = n_hyp
        cfg.TEST.DEVICE_EVAL = variant == "device_eval"
        cfg.TEST.VSD = True
        cfg.TEST.VSD_TAU = [0.02, 0.05]
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
        data = SyntheticPairs(cfg, PAIRS, BATCH, seed=2333, subdiv=3)
        ev, rm = data.evaluator(), data.render_machine
        ref = Refiner(cfg, Predictor(cfg, params, BATCH * n_hyp), rm, BATCH)
        batches = list(data.test_batches())
        assert len(batches) == PAIRS // BATCH and all("depth_observed" in b for b in batches)
        if variant == "plain":   # an undetected pair (tester.py:419-445): pose_rendered = -1 everywhere
            batches[1]["src_pose"] = batches[1]["src_pose"].clone()
            batches[1]["src_pose"][1] = -1.0
        f_off, f_on = str(tmp_path / "off.pkl"), str(tmp_path / "on.pkl")
        cfg.TEST.VSD = False
        off = pred_eval(cfg, ref, batches, ev, result_file=f_off)
        cfg.TEST.VSD = True
        on = pred_eval(cfg, ref, batches, ev, result_file=f_on)
        # every output VSD off has is unchanged, and so is the result cache
        assert "vsd" not in off and "vsd" in on
        icp_vsd = on["icp"].pop("vsd") if with_icp else None
        _same(off, {k: v for k, v in on.items() if k != "vsd"})
        assert open(f_off, "rb").read() == open(f_on, "rb").read()
        # the host on planes rendered one pose at a time, in the order pred_eval fills its per-class lists
        K = np.asarray(rm.K, np.float64)
        delta, taus, cost = float(cfg.TEST.VSD_DELTA), [0.02, 0.05], cfg.TEST.VSD_COST
        n_it = 2

        def alone(c, pose):
            d = torch.zeros((1, 1, 480, 640), dtype=torch.float32, device=DEV)
            rm.render_batch(torch.tensor([c], dtype=torch.int32, device=DEV), _dev(np.asarray(pose, np.float32)[None]), depth=d, mask_thr=0.0)
            return d[0, 0].cpu().numpy()

        want = {k: [[[] for _ in range(n_it)] for _ in ev.classes] for k in ("vsd", "counts")}
        want_icp = {k: [[[]] for _ in ev.classes] for k in ("vsd", "counts")}
        for batch in batches:
            extra = {"hyp_poses": batch["hyp_poses"]} if batch.get("hyp_poses") is not None else {}
            ref.load(batch["image_observed"], batch["image_rendered"], batch["mask_observed"], batch["mask_rendered"], batch["src_pose"],
                     batch["class_index"], depth_observed=batch.get("depth_observed"), K=batch.get("K"), **extra)
            poses = ref.refine().cpu().numpy()
            sets = [(want, it, poses[it]) for it in range(n_it)]
            if with_icp:
                sets.append((want_icp, 0, ref.pose_icp.cpu().numpy()))
            cls = batch["class_index"].cpu().numpy().astype(int)
            obs = batch["depth_observed"].cpu().numpy().reshape(BATCH, 480, 640)
            gts = batch["pose_observed"].cpu().numpy().astype(np.float32)
            src = batch["src_pose"].cpu().numpy()
            for b in range(BATCH):
                d_gt = alone(cls[b], gts[b])
                for lists, it, p in sets:
                    if src[b].sum() == -12:
                        e, n = [1.0, 1.0], (0, 0, 0)
                    else:
                        d_est = alone(cls[b], p[b])
                        res = [vsd(d_est, d_gt, obs[b], K, delta, tau, cost) for tau in taus]
                        e, n = [r[0] for r in res], res[0][1]
                    lists["vsd"][cls[b]][it].append(e)
                    lists["counts"][cls[b]][it].append(list(n))

        def compare(got, exp, what):
            errs = got["errors"]
            assert errs["vsd"] == exp["vsd"], (what, errs["vsd"], exp["vsd"])   # step: exact
            for c in range(len(ev.classes)):
                for it in range(len(exp["counts"][c])):
                    have = [list(v) for v in zip(errs["visib_gt"][c][it], errs["union"][c][it], errs["inter"][c][it])]
                    assert have == exp["counts"][c][it], (what, c, it)
            assert sum(len(v[0]) for v in errs["vsd"]) == PAIRS and got["acc"].shape[2] == 2

        compare(on["vsd"], want, variant)
        if with_icp:
            compare(icp_vsd, want_icp, "icp row")
        if variant == "plain":
            lost = int(batches[1]["class_index"][1])
            assert [1.0, 1.0] in on["vsd"]["errors"]["vsd"][lost][1]
            some = [e for c in on["vsd"]["errors"]["vsd"] for e in c[1]]
            assert any(v[1] < 1.0 for v in some)   # the refined pairs overlap their ground truth
            short = dict(batches[0])
            del short["depth_observed"]
            with pytest.raises(KeyError, match="depth_observed"):
                pred_eval(cfg, ref, [short], ev)
    finally:
        cfg.TEST.ICP_ITER = 0
        cfg.TEST.HYP_NUM = 1
        cfg.TEST.DEVICE_EVAL = False
        cfg.TEST.VSD = False
        cfg.TEST.VSD_TAU = [0.02]
