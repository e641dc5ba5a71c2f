"""The step-cost VSD on BOP's grid on the device (csrc/vsd.hip dim_vsd_grid_errors, ops.vsd_grid_errors, pred_eval with TEST.BOP_VSD)
against lib/utils/pose_error.py vsd(..., "step") called once per tau on the host.

Bar: everything the kernel sums is an integer and the error is one float64 division of two of them, the host's own: errors (compared
as bits), counts and n_ge are equal exactly, whatever the tau count, the row order, the boxes or the state of the workspace."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_test_config  # noqa: E402
from test_gpu_vsd import ROWS, T_SETS, _box, _dev, _same, layout  # noqa: E402  (the golden planes as that file arranges them)

DEV = "cuda:0"
DELTA = 0.015
DIAMETERS = (0.05, 0.1, 0.2)                              # three classes
FRACS = [round(0.05 * k, 2) for k in range(1, 17)]        # BOP's ten fractions of the diameter, and six more for n_tau = 16
# the class of each golden row.  Row 2 (the two renders in each other's role) has few distinct costs and gets the smallest taus; with
# this choice every row's ten errors take at least 7 distinct values on the host (10, 7 and 7 for the first estimate)
ROW_CLASS = (1, 2, 0)


def ops():
    from lib.hip import ops as o

    return o


def table(n_tau, diameters=DIAMETERS):
    return np.array([[float(f) * float(d) for f in FRACS[:n_tau]] for d in diameters], dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(est, gt, obs, K, delta, taus):
    """-> (errors per tau from pose_error.vsd, (visib_gt, union, inter, drawn_gt), n_ge per tau from the host's masks)"""
    from lib.utils.misc import depth_im_to_dist_im
    from lib.utils.pose_error import vsd
    from lib.utils.visibility import estimate_visib_mask_est, estimate_visib_mask_gt

    res = [vsd(est, gt, obs, K, delta, float(tau), "step") for tau in taus]
    s_obs, s_gt, s_est = (depth_im_to_dist_im(d, K) for d in (obs, gt, est))
    vg = estimate_visib_mask_gt(s_obs, s_gt, delta)
    inter = vg & estimate_visib_mask_est(s_obs, s_est, vg, delta)
    c = np.abs(s_gt[inter] - s_est[inter])
    return [r[0] for r in res], list(res[0][1]) + [int((s_gt > 0).sum())], [int((c >= float(tau)).sum()) for tau in taus]


def host_stack(obs, gt, est, cams, classes, tab, delta=DELTA):
    """obs, gt: B planes; est: T x B planes; cams: B cameras -> errors (T,B,n_tau), counts (T,B,4), n_ge (T,B,n_tau)"""
    T, B, n_tau = len(est), len(gt), tab.shape[1]
    e, n, ge = np.zeros((T, B, n_tau)), np.zeros((T, B, 4), np.int32), np.zeros((T, B, n_tau), np.int32)
    for t in range(T):
        for b in range(B):
            e[t, b], n[t, b], ge[t, b] = host(est[t][b], gt[b], obs[b], cams[b], delta, tab[classes[b]])
    return e, n, ge


def run(obs, gt, est, K, classes, tab, cams=None, boxes=False, delta=DELTA, **kw):
    extra = dict(kw)
    if cams is not None:
        extra["K_per_sample"] = np.stack(cams)
    if boxes:
        extra["bbox_gt"] = _dev(np.array([_box(g) for g in gt], np.int32))
        extra["bbox_est"] = _dev(np.array([[_box(e) for e in row] for row in est], np.int32))
    e, n, ge = ops().vsd_grid_errors(_dev(np.stack(obs)), _dev(np.stack(gt)), _dev(np.stack([np.stack(row) for row in est])), K, delta,
                                     _dev(np.asarray(classes, np.int32)), tab, **extra)
    return e.cpu().numpy(), n.cpu().numpy(), ge.cpu().numpy()


def equal(got, want, what):
    e, n, ge = got
    assert np.array_equal(n, want[1]), (what, n.tolist(), want[1].tolist())
    assert np.array_equal(ge, want[2]), (what, ge.tolist(), want[2].tolist())
    assert np.array_equal(bits(e), bits(want[0])), (what, np.abs(e - want[0]).max())


# ------------------------------------------------------------------------------------------------------------------ golden planes
_REF = {}


def golden_ref(name):
    """the host's numbers for the layout of test_gpu_vsd.py at all 16 fractions, one camera and per-pair cameras -- computed once"""
    if name not in _REF:
        L = layout(name)
        tab = table(16)
        _REF[name] = {mode: host_stack(L["obs"], L["gt"], L["est"], cams, ROW_CLASS, tab)
                      for mode, cams in (("one", [L["K"]] * ROWS), ("per_pair", L["cams"]))}
        for e, _, _ in _REF[name].values():   # a wrong table row or a wrong tau shows: BOP's ten taus give at least 5 distinct errors
            assert all(len(set(e[t, b, :10].tolist())) >= 5 for t in range(T_SETS) for b in range(ROWS)), e[:, :, :10]
    return _REF[name]


def permuted(L, perm):
    return ([L["obs"][b] for b in perm], [L["gt"][b] for b in perm], [[L["est"][t][b] for b in perm] for t in range(T_SETS)],
            [L["cams"][b] for b in perm], [ROW_CLASS[b] for b in perm])


@pytest.mark.parametrize("per_pair", [False, True], ids=["one_K", "per_pair_K"])
@pytest.mark.parametrize("name", ["a", "b"], ids=["48x64", "50x63"])
def test_kernel_equals_the_host_on_the_golden_planes(hip_lib, name, per_pair):
    L = layout(name)
    ref = golden_ref(name)["per_pair" if per_pair else "one"]
    for n_tau in (1, 10, 16):
        tab = table(n_tau)
        for perm in ((0, 1, 2), (2, 0, 1)):
            obs, gt, est, cams, classes = permuted(L, perm)
            want = (ref[0][:, list(perm), :n_tau], ref[1][:, list(perm)], ref[2][:, list(perm), :n_tau])
            got = {boxes: run(obs, gt, est, L["K"], classes, tab, cams=cams if per_pair else None, boxes=boxes) for boxes in (False, True)}
            for boxes in (False, True):
                equal(got[boxes], want, (name, n_tau, perm, boxes))
            assert np.array_equal(bits(got[False][0]), bits(got[True][0]))   # boxes only skip pixels that add nothing


@pytest.mark.parametrize("name", ["a", "b"], ids=["48x64", "50x63"])
def test_absolute_taus_in_every_row_equal_the_existing_entry(hip_lib, name):
    L = layout(name)
    tab = np.tile(np.asarray(L["taus"], np.float64)[None], (3, 1))
    obs, gt, est, cams, classes = permuted(L, (0, 1, 2))
    e, n, _ = run(obs, gt, est, L["K"], classes, tab, cams=cams, boxes=True)
    boxes = dict(bbox_gt=_dev(np.array([_box(g) for g in gt], np.int32)),
                 bbox_est=_dev(np.array([[_box(x) for x in row] for row in est], np.int32)))
    e0, n0 = ops().vsd_errors(_dev(np.stack(obs)), _dev(np.stack(gt)), _dev(np.stack([np.stack(row) for row in est])), L["K"], L["delta"],
                              L["taus"], "step", K_per_sample=np.stack(cams), **boxes)
    assert L["delta"] == DELTA
    assert np.array_equal(bits(e), bits(e0.cpu().numpy())) and np.array_equal(n, n0.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ synthetic planes
def synthetic(H, W):
    """two pairs x two estimates of a tilted ellipse that fills most of the frame, in front of a wall with a plate over one corner; the
    estimates are shifted and rippled so that |S_gt - S_est| spreads over [0, 0.07] m"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    K = np.array([[300.0, 0, W / 2.0 - 0.5], [0, 300.0, H / 2.0 - 0.5], [0, 0, 1]])

    def ellipse(dx, dy, ripple, phase):
        inside = ((x - W / 2.0 - dx) / (0.46 * W)) ** 2 + ((y - H / 2.0 - dy) / (0.46 * H)) ** 2 < 1.0
        d = 0.9 + 0.0004 * x + 0.0007 * y + ripple * np.sin(0.05 * x + 0.11 * y + phase)
        return np.where(inside, d, 0.0).astype(np.float32)

    gt = [ellipse(0, 0, 0.0, 0.0), ellipse(3, -2, 0.01, 1.0)]
    est = [[ellipse(2, 1, 0.035, 0.3), ellipse(0, 0, 0.07, 2.0)], [ellipse(-3, 2, 0.02, 0.0), ellipse(5, -1, 0.05, 0.7)]]
    obs = []
    for g in gt:
        o = np.where(g > 0, g, np.float32(1.5)).astype(np.float32)
        o[: H // 3, : W // 4] = 0.4   # the plate, in front of the object
        obs.append(o)
    return obs, gt, est, K


@pytest.mark.parametrize("shape", [(70, 252), (67, 63)], ids=["70x252_vector", "67x63_scalar"])
def test_synthetic_planes_a_workgroup_walks_more_than_one_piece(hip_lib, shape):
    # 16 workgroups per pair take pieces of 256 lanes x 4 (vector) or x 1 (scalar) pixels in turn: 17.2 pieces of 1024 in 70 x 252 and
    # 16.5 pieces of 256 in 67 x 63, so workgroup 0 takes two and the last piece is cut
    H, W = shape
    assert (H * W) % (1024 if W % 4 == 0 else 256) != 0 and H * W > 16 * (1024 if W % 4 == 0 else 256)
    obs, gt, est, K = synthetic(H, W)
    classes, tab = (0, 1), table(10)   # diameters 0.05 and 0.1 m: 9 or 10 distinct errors per row
    want = host_stack(obs, gt, est, [K, K], classes, tab)
    assert all(len(set(want[0][t, b].tolist())) >= 5 for t in range(2) for b in range(2)), want[0]
    for boxes in (False, True):
        equal(run(obs, gt, est, K, classes, tab, boxes=boxes), want, (shape, boxes))


def test_a_cost_equal_to_tau_counts(hip_lib):
    # at the principal point S = d exactly, so c = |1.0 - 0.75| = 0.25 = 0.5 * 0.5: in at this tau (>=), out at the next larger double
    K = np.array([[100.0, 0, 3.0], [0, 100.0, 2.0], [0, 0, 1]])
    obs, gt, est = (np.zeros((6, 8), np.float32) for _ in range(3))
    obs[2, 3], gt[2, 3], est[2, 3] = 1.0, 1.0, 0.75
    tab = np.array([[0.5 * 0.5, np.nextafter(0.25, 1.0), 0.2]])
    assert tab[0, 0] == 0.25 and tab[0, 1] > 0.25
    e, n, ge = run([obs], [gt], [[est]], K, [0], tab)
    assert ge[0, 0].tolist() == [1, 0, 1] and n[0, 0].tolist() == [1, 1, 1, 1] and e[0, 0].tolist() == [1.0, 0.0, 1.0]
    equal((e, n, ge), host_stack([obs], [gt], [[est]], [K], [0], tab), "boundary")


# ------------------------------------------------------------------------------------------------------------------ degenerate inputs
def test_empty_planes_and_a_nan_pixel(hip_lib):
    from lib.utils.misc import depth_im_to_dist_im
    from lib.utils.visibility import estimate_visib_mask_est, estimate_visib_mask_gt

    L = layout("b")
    obs, gt, est = L["obs"][0], L["gt"][0], L["est"][0][0]
    zero = np.zeros_like(gt)
    tab = table(10)
    for planes in ((zero, zero, zero), (zero, gt, est)):      # everything empty; no observed depth at all
        e, n, ge = run([planes[0]], [planes[1]], [[planes[2]]], L["K"], [1], tab)
        assert e.tolist() == [[[1.0] * 10]] and n[0, 0, :3].tolist() == [0, 0, 0] and not ge.any()
    # one NaN in the observed depth, on a pixel of the intersection: it drops out of every count, as on the host
    s = [depth_im_to_dist_im(d, L["K"]) for d in (obs, gt, est)]
    vg = estimate_visib_mask_gt(s[0], s[1], DELTA)
    y, x = np.argwhere(vg & estimate_visib_mask_est(s[0], s[2], vg, DELTA))[7]
    holed = obs.copy()
    holed[y, x] = np.nan
    whole, want = host_stack([obs], [gt], [[est]], [L["K"]], [1], tab), host_stack([holed], [gt], [[est]], [L["K"]], [1], tab)
    assert (whole[1][0, 0, :3] - want[1][0, 0, :3]).tolist() == [1, 1, 1]
    equal(run([holed], [gt], [[est]], L["K"], [1], tab), want, "nan pixel")


def test_a_class_outside_the_table_gives_a_nan_row_and_leaves_the_others(hip_lib):
    L = layout("a")
    tab = table(10)
    obs, gt, est, cams, classes = permuted(L, (0, 1, 2))
    good = run(obs, gt, est, L["K"], classes, tab, cams=cams, boxes=True)
    for bad_row, bad in ((1, -1), (2, len(DIAMETERS)), (0, 1 << 30)):
        cl = list(classes)
        cl[bad_row] = bad
        e, n, ge = run(obs, gt, est, L["K"], cl, tab, cams=cams, boxes=True)
        keep = [b for b in range(ROWS) if b != bad_row]
        assert np.isnan(e[:, bad_row]).all() and not n[:, bad_row].any() and not ge[:, bad_row].any()
        equal((e[:, keep], n[:, keep], ge[:, keep]), (good[0][:, keep], good[1][:, keep], good[2][:, keep]), (bad_row, bad))


def test_bad_arguments_raise(hip_lib):
    from lib.hip import capi

    z = torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV)
    cls = torch.zeros((1,), dtype=torch.int32, device=DEV)
    K = np.eye(3)
    o = ops()
    assert o.VSD_GRID_MAX_TAU == 16
    for bad in ([[0.01] * 17], [[0.0, 0.01]], [[0.01, float("nan")]], [[0.01, float("inf")]], [0.01, 0.02], np.zeros((0, 3)), [[]]):
        with pytest.raises(ValueError):
            o.vsd_grid_errors(z, z, z, K, DELTA, cls, bad)
    with pytest.raises(ValueError):   # a device table must be float64
        o.vsd_grid_errors(z, z, z, K, DELTA, cls, torch.full((1, 2), 0.01, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        o.vsd_grid_errors(z, z, z, K, DELTA, cls, torch.full((1, 17), 0.01, dtype=torch.float64, device=DEV))
    with pytest.raises(AssertionError):   # one box without the other
        o.vsd_grid_errors(z, z, z, K, DELTA, cls, [[0.01]], bbox_gt=torch.zeros((1, 4), dtype=torch.int32, device=DEV))
    # the C entry's own checks: nothing is enqueued, the call returns an error
    tab = torch.full((1, 2), 0.01, dtype=torch.float64, device=DEV)
    work = o.vsd_grid_workspace(1, 1, DEV)
    e = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    n = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    ge = torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    k9 = np.ascontiguousarray(K.reshape(-1))
    box = torch.zeros((1, 4), dtype=torch.int32, device=DEV)

    def call(n_classes=1, n_tau=2, workspace=None, bbox_est=None, table=tab):
        return capi.lib().dim_vsd_grid_errors(z.data_ptr(), z.data_ptr(), z.data_ptr(), k9.ctypes.data, None, box.data_ptr(), bbox_est,
                                              cls.data_ptr(), table.data_ptr() if table is not None else None, n_classes, n_tau, 1, 1, 8, 8,
                                              DELTA, work.data_ptr() if workspace is None else workspace, e.data_ptr(), n.data_ptr(),
                                              ge.data_ptr(), o.current_stream())

    assert call(bbox_est=box.data_ptr()) == 0
    for kw in (dict(n_tau=0), dict(n_tau=17), dict(n_classes=0), dict(), dict(bbox_est=box.data_ptr(), table=None),
               dict(bbox_est=box.data_ptr(), workspace=work.data_ptr() + 4)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()


def test_a_dirty_workspace_and_a_replayed_graph_change_nothing(hip_lib):
    L = layout("a")
    tab = table(10)
    obs, gt, est, cams, classes = permuted(L, (0, 1, 2))
    want = run(obs, gt, est, L["K"], classes, tab, cams=cams, boxes=True)
    # exactly dim_vsd_grid_workspace_bytes between guards, at the documented minimum alignment (8 mod 16)
    arena = guard_arena.workspace(ops().lib().dim_vsd_grid_workspace_bytes(T_SETS, ROWS), 8, DEV)
    work = arena.view()
    assert work.dtype == torch.float64
    for fill in ("nan", "noise"):
        if fill == "nan":
            work.fill_(float("nan"))
        else:
            work.copy_(torch.randn(work.shape, dtype=torch.float64, device=DEV) * 1e6)
        equal(run(obs, gt, est, L["K"], classes, tab, cams=cams, boxes=True, workspace=work), want, fill)
        arena.check("dim_vsd_grid_errors workspace, {} before the call".format(fill))
    # captured once, replayed twice: everything the call reads is resident, nothing is allocated inside
    d_obs, d_gt, d_est = _dev(np.stack(obs)), _dev(np.stack(gt)), _dev(np.stack([np.stack(row) for row in est]))
    d_cls, d_tab, d_K = _dev(np.asarray(classes, np.int32)), _dev(tab), _dev(np.stack(cams).reshape(ROWS, 9))
    boxes = dict(bbox_gt=_dev(np.array([_box(g) for g in gt], np.int32)),
                 bbox_est=_dev(np.array([[_box(x) for x in row] for row in est], np.int32)))
    e = torch.zeros((T_SETS, ROWS, 10), dtype=torch.float64, device=DEV)
    n = torch.zeros((T_SETS, ROWS, 4), dtype=torch.int32, device=DEV)
    ge = torch.zeros((T_SETS, ROWS, 10), dtype=torch.int32, device=DEV)

    def launch():
        ops().vsd_grid_errors(d_obs, d_gt, d_est, L["K"], DELTA, d_cls, d_tab, K_per_sample=d_K, errors=e, counts=n, n_ge=ge,
                              workspace=work, **boxes)

    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        e.fill_(-1.0), n.fill_(-1), ge.fill_(-1), work.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        equal((e.cpu().numpy(), n.cpu().numpy(), ge.cpu().numpy()), want, "replay")


# ------------------------------------------------------------------------------------------------------------------ pred_eval
PAIRS, BATCH = 4, 2


@pytest.mark.parametrize("variant", ["plain", "device_eval", "icp", "hyp"])
def test_pred_eval_bop19_equals_the_host_on_single_renders(hip_lib, variant, tmp_path):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "glue"]
    n_hyp = 2 if variant == "hyp" else 1
    with_icp = variant == "icp"
    n_it = 2
    try:
        cfg.TEST.ICP_ITER = 2 if with_icp else 0
        cfg.TEST.HYP_NUM = n_hyp
        cfg.TEST.DEVICE_EVAL = variant == "device_eval"
        cfg.TEST.BOP = True
        cfg.TEST.BOP_SYM_STEP = 0.2
        cfg.TEST.BOP_VSD = True    # the batches carry depth_observed
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
        data = SyntheticPairs(cfg, PAIRS, BATCH, seed=2333, subdiv=3)
        ev, rm = data.evaluator(), data.render_machine
        ref = Refiner(cfg, Predictor(cfg, params, BATCH * n_hyp), rm, BATCH)
        batches = list(data.test_batches())
        assert len(batches) == PAIRS // BATCH and all("depth_observed" in b for b in batches)
        K_cfg = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float64).reshape(3, 3)
        if variant == "plain":   # an undetected pair: pose_rendered = -1 everywhere
            batches[1]["src_pose"] = batches[1]["src_pose"].clone()
            batches[1]["src_pose"][1] = -1.0
        if variant == "device_eval":   # every pair with a camera of its own
            for i, b in enumerate(batches):
                b["K"] = torch.from_numpy(np.stack([K_cfg * np.array([[1.0 + 0.05 * (i + j), 1, 1], [1, 1.0 + 0.05 * (i + j), 1], [1, 1, 1]])
                                                    for j in range(BATCH)]).astype(np.float32))
        f_off, f_on = str(tmp_path / "off.pkl"), str(tmp_path / "on.pkl")
        cfg.TEST.BOP_VSD = False
        off = pred_eval(cfg, ref, batches, ev, result_file=f_off)
        cfg.TEST.BOP_VSD = True
        on = pred_eval(cfg, ref, batches, ev, result_file=f_on)
        # every output BOP_VSD off has is unchanged, and so is the result cache
        assert "bop19" not in off["bop"] and "bop19" in on["bop"]
        got = on["bop"].pop("bop19")
        got_icp = on["icp"].pop("bop19") if with_icp else None
        _same(off, on)
        assert open(f_off, "rb").read() == open(f_on, "rb").read()

        # the host on planes rendered one pose at a time with the pair's camera, in the order pred_eval fills its per-class lists
        tab = ev.vsd_tau_table(cfg.TEST.BOP_VSD_TAU)
        assert tab.shape == (2, 10)

        def alone(c, pose, K):
            d = torch.zeros((1, 1, 480, 640), dtype=torch.float32, device=DEV)
            extra = {} if K is None else {"K": K.reshape(1, 9).to(DEV)}
            rm.render_batch(torch.tensor([c], dtype=torch.int32, device=DEV), _dev(np.asarray(pose, np.float32)[None]), depth=d, mask_thr=0.0,
                            **extra)
            return d[0, 0].cpu().numpy()

        keys = ("vsd_grid", "visib_gt", "union", "inter", "drawn_gt")
        want = {k: [[[] for _ in range(n_it)] for _ in ev.classes] for k in keys}
        want_icp = {k: [[[]] for _ in ev.classes] for k in keys}
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
                K_b = batch["K"][b] if batch.get("K") is not None else None
                K64 = K_b.numpy().astype(np.float64) if K_b is not None else np.asarray(rm.K, np.float64)
                d_gt = alone(cls[b], gts[b], K_b)
                for lists, it, p in sets:
                    if src[b].sum() == -12:
                        e, n = [1.0] * 10, [0, 0, 0, 0]
                    else:
                        e, n, _ = host(alone(cls[b], p[b], K_b), d_gt, obs[b], K64, float(cfg.TEST.BOP_VSD_DELTA), tab[cls[b]])
                    for k, v in zip(keys, [e] + list(n)):
                        lists[k][cls[b]][it].append(v)

        def compare(table_, exp, bop, what):
            errs = table_["errors"]
            assert set(errs) == set(keys) | {"mssd", "mspd"}
            for k in keys:
                assert errs[k] == exp[k], (what, k, errs[k], exp[k])   # integers and one division: exact
            assert errs["mssd"] == bop["errors"]["mssd"] and errs["mspd"] == bop["errors"]["mspd"]
            assert sum(len(v[0]) for v in errs["vsd_grid"]) == PAIRS
            # the table is the evaluator's on the host's errors (MSSD / MSPD: the lists of TEST.BOP, checked by test_gpu_bop.py)
            host_table = ev.evaluate_pose_bop19(cfg, dict(exp, mssd=bop["errors"]["mssd"], mspd=bop["errors"]["mspd"]))
            _same(host_table, {k: v for k, v in table_.items() if k != "errors"}, what)
            assert table_["recall_vsd"].shape == (2, len(exp["vsd_grid"][0]), 10, 10)

        compare(got, want, on["bop"], variant)
        if with_icp:
            compare(got_icp, want_icp, on["icp"]["bop"], "icp row")
        some = [e for c in got["errors"]["vsd_grid"] for e in c[n_it - 1]]
        assert any(v[-1] < 1.0 for v in some)   # the refined pairs overlap their ground truth
        # the key absent altogether (an older config): the outputs and the result cache of BOP_VSD: false
        f_absent = str(tmp_path / "absent.pkl")
        cfg.TEST.pop("BOP_VSD")
        cfg.TEST.__dict__.pop("BOP_VSD", None)
        assert "BOP_VSD" not in cfg.TEST
        absent = pred_eval(cfg, ref, batches, ev, result_file=f_absent)
        cfg.TEST.BOP_VSD = True
        _same(off, absent)
        assert open(f_off, "rb").read() == open(f_absent, "rb").read()
        # TEST.VSD next to it: out["vsd"] is what it is without the grid, and the grid what it is without TEST.VSD
        cfg.TEST.VSD, cfg.TEST.BOP_VSD = True, False
        vsd_only = pred_eval(cfg, ref, batches, ev)
        cfg.TEST.BOP_VSD = True
        both = pred_eval(cfg, ref, batches, ev)
        _same(vsd_only["vsd"], both["vsd"], "vsd")
        _same(got, both["bop"]["bop19"], "bop19")
        if with_icp:
            _same(vsd_only["icp"]["vsd"], both["icp"]["vsd"], "icp vsd")
            _same(got_icp, both["icp"]["bop19"], "icp bop19")
        cfg.TEST.VSD = False
        if variant == "plain":
            lost = int(batches[1]["class_index"][1])
            j = got["errors"]["vsd_grid"][lost][1].index([1.0] * 10)
            assert got["errors"]["drawn_gt"][lost][1][j] == 0 and got["count_targets"].sum() == (PAIRS - 1) * n_it
            short = dict(batches[0])
            del short["depth_observed"]
            with pytest.raises(KeyError, match="TEST.BOP_VSD needs the blob 'depth_observed'"):
                pred_eval(cfg, ref, [short], ev)
            cfg.TEST.BOP = False
            with pytest.raises(ValueError, match="TEST.BOP_VSD needs TEST.BOP"):
                pred_eval(cfg, ref, batches, ev)
    finally:
        cfg.TEST.ICP_ITER = 0
        cfg.TEST.HYP_NUM = 1
        cfg.TEST.DEVICE_EVAL = False
        cfg.TEST.VSD = False
        cfg.TEST.BOP = False
        cfg.TEST.BOP_VSD = False
        cfg.TEST.BOP_SYM_STEP = 0.01
