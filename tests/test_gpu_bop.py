"""The BOP symmetry-aware pose errors on the device (csrc/bop.hip, ops.bop_errors, pred_eval with TEST.BOP) against the float64
restatement tests/bop_reference.py (plain loops over the symmetries, the model point transformed twice).

The bar of every comparison: |dev - ref| <= 1e-10 * max(1, |ref|) in metres and pixels.  One float64 distance is rounded to ~1e-16
relative and maximum and minimum add nothing; composing pose_gt . S once per symmetry instead of transforming the point twice
moves a point by ~1e-16 relative.  tests/test_gpu_pose_errors.py records that the same kind of computation in float32 misses this bar
by 5e-10 .. 4e-8 m, so the bar separates the two.  best_sym is compared exactly on inputs whose best and second-best symmetry differ
by more than 1e-6 relative (asserted on the restatement's numbers for every row), ten orders above the rounding."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bop_reference as ref  # noqa: E402
import guard_arena  # noqa: E402
from loop_parity import moving_head  # noqa: E402
from scene import make_test_config  # noqa: E402

DEV = "cuda:0"
K_LM = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float64)
BAD_CLASS = 4
FLIP_X = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
# point tile 512 (two per lane), 16 workgroups per pose (8705 points: a second pass for workgroup 0, one point in its tile), symmetry
# chunk 64 (64: one full chunk, 65: one symmetry in the second, 315 / 630: five / ten chunks with a ragged last one)
SIZES = (1, 255, 256, 257, 511, 512, 513, 1025, 8705)
SETS = (2, 65, 64, 1, 3, 315, 2, 630, 3)
MAX_SYM = 630


def ops():
    from lib.hip import ops as o

    return o


def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _within_bar(dev, want, what):
    dev, want = np.asarray(dev, np.float64), np.asarray(want, np.float64)
    diff = np.abs(dev - want)
    bar = 1e-10 * np.maximum(1.0, np.abs(want))
    print("{}: max |dev - ref| = {:.3e} (bar 1e-10 * max(1, |ref|), largest ratio {:.3e})".format(what, diff.max(), (diff / bar).max()))
    assert np.all(diff <= bar), (what, float(diff.max()), int(np.argmax(diff / bar)))


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _mul(P, S):
    return np.concatenate([P[:, :3] @ S[:, :3], (P[:, :3] @ S[:, 3] + P[:, 3])[:, None]], axis=1)


def _gt_pose(rng):
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
    return np.concatenate([_rot(rng.normal(size=3), rng.uniform(0, 180)), t[:, None]], axis=1)


def _estimates(rng, gt, T, dtype):
    """(T,B,3,4): the ground truth turned by 0.5 .. 175 deg and moved by ~1.5 cm; float32 poses are rounded as the loop leaves them"""
    est = np.zeros((T,) + gt.shape)
    for t in range(T):
        for b in range(gt.shape[0]):
            est[t, b, :, :3] = _rot(rng.normal(size=3), rng.uniform(0.5, 175.0)) @ gt[b][:, :3]
            est[t, b, :, 3] = gt[b][:, 3] + rng.normal(size=3) * 0.015
    return est.astype(dtype)


def _random_set(rng, n):
    """the identity and n - 1 rigid transformations: any rotation, up to 1 cm"""
    out = [np.eye(4)[:3]]
    for _ in range(n - 1):
        out.append(np.concatenate([_rot(rng.normal(size=3), rng.uniform(5, 180)), rng.uniform(-0.01, 0.01, size=(3, 1))], axis=1))
    return np.stack(out)


def _set_of(rng, n):
    if n == 315:
        return ref.symmetry_set({"symmetries_continuous": [{"axis": [0.2, -0.1, 1.0], "offset": [0.004, 0.0, -0.003]}]}, 0.01)
    if n == 630:
        return ref.symmetry_set({"symmetries_discrete": [FLIP_X], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01)
    return _random_set(rng, n)


def _device_tables(pts, sets):
    off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
    soff = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    allp = np.concatenate([p for p in pts if len(p)]) if any(len(p) for p in pts) else np.zeros((0, 3))
    alls = np.concatenate([s for s in sets if len(s)]) if any(len(s) for s in sets) else np.zeros((0, 3, 4))
    return _dev(allp), _dev(off), _dev(alls), _dev(soff)


_TABLES = {}


def tables():
    """the nine classes and their symmetry sets, host and device: built once"""
    if not _TABLES:
        rng = np.random.default_rng(3)
        pts = [rng.uniform(-0.05, 0.05, size=(n, 3)) * np.array([1.0, 0.7, 0.4]) for n in SIZES]
        sets = [_set_of(rng, n) for n in SETS]
        assert [len(s) for s in sets] == list(SETS) and sorted(set(SETS)) == [1, 2, 3, 64, 65, 315, 630]
        _TABLES.update(pts=pts, sets=sets)
    if "dev" not in _TABLES and torch.cuda.is_available():
        _TABLES["dev"] = _device_tables(_TABLES["pts"], _TABLES["sets"])
    return _TABLES


def _reference(pts, sets, cls, est, gt, Ks):
    """-> errors (T,B,2), best (T,B,2), the smallest relative margin between the best and the second-best symmetry"""
    est = np.asarray(est, np.float64)
    e, s, worst = np.zeros(est.shape[:2] + (2,)), np.zeros(est.shape[:2] + (2,), dtype=np.int64), np.inf
    for t in range(est.shape[0]):
        for b in range(est.shape[1]):
            e[t, b], s[t, b], table = ref.mssd_mspd(est[t, b], gt[b], Ks[b], pts[cls[b]], sets[cls[b]])
            worst = min([worst] + ref.margin(table))
    return e, s, worst


CASES = {"f32_one_K": ((8, 0, 5, 3, 1, 7, 4), np.float32, False), "f32_per_pair_K": ((2, 6, 7, 0, 5, 4, 8), np.float32, True),
         "f64_per_pair_K": ((8, 0, 5, 3, 1, 7, 4), np.float64, True), "f64_one_K": ((2, 6, 7, 0, 5, 4, 8), np.float64, False)}
_CASES = {}


def case(name):
    """inputs and the restatement's numbers of one parity case, computed once and shared"""
    if name not in _CASES:
        draw, dtype, per_pair = CASES[name]
        tb = tables()
        rng = np.random.default_rng(41 + draw[0] + (dtype == np.float64))
        gt = np.stack([_gt_pose(rng) for _ in draw])
        est = _estimates(rng, gt, 2, dtype)
        cams = np.stack([K_LM * np.array([[s, 1, 1], [1, s, 1], [1, 1, 1]]) + np.array([[0, 0, dx], [0, 0, -dx], [0, 0, 0]])
                         for s, dx in zip(rng.uniform(0.8, 1.3, size=len(draw)), rng.uniform(-20, 20, size=len(draw)))])
        Ks = cams if per_pair else np.stack([K_LM] * len(draw))
        want, best, margin = _reference(tb["pts"], tb["sets"], draw, est, gt, Ks)
        _CASES[name] = dict(draw=draw, gt=gt, est=est, cams=cams if per_pair else None, want=want, best=best, margin=margin)
    return _CASES[name]


def _run(dev_tables, cls, est, gt, K=K_LM, max_sym=MAX_SYM, **kw):
    return ops().bop_errors(dev_tables[0], dev_tables[1], dev_tables[2], dev_tables[3], _dev(np.asarray(cls, np.int32)), _dev(est),
                            _dev(gt, torch.float64), K, max_sym, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
def test_all_nine_classes_and_seven_set_sizes_are_drawn():
    used = set(c for draw, _, _ in CASES.values() for c in draw)
    assert used == set(range(len(SIZES)))
    for dtype in (np.float32, np.float64):
        assert set(c for draw, dt, _ in CASES.values() if dt == dtype for c in draw) == set(range(len(SIZES)))


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_restatement(hip_lib, name):
    c = case(name)
    assert c["gt"][:, 2, 3].min() >= 0.6   # points within 7 cm of the origin, symmetries move them by <= 1 cm: every depth > 0.2 m
    assert c["margin"] > 1e-6, c["margin"]
    status = torch.zeros((7,), dtype=torch.int32, device=DEV)
    e, s = _run(tables()["dev"], c["draw"], c["est"], c["gt"], K_per_sample=c["cams"], status=status)
    e, s = e.cpu().numpy(), s.cpu().numpy()
    assert e.shape == (2, 7, 2) and e.dtype == np.float64 and s.dtype == np.int32 and status.cpu().tolist() == [0] * 7
    _within_bar(e[..., 0], c["want"][..., 0], name + " mssd")
    _within_bar(e[..., 1], c["want"][..., 1], name + " mspd")
    assert np.array_equal(s, c["best"]), (s.tolist(), c["best"].tolist())
    # the symmetries matter in these draws: a set of one scores the identity's column, the larger sets mostly another
    assert (c["best"] != 0).any()


def test_a_single_pose_set_without_the_T_axis(hip_lib):
    c = case("f32_one_K")
    e, s = _run(tables()["dev"], c["draw"], c["est"][1], c["gt"])
    assert e.shape == (7, 2) and s.shape == (7, 2)
    _within_bar(e.cpu().numpy(), c["want"][1], "one set")
    assert np.array_equal(s.cpu().numpy(), c["best"][1])


# ------------------------------------------------------------------------------------------------------------------ 2. the argmin
def test_two_identical_symmetries_the_smaller_index_wins(hip_lib):
    rng = np.random.default_rng(71)
    pts = [rng.uniform(-0.05, 0.05, size=(700, 3))]
    base = _random_set(rng, 3)
    sets = [np.stack([base[0], base[1], base[2], base[2].copy(), base[1].copy()])]
    assert sets[0][2].tobytes() == sets[0][3].tobytes()
    gt = np.stack([_gt_pose(rng) for _ in range(2)])
    near = np.concatenate([_rot([1, 2, 3], 0.7), np.full((3, 1), 0.002)], axis=1)
    est = np.stack([_mul(_mul(gt[0], base[2]), near), _mul(_mul(gt[1], base[1]), near)])   # next to gt . S_2 and to gt . S_1
    want, best, _ = _reference(pts, sets, (0, 0), est[None], gt, [K_LM] * 2)
    assert best[0].tolist() == [[2, 2], [1, 1]]
    e, s = _run(_device_tables(pts, sets), (0, 0), est, gt, max_sym=5)
    assert s.cpu().tolist() == [[2, 2], [1, 1]]
    _within_bar(e.cpu().numpy(), want[0], "identical symmetries")


def test_estimate_on_a_symmetry_of_a_cloud_of_revolution(hip_lib):
    syms = ref.symmetry_set({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01)
    assert len(syms) == 315
    rng = np.random.default_rng(73)
    seed = rng.uniform(0.01, 0.05, size=(4, 3))
    pts = [np.concatenate([seed @ m[:, :3].T + m[:, 3] for m in syms])]   # the orbit: invariant under the (cyclic) set
    ks = (7, 200, 314)
    gt = np.stack([_gt_pose(rng) for _ in ks])
    est = np.stack([_mul(g, syms[k]) for g, k in zip(gt, ks)])
    dev_tables = _device_tables(pts, [syms])
    e, s = _run(dev_tables, (0, 0, 0), est, gt, max_sym=315)
    e, s = e.cpu().numpy(), s.cpu().numpy()
    print("estimate = gt . S_k: mssd", e[:, 0], "mspd", e[:, 1])
    assert s.tolist() == [[k, k] for k in ks]
    assert np.all(e[:, 0] <= 1e-12) and np.all(e[:, 1] <= 1e-9)   # 1e-12 m at >= 0.6 m under a focal length of 572: < 1e-9 px
    # the identity alone sees the rotation: centimetres
    e1, s1 = _run(_device_tables(pts, [syms[:1]]), (0, 0, 0), est, gt, max_sym=1)
    assert np.all(e1.cpu().numpy()[:, 0] > 1e-3) and s1.cpu().tolist() == [[0, 0]] * 3


# ------------------------------------------------------------------------------------------------------------------ 3. NaN rows
def test_bad_empty_and_oversized_classes_give_nan_rows_only_there(hip_lib):
    rng = np.random.default_rng(79)
    pts = [rng.uniform(-0.05, 0.05, size=(300, 3)), np.zeros((0, 3)), rng.uniform(-0.05, 0.05, size=(40, 3)),
           rng.uniform(-0.05, 0.05, size=(40, 3))]
    sets = [_random_set(rng, 2), _random_set(rng, 2), _random_set(rng, 3), np.zeros((0, 3, 4))]
    dev_tables = _device_tables(pts, sets)
    cls = (0, 4, 0, -1, 1, 2, 3, 0)   # 4 and -1: outside the table; 1: no points; 2: three symmetries > max_sym 2; 3: no symmetries
    gt = np.stack([_gt_pose(rng) for _ in cls])
    est = _estimates(rng, gt, 2, np.float32)
    good = [b for b, c in enumerate(cls) if c == 0]
    want, best, _ = _reference(pts, sets, [0] * len(good), est[:, good], gt[good], [K_LM] * len(good))
    status = torch.zeros((len(cls),), dtype=torch.int32, device=DEV)
    e, s = _run(dev_tables, cls, est, gt, max_sym=2, status=status)
    e, s = e.cpu().numpy(), s.cpu().numpy()
    bad = [b for b in range(len(cls)) if b not in good]
    assert np.isnan(e[:, bad]).all() and (s[:, bad] == -1).all()
    assert status.cpu().tolist() == [BAD_CLASS if c in (4, -1) else 0 for c in cls]
    _within_bar(e[:, good], want, "rows next to NaN rows")
    assert np.array_equal(s[:, good], best)
    # with room for three symmetries class 2 is scored
    e3, _ = _run(dev_tables, cls, est, gt, max_sym=3)
    assert not np.isnan(e3.cpu().numpy()[:, 5]).any()
    # a non-finite pose stays in its own row
    est_nan = est.copy()
    est_nan[0, 0, 1, 2] = np.nan
    en, _ = _run(dev_tables, cls, est_nan, gt, max_sym=2)
    en = en.cpu().numpy()
    assert np.isnan(en[0, 0]).all() and np.array_equal(en[1], e[1], equal_nan=True) and np.array_equal(en[0, 2], e[0, 2])


def test_argument_errors_before_anything_is_enqueued(hip_lib):
    from lib.hip.capi import DeepIMHipError

    c = case("f32_one_K")
    tb = tables()["dev"]
    with pytest.raises(DeepIMHipError):
        _run(tb, c["draw"], c["est"], c["gt"], max_sym=0, workspace=torch.zeros(8, dtype=torch.float64, device=DEV))
    lib, z = hip_lib, torch.zeros(64, dtype=torch.float64, device=DEV)
    p = z.data_ptr()
    K = np.ascontiguousarray(K_LM.reshape(-1))
    for T, B, n_classes, max_sym, p32, p64 in ((0, 1, 1, 1, p, None), (1, 65536, 1, 1, p, None), (1, 1, 0, 1, p, None),
                                               (1, 1, 1, 1, p, p), (1, 1, 1, 1, None, None)):
        assert lib.dim_bop_errors(p, p, p, p, n_classes, p, p32, p64, p, K.ctypes.data, None, T, B, max_sym, p, p, None, None, None) != 0
    assert lib.dim_bop_errors(p, p, p, p, 1, p, p, None, p, K.ctypes.data, None, 1, 1, 1, None, p, None, None, None) != 0
    assert lib.dim_bop_errors_workspace_bytes(4, 16, 630) == 4 * 16 * 16 * 630 * 2 * 8


# ------------------------------------------------------------------------------------------------------------------ 4. determinism
def test_dirty_workspace_and_graph_replay_give_the_same_bits(hip_lib):
    c = case("f32_one_K")   # holds the 8705-point class: its first workgroup joins a second tile to what the first left
    tb = tables()["dev"]
    o = ops()
    first_e, first_s = _run(tb, c["draw"], c["est"], c["gt"])
    # exactly dim_bop_errors_workspace_bytes between guards, at the documented minimum alignment (8 mod 16)
    arena = guard_arena.workspace(o.lib().dim_bop_errors_workspace_bytes(2, 7, MAX_SYM), 8, DEV)
    work = arena.view()
    for fill in (float("nan"), -1.0e300, 1.0e300):
        work.fill_(fill)
        e, s = _run(tb, c["draw"], c["est"], c["gt"], workspace=work)
        arena.check("dim_bop_errors workspace, {} before the call".format(fill))
        assert np.array_equal(e.cpu().numpy().view(np.uint64), first_e.cpu().numpy().view(np.uint64)), fill
        assert np.array_equal(s.cpu().numpy(), first_s.cpu().numpy())
    # captured and replayed
    cls, est, gt = _dev(np.asarray(c["draw"], np.int32)), _dev(c["est"]), _dev(c["gt"], torch.float64)
    e_g = torch.zeros((2, 7, 2), dtype=torch.float64, device=DEV)
    s_g = torch.zeros((2, 7, 2), dtype=torch.int32, device=DEV)
    call = lambda: o.bop_errors(tb[0], tb[1], tb[2], tb[3], cls, est, gt, K_LM, MAX_SYM, errors=e_g, best_sym=s_g, workspace=work)  # noqa: E731
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        e_g.fill_(-7.0)
        s_g.fill_(-7)
        work.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e_g.cpu().numpy().view(np.uint64), first_e.cpu().numpy().view(np.uint64))
        assert np.array_equal(s_g.cpu().numpy(), first_s.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 5. pred_eval
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
def test_pred_eval_bop_off_against_on_and_the_host_errors(hip_lib, variant, tmp_path):
    from deepim.core.tester import Predictor, Refiner, pred_eval
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.evaluation import PoseEvaluator
    from lib.dataset.synthetic_pairs import SyntheticPairs
    from lib.utils import pose_error as pe

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = ["ape", "glue"]
    n_hyp = 2 if variant == "hyp" else 1
    with_icp = variant == "icp"
    n_it = 2
    try:
        cfg.TEST.ICP_ITER = 2 if with_icp else 0
        cfg.TEST.HYP_NUM = n_hyp
        cfg.TEST.DEVICE_EVAL = variant == "device_eval"
        cfg.TEST.BOP_SYM_STEP = 0.2   # 16 rotations
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=False)
        params = moving_head(sym.init_weights(cfg, {}, {}, seed=0), seed=1)
        data = SyntheticPairs(cfg, PAIRS, BATCH, seed=2333, subdiv=3)
        ev0, rm = data.evaluator(), data.render_machine
        ev = PoseEvaluator(ev0.classes, ev0._points, ev0._diameters, symmetries={
            "ape": {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0.01]}]}, "glue": {"symmetries_discrete": [FLIP_X]}})
        sets = ev.symmetry_sets(0.2)
        assert [len(s) for s in sets] == [16, 2]
        ref_ = Refiner(cfg, Predictor(cfg, params, BATCH * n_hyp), rm, BATCH)
        batches = list(data.test_batches())
        assert len(batches) == PAIRS // BATCH
        K_cfg = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float64).reshape(3, 3)
        if variant == "plain":   # an undetected pair (tester.py:419-445): pose_rendered = -1 everywhere
            batches[1]["src_pose"] = batches[1]["src_pose"].clone()
            batches[1]["src_pose"][1] = -1.0
        if variant == "device_eval":   # every pair with a camera of its own
            for i, b in enumerate(batches):
                b["K"] = torch.from_numpy(np.stack([K_cfg * np.array([[1.0 + 0.05 * (i + j), 1, 1], [1, 1.0 + 0.05 * (i + j), 1], [1, 1, 1]])
                                                    for j in range(BATCH)]).astype(np.float32))
        f_off, f_on = str(tmp_path / "off.pkl"), str(tmp_path / "on.pkl")
        cfg.TEST.BOP = False
        off = pred_eval(cfg, ref_, batches, ev, result_file=f_off)
        cfg.TEST.BOP = True
        on = pred_eval(cfg, ref_, batches, ev, result_file=f_on)
        # every output BOP off has is unchanged, and so is the result cache
        assert "bop" not in off and "bop" in on
        icp_bop = on["icp"].pop("bop") if with_icp else None
        _same(off, {k: v for k, v in on.items() if k != "bop"})
        for k in ("pose", "add", "arp_2d"):
            _same(off[k], on[k], k)
        assert open(f_off, "rb").read() == open(f_on, "rb").read()
        # the host functions on the poses pred_eval returned (the result cache), with each pair's camera, in list order
        with open(f_on, "rb") as f:
            _, _, poses_est, poses_gt = pickle.load(f)
        cams = [[] for _ in ev.classes]
        lost = [[] for _ in ev.classes]
        for b in batches:
            cls = b["class_index"].cpu().numpy().astype(int)
            for j in range(BATCH):
                cams[cls[j]].append(b["K"][j].numpy().astype(np.float64) if b.get("K") is not None else K_cfg)
                lost[cls[j]].append(bool(b["src_pose"][j].sum().item() == -12))
        errs = on["bop"]["errors"]
        assert set(errs) == {"mssd", "mspd", "sym_mssd", "sym_mspd"}
        got, want, n_lost = [], [], 0
        for c, name in enumerate(ev.classes):
            for it in range(n_it):
                assert len(errs["mssd"][c][it]) == len(poses_est[c][it]) == len(cams[c])
                for j, (e, g) in enumerate(zip(poses_est[c][it], poses_gt[c][it])):
                    have = (errs["mssd"][c][it][j], errs["mspd"][c][it][j])
                    if lost[c][j]:
                        assert have == (float("inf"), float("inf")) and errs["sym_mssd"][c][it][j] == -1 and errs["sym_mspd"][c][it][j] == -1
                        n_lost += 1
                        continue
                    e, g = np.asarray(e, np.float64), np.asarray(g, np.float64)
                    got.append(have)
                    want.append((pe.mssd(e[:, :3], e[:, 3], g[:, :3], g[:, 3], ev._points[name], sets[c]),
                                 pe.mspd(e[:, :3], e[:, 3], g[:, :3], g[:, 3], cams[c][j], ev._points[name], sets[c])))
                    assert 0 <= errs["sym_mssd"][c][it][j] < len(sets[c]) and 0 <= errs["sym_mspd"][c][it][j] < len(sets[c])
        assert n_lost == (n_it if variant == "plain" else 0) and len(got) + n_lost == PAIRS * n_it
        got, want = np.array(got), np.array(want)
        _within_bar(got[:, 0], want[:, 0], variant + " mssd")
        _within_bar(got[:, 1], want[:, 1], variant + " mspd")
        assert on["bop"]["recall_mssd"].shape == (2, n_it, 10) and len(on["bop"]["overall"]) == n_it
        if with_icp:
            p_icp = on["icp"]  # the ICP row: one iteration, scored like the others
            assert len(icp_bop["errors"]["mssd"]) == 2 and sum(len(v[0]) for v in icp_bop["errors"]["mssd"]) == PAIRS
            assert all(np.isfinite(v) for c in icp_bop["errors"]["mssd"] for v in c[0]) and "pose" in p_icp
            assert icp_bop["recall_mspd"].shape == (2, 1, 10)
    finally:
        cfg.TEST.ICP_ITER = 0
        cfg.TEST.HYP_NUM = 1
        cfg.TEST.DEVICE_EVAL = False
        cfg.TEST.BOP = False
        cfg.TEST.BOP_SYM_STEP = 0.01
