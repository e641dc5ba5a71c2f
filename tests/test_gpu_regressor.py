"""Per-class pose regressors (network.REGRESSOR_NUM = K > 1) on the device.

Kernels (dim_pose_head_fwd_cls, dim_pose_head_bwd_cls, dim_se3_dist_loss_grad_cls, dim_fc_wgrad_cls through their ops wrappers), on the
seeded inputs of tests/regressor_reference.py: (a) bit equality with the shared-head op on class slices / sub-batches, as the C
contract states it, (b) inside the float64 bars of the reference, (c) K = 1 without class_index bit equal to the shared-head op.
Then the refinement loop (Refiner eager / captured / replayed with other classes, and the C loop object) against the oracle run with
each pair's class slice, and one training iteration plus an SGD step with a class absent from the batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import regressor_reference as G  # noqa: E402
import train_head_reference as R  # noqa: E402
from loop_parity import check_loop, moving_head, oracle_free_and_forced  # noqa: E402
from scene import make_test_config, make_train_config, make_train_scene  # noqa: E402

DEV = "cuda:0"
BAD_CLASS = 4      # DIM_STATUS_BAD_CLASS
KERNEL_CASES = [pytest.param(*c, id="B{}-K{}".format(c[0], c[1])) for c in G.CASES]


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if a.dtype == np.int32 else a.astype(np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def inside(got, ref, what):
    want, bar = ref
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    assert np.all(np.isfinite(got)), what
    ratio = R.worst_ratio(got, want, bar)
    print("{}: worst error {:.3f} bars".format(what, ratio))
    assert ratio <= 1.0, "{}: {:.3g} x its bar".format(what, ratio)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    assert np.array_equal(bits(got), bits(want)), what


def head_params(inp, unaligned=False):
    """the seven parameter arrays on the device; unaligned: as views of one flat blob that start 4 bytes past a 16-byte boundary (fc7_w
    and so every row of it: pose_head_kernel's scalar-load path)"""
    names = (("fc7_weight", "fc7_w"), ("fc7_bias", "fc7_b"), ("rot_weight", "rot_w"), ("rot_bias", "rot_b"), ("trans_weight", "trans_w"),
             ("trans_bias", "trans_b"))
    if not unaligned:
        return {k: dev(inp[s]) for k, s in names}
    blob = torch.zeros(1 + sum(inp[s].size for _, s in names), dtype=torch.float32, device=DEV)
    assert blob.data_ptr() % 16 == 0
    p, off = {}, 1
    for k, s in names:
        p[k] = blob[off:off + inp[s].size].view(inp[s].shape)
        p[k].copy_(dev(inp[s]))
        off += inp[s].size
    assert p["fc7_weight"].data_ptr() % 16 == 4
    return p


def class_slice(p, c):
    """class c's head as the shared-head ops read it: row views of the K-fold arrays, nothing copied"""
    q = dict(p)
    q["rot_weight"], q["rot_bias"] = p["rot_weight"][4 * c:4 * c + 4], p["rot_bias"][4 * c:4 * c + 4]
    q["trans_weight"], q["trans_bias"] = p["trans_weight"][3 * c:3 * c + 3], p["trans_bias"][3 * c:3 * c + 3]
    return q


def groups(classes, K):
    cls = np.asarray(classes)
    return [(c, np.nonzero(cls == c)[0]) for c in range(K) if (cls == c).any()]


def sub(t, idx):
    return t[torch.as_tensor(idx, device=DEV)].contiguous()


# ------------------------------------------------------------------------------------------------ forward
def _fwd(ops, inp, K, p, status=None):
    B = inp["fc6"].shape[0]
    se3, fc7 = torch.full((B, 7), 7.0, device=DEV), torch.full((B, 256), 7.0, device=DEV)
    ops.pose_head_fwd_cls(dev(inp["fc6"]), p, dev(inp["class_index"]), K, dev(inp["zoom_factor"]), se3=se3, fc7_out=fc7, status=status)
    return host(se3), host(fc7)


@pytest.mark.parametrize("B,K,classes,unaligned", [pytest.param(*c, False, id="B{}-K{}".format(c[0], c[1])) for c in G.CASES]
                         + [pytest.param(*G.CASES[1], True, id="B5-K3-unaligned-blob")])
def test_pose_head_fwd_cls(ops, B, K, classes, unaligned):
    inp = G.inputs(B, K, classes)
    p = head_params(inp, unaligned)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    se3, fc7 = _fwd(ops, inp, K, p, status)
    assert not host(status).any()
    ref = G.run_all(inp, K)["fwd"]
    inside(se3, ref["se3"], "fwd se3 B={} K={}".format(B, K))                                           # (b)
    inside(fc7, ref["fc7"], "fwd fc7 B={} K={}".format(B, K))
    fc6, zf = dev(inp["fc6"]), dev(inp["zoom_factor"])
    for c, idx in groups(classes, K):                                                                   # (a)
        f7 = torch.full((len(idx), 256), 7.0, device=DEV)
        want = ops.pose_head_fwd(sub(fc6, idx), class_slice(p, c), sub(zf, idx), fc7_out=f7)
        same_bits(se3[idx], host(want), "fwd se3 class {}".format(c))
        same_bits(fc7[idx], host(f7), "fwd fc7 class {}".format(c))


def test_pose_head_fwd_one_regressor_is_the_shared_kernel(ops):
    B = 5
    inp = G.inputs(B, 1, (0,) * B)
    p = head_params(inp)
    se3 = torch.full((B, 7), 7.0, device=DEV)
    ops.pose_head_fwd_cls(dev(inp["fc6"]), p, None, 1, dev(inp["zoom_factor"]), se3=se3)                # (c)
    want = ops.pose_head_fwd(dev(inp["fc6"]), p, dev(inp["zoom_factor"]))
    same_bits(host(se3), host(want), "K = 1")
    inside(host(se3), G.run_all(inp, 1, class_index=None)["fwd"]["se3"], "fwd se3 K=1")


# ------------------------------------------------------------------------------------------------ backward
def _bwd(ops, inp, K, p, cls):
    B = inp["fc6a"].shape[0]
    out = [torch.full(s, 7.0, device=DEV) for s in ((B, 4), (B, 256), (B, 256))]
    ops.pose_head_bwd_cls(dev(inp["fc6a"]), dev(inp["fc7"]), dev(inp["rot_raw"]), dev(inp["d_rot_norm"]), dev(inp["d_trans"]), p, cls, K, *out)
    return [host(t) for t in out]


@pytest.mark.parametrize("B,K,classes", KERNEL_CASES)
def test_pose_head_bwd_cls(ops, B, K, classes):
    inp = G.inputs(B, K, classes)
    p = head_params(inp)
    got = dict(zip(("d_rot", "dz7", "dz6"), _bwd(ops, inp, K, p, dev(inp["class_index"]))))
    ref = G.run_all(inp, K)["bwd"]
    for k in got:
        inside(got[k], ref[k], "bwd {} B={} K={}".format(k, B, K))                                      # (b)
    t = {k: dev(inp[k]) for k in ("fc6a", "fc7", "rot_raw", "d_rot_norm", "d_trans")}
    for c, idx in groups(classes, K):                                                                   # (a)
        want = [torch.full((len(idx), n), 7.0, device=DEV) for n in (4, 256, 256)]
        ops.pose_head_bwd(sub(t["fc6a"], idx), sub(t["fc7"], idx), sub(t["rot_raw"], idx), sub(t["d_rot_norm"], idx), sub(t["d_trans"], idx),
                          class_slice(p, c), *want)
        for k, w in zip(("d_rot", "dz7", "dz6"), want):
            same_bits(got[k][idx], host(w), "bwd {} class {}".format(k, c))


def test_pose_head_bwd_one_regressor_is_the_shared_kernel(ops):
    B = 5
    inp = G.inputs(B, 1, (0,) * B)
    p = head_params(inp)
    got = _bwd(ops, inp, 1, p, None)                                                                    # (c)
    want = [torch.full(s, 7.0, device=DEV) for s in ((B, 4), (B, 256), (B, 256))]
    ops.pose_head_bwd(dev(inp["fc6a"]), dev(inp["fc7"]), dev(inp["rot_raw"]), dev(inp["d_rot_norm"]), dev(inp["d_trans"]), p, *want)
    for g, w in zip(got, want):
        same_bits(g, host(w), "K = 1")


# ------------------------------------------------------------------------------------------------ SE3_DIST_LOSS
def _dist(ops, inp, K, p, cls, kind, idx=None, cls_op=True):
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    d_rot, d_zt, sums = dev(pick(inp["d_rot_prior"])), dev(pick(inp["d_zt_prior"])), dev(np.array(inp["sums_prior"]))
    args = (dev(pick(inp["rot_norm"])), dev(pick(inp["rot_gt"])), dev(pick(inp["fc7_dist"])), p)
    tail = (dev(pick(inp["zt_gt"])), d_rot, d_zt, G.DIST_ARGS["lw_rot"], G.DIST_ARGS["lw_trans"])
    kw = dict(trans_loss_type=kind, smooth_l1_scalar=G.DIST_ARGS["s"], loss_sums2=sums)
    if cls_op:
        ops.se3_dist_loss_grad_cls(*args, cls, K, *tail, **kw)
    else:
        ops.se3_dist_loss_grad(*args, *tail, **kw)
    return host(d_rot), host(d_zt), host(sums)


@pytest.mark.parametrize("kind", R.LOSS_TYPES)
@pytest.mark.parametrize("B,K,classes", KERNEL_CASES)
def test_se3_dist_loss_grad_cls(ops, B, K, classes, kind):
    inp = G.inputs(B, K, classes)
    p = head_params(inp)
    d_rot, d_zt, sums = _dist(ops, inp, K, p, dev(inp["class_index"]), kind)
    ref = G.run_all(inp, K, trans_type=kind)["dist"]
    for name, got, prior in (("d_rot_norm", d_rot, inp["d_rot_prior"]), ("d_zoom_trans", d_zt, inp["d_zt_prior"])):     # (b)
        want, bar = ref[name]
        inside(R.f64(got) - R.f64(prior), (want - R.f64(prior), bar), "dist {} increment {} B={} K={}".format(name, kind, B, K))
    inside(sums[0], ref["rot_loss_sum"], "dist rot loss sum")
    inside(sums[1], ref["trans_loss_sum"], "dist trans loss sum")
    for c, idx in groups(classes, K):                                                                   # (a)
        w_rot, w_zt, _ = _dist(ops, inp, K, class_slice(p, c), None, kind, idx=idx, cls_op=False)
        same_bits(d_rot[idx], w_rot, "dist d_rot_norm class {}".format(c))
        same_bits(d_zt[idx], w_zt, "dist d_zoom_trans class {}".format(c))


def test_se3_dist_loss_grad_one_regressor_is_the_shared_kernel(ops):
    B = 5
    inp = G.inputs(B, 1, (0,) * B)
    p = head_params(inp)
    got = _dist(ops, inp, 1, p, None, "smooth_L1")                                                      # (c)
    want = _dist(ops, inp, 1, p, None, "smooth_L1", cls_op=False)
    same_bits(got[0], want[0], "K = 1 d_rot_norm")
    same_bits(got[1], want[1], "K = 1 d_zoom_trans")


# ------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("which", ["rot", "trans"])
@pytest.mark.parametrize("B,K,classes", KERNEL_CASES)
def test_fc_wgrad_cls(ops, B, K, classes, which):
    inp = G.inputs(B, K, classes)
    dz = inp["d_rot_norm"] if which == "rot" else inp["d_trans"]
    Out = dz.shape[1]
    nan = float("nan")
    dW, db = torch.full((K * Out, 256), nan, device=DEV), torch.full((K * Out,), nan, device=DEV)
    ops.fc_wgrad_cls(dev(dz), dev(inp["fc7"]), dev(inp["class_index"]), K, dW, db)
    dW, db = host(dW), host(db)
    assert np.all(np.isfinite(dW)) and np.all(np.isfinite(db))                                          # every element written
    ref = G.run_all(inp, K)["wgrad" if which == "rot" else "wgrad_trans"]
    inside(dW, ref["dW"], "wgrad {} dW B={} K={}".format(which, B, K))                                  # (b); absent classes: bar 0
    inside(db, ref["db"], "wgrad {} db B={} K={}".format(which, B, K))
    present = dict(groups(classes, K))
    tz, tx = dev(dz), dev(inp["fc7"])
    for c in range(K):                                                                                  # (a)
        rows = slice(c * Out, (c + 1) * Out)
        if c not in present:
            assert not bits(dW[rows]).any() and not bits(db[rows]).any(), c      # +0.0 exactly
            continue
        w, b = torch.full((Out, 256), nan, device=DEV), torch.full((Out,), nan, device=DEV)
        ops.fc_wgrad(sub(tz, present[c]), sub(tx, present[c]), w, b)
        same_bits(dW[rows], host(w), "wgrad dW class {}".format(c))
        same_bits(db[rows], host(b), "wgrad db class {}".format(c))
    only_w = torch.full((K * Out, 256), nan, device=DEV)
    ops.fc_wgrad_cls(dev(dz), dev(inp["fc7"]), dev(inp["class_index"]), K, only_w)                       # db = NULL
    same_bits(host(only_w), dW, "wgrad without db")


def test_fc_wgrad_one_regressor_is_the_shared_kernel(ops):
    B = 5
    inp = G.inputs(B, 1, (0,) * B)
    got = [torch.full((4, 256), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)]
    want = [torch.full((4, 256), 7.0, device=DEV), torch.full((4,), 7.0, device=DEV)]
    ops.fc_wgrad_cls(dev(inp["d_rot_norm"]), dev(inp["fc7"]), None, 1, *got)                            # (c)
    ops.fc_wgrad(dev(inp["d_rot_norm"]), dev(inp["fc7"]), *want)
    for g, w in zip(got, want):
        same_bits(host(g), host(w), "K = 1")


# ------------------------------------------------------------------------------------------------ class outside [0, K), bad arguments
def test_class_outside_the_table(ops):
    B, K, classes = G.BAD_CASE
    inp = G.inputs(B, K, classes)
    p = head_params(inp)
    ref = G.run_all(inp, K, trans_type="L2")
    bad = np.array([not 0 <= c < K for c in classes])
    status = torch.as_tensor(np.array([1, 1, 0, 0], np.int32)).to(DEV)
    se3, fc7 = _fwd(ops, inp, K, p, status)
    assert host(status).tolist() == [1 | BAD_CLASS, 1, BAD_CLASS, 0]                                     # OR-ed in, other bits kept
    same_bits(se3[bad], np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (int(bad.sum()), 1)), "identity delta")
    inside(se3, ref["fwd"]["se3"], "fwd se3 with bad classes")
    inside(fc7, ref["fwd"]["fc7"], "fwd fc7 with bad classes")                                          # fc7 as usual
    se3_2, _ = _fwd(ops, inp, K, p, None)                                                               # status = NULL
    same_bits(se3_2, se3, "fwd without status")
    cls = dev(inp["class_index"])
    got = dict(zip(("d_rot", "dz7", "dz6"), _bwd(ops, inp, K, p, cls)))
    for k in got:
        assert not bits(got[k][bad]).any(), k                                                           # zero rows
        inside(got[k], ref["bwd"][k], "bwd {} with bad classes".format(k))
    d_rot, d_zt, sums = _dist(ops, inp, K, p, cls, "L2")
    same_bits(d_rot[bad], inp["d_rot_prior"][bad], "dist: nothing added to d_rot_norm")
    same_bits(d_zt[bad], inp["d_zt_prior"][bad], "dist: nothing added to d_zoom_trans")
    inside(R.f64(d_zt) - R.f64(inp["d_zt_prior"]), (ref["dist"]["d_zoom_trans"][0] - R.f64(inp["d_zt_prior"]), ref["dist"]["d_zoom_trans"][1]),
           "dist d_zoom_trans with bad classes")
    inside(sums[0], ref["dist"]["rot_loss_sum"], "dist rot loss sum without the bad samples")
    inside(sums[1], ref["dist"]["trans_loss_sum"], "dist trans loss sum without the bad samples")
    dW, db = torch.full((K * 4, 256), float("nan"), device=DEV), torch.full((K * 4,), float("nan"), device=DEV)
    ops.fc_wgrad_cls(dev(inp["d_rot_norm"]), dev(inp["fc7"]), cls, K, dW, db)
    inside(host(dW), ref["wgrad"]["dW"], "wgrad dW skips the bad samples")
    inside(host(db), ref["wgrad"]["db"], "wgrad db skips the bad samples")
    assert not bits(host(dW)[8:12]).any()                                                               # class 2: absent


def test_argument_errors(ops):
    from lib.hip.capi import current_stream, dptr

    f32, lib = torch.float32, ops.lib()
    B, K, classes = G.CASES[1]
    inp = G.inputs(B, K, classes)
    p = head_params(inp)
    t = {k: dev(inp[k]) for k in ("fc6", "zoom_factor", "fc6a", "fc7", "rot_raw", "d_rot_norm", "d_trans", "rot_norm", "rot_gt", "fc7_dist", "zt_gt")}
    cls = dev(inp["class_index"])
    out = {k: torch.full(s, 7.0, device=DEV) for k, s in (("se3", (B, 7)), ("d_rot", (B, 4)), ("dz7", (B, 256)), ("dz6", (B, 256)),
                                                           ("dW", (K * 4, 256)))}
    P = lambda k: dptr(p[k], f32)  # noqa: E731
    D = lambda k: dptr(t[k], f32)  # noqa: E731
    O = lambda k: dptr(out[k], f32)  # noqa: E731
    for n_reg, ci in ((0, dptr(cls, torch.int32)), (-3, dptr(cls, torch.int32)), (K, None)):
        calls = (
            lambda: lib.dim_pose_head_fwd_cls(D("fc6"), P("fc7_weight"), P("fc7_bias"), P("rot_weight"), P("rot_bias"), P("trans_weight"),
                                              P("trans_bias"), ci, n_reg, D("zoom_factor"), O("se3"), None, None, B, current_stream()),
            lambda: lib.dim_pose_head_bwd_cls(D("fc6a"), D("fc7"), D("rot_raw"), D("d_rot_norm"), D("d_trans"), P("fc7_weight"), P("rot_weight"),
                                              P("trans_weight"), ci, n_reg, O("d_rot"), O("dz7"), O("dz6"), B, current_stream()),
            lambda: lib.dim_se3_dist_loss_grad_cls(D("rot_norm"), D("rot_gt"), D("fc7_dist"), P("trans_weight"), P("trans_bias"), ci, n_reg,
                                                   D("zt_gt"), O("d_rot"), O("se3"), B, 1.0, 1.0, 1, 3.0, None, current_stream()),
            lambda: lib.dim_fc_wgrad_cls(D("d_rot_norm"), D("fc7"), ci, n_reg, O("dW"), None, B, 4, 256, current_stream()),
        )
        for i, call in enumerate(calls):
            assert call() == -1, (n_reg, i)                                                             # DIM_ERR_ARG
            assert (b"must be >= 1" if n_reg < 1 else b"class_index is required") in lib.dim_last_error()
    for v in out.values():
        assert np.all(host(v) == 7.0)                                                                   # nothing was launched


# ------------------------------------------------------------------------------------------------ refinement loop
LOOP_SEED = 126        # tests/scene.py draws the classes [1, 0, 1] for three pairs of two models from it
LOOP_KEYS = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose")


def _two_class_config(cfg):
    cfg.dataset.class_name = ["ape", "can"]
    cfg.network.REGRESSOR_NUM = 2
    return cfg


def _two_heads(cfg, seeds=(1, 2)):
    """-> (K-fold params, [the shared-head parameter dict of class 0, of class 1]): each class's slice is a moving head of its own seed"""
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    assert params["rot_weight"].shape == (8, 256) and params["trans_weight"].shape == (6, 256)
    per_class = []
    for c, seed in enumerate(seeds):
        p = dict(params)
        for k, rows in (("rot_weight", 4), ("rot_bias", 4), ("trans_weight", 3), ("trans_bias", 3)):
            p[k] = params[k][rows * c:rows * (c + 1)].copy()
        per_class.append(moving_head(p, seed=seed))
    for k in ("rot_weight", "rot_bias", "trans_weight", "trans_bias"):
        params[k] = np.concatenate([p[k] for p in per_class])
    return params, per_class


@pytest.fixture(scope="module")
def loop_scene(hip_lib):
    scene = make_train_scene(B=3, seed=LOOP_SEED, subdiv=3, n_models=2)
    assert scene["blobs"]["class_index"].tolist() == [1, 0, 1]
    return scene


def _check_pairs(cfg, per_class, scene, classes, poses, se3, tag, step_tol=2e-5):
    bl = scene["blobs"]
    for b, c in enumerate(classes):
        blobs_b = {k: bl[k][b:b + 1] for k in LOOP_KEYS}
        mesh = scene["models"][c]
        free, forced = oracle_free_and_forced(per_class[c], mesh, blobs_b, scene["K"], cfg.network.PIXEL_MEANS, poses[:, b], test_iter=2)
        pts = mesh[0].astype(np.float64)
        check_loop(bl["src_pose"][b], poses[:, b], se3[:, b], free, forced, pts, np.linalg.norm(pts.max(0) - pts.min(0)),
                   tag="{} pair {} class {}".format(tag, b, c), step_tol=step_tol)


def test_refine_loop_picks_each_pairs_head(loop_scene):
    from deepim.core.tester import Predictor, Refiner
    from lib.hip.refiner_capi import CRefiner
    from lib.render_hip.render_py_multi import Render_Py
    from oracle import refine as orefine

    step_tol = 2e-5       # check_loop's own
    scene, bl = loop_scene, loop_scene["blobs"]
    cfg = _two_class_config(make_test_config(test_iter=2))
    try:
        params, per_class = _two_heads(cfg)
        B, classes = 3, [1, 0, 1]
        # negative control, on the host before the inputs are used: a class-1 pair stepped with class 0's slice lands more than 10 bars
        # of check_loop's step check away from where its own slice puts it
        z3, o3 = np.zeros(3), np.ones(3)
        blobs_0 = {k: bl[k][0:1] for k in LOOP_KEYS}
        own, other = (orefine.refine_pair(per_class[c], scene["models"][1], blobs_0, scene["K"], cfg.network.PIXEL_MEANS, z3, o3, "CAMERA",
                                          test_iter=1) for c in (1, 0))
        src = np.asarray(bl["src_pose"][0], np.float64)
        d_own, d_other = np.asarray(own[0][0], np.float64) - src, np.asarray(other[0][0], np.float64) - src
        miss = float(np.abs(d_own - d_other).max()) / (step_tol * max(1.0, float(np.abs(d_own).max())))
        print("class 0's head on a class-1 pair misses the step bar {:.0f} x".format(miss))
        assert miss > 10.0, miss
        rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
        load = lambda r, cls: r.load(bl["image_observed"], bl["image_rendered"], bl["mask_observed"], bl["mask_rendered"], bl["src_pose"],  # noqa: E731
                                     np.asarray(cls, np.int32))
        # the Python-driven loop, eager
        ref = Refiner(cfg, Predictor(cfg, params, B), rm, B, capture_graph=False)
        load(ref, classes)
        poses = ref.refine().cpu().numpy().copy()
        se3 = ref.se3_iter.cpu().numpy().copy()
        assert not (ref.status_iter.cpu().numpy() & BAD_CLASS).any()
        _check_pairs(cfg, per_class, scene, classes, poses, se3, "eager")
        # the C loop object on the same batch
        cref = CRefiner(cfg, params, rm, B)
        dev_bl = {k: torch.as_tensor(np.ascontiguousarray(bl[k])).to(DEV) for k in LOOP_KEYS + ("class_index",)}
        poses_c = cref.refine(*[dev_bl[k] for k in LOOP_KEYS + ("class_index",)]).cpu().numpy().copy()
        for it in range(2):
            prev = bl["src_pose"] if it == 0 else poses[it - 1]
            for b in range(B):
                bar = step_tol * max(1.0, float(np.abs(poses[it, b] - prev[b]).max()))
                assert float(np.abs(poses_c[it, b] - poses[it, b]).max()) <= bar, (it, b)
        cref.close()
        # captured: [1, 0, 1], then other classes written into the resident buffer and the SAME graph replayed
        gref = Refiner(cfg, Predictor(cfg, params, B), rm, B, capture_graph=True)
        load(gref, classes)
        poses_g = gref.refine().cpu().numpy().copy()
        _check_pairs(cfg, per_class, scene, classes, poses_g, gref.se3_iter.cpu().numpy(), "graph")
        graph = gref.graph
        assert graph is not None
        swapped = [0, 1, 0]
        load(gref, swapped)
        poses_s = gref.refine().cpu().numpy().copy()
        assert gref.graph is graph                                                                      # a replay, not a new capture
        assert float(np.abs(poses_s - poses_g).max()) > 1e-3
        _check_pairs(cfg, per_class, scene, swapped, poses_s, gref.se3_iter.cpu().numpy(), "graph replayed with other classes")
    finally:
        make_test_config()      # the configuration object is shared: back to one class, one head


# ------------------------------------------------------------------------------------------------ training
def test_train_iteration_and_absent_class_update(loop_scene):
    import copy

    from deepim.core.module import FROZEN, MutableModule
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    scene, bl = loop_scene, loop_scene["blobs"]
    cfg = _two_class_config(make_train_config())
    try:
        cfg.network.PRED_FLOW = cfg.network.PRED_MASK = False        # no decoder
        cfg.train_iter.SE3_PM_LOSS, cfg.train_iter.SE3_DIST_LOSS = True, True
        cfg.train_iter.LW_ROT, cfg.train_iter.LW_TRANS, cfg.train_iter.TRANS_LOSS_TYPE = 0.8, 1.3, "L2"
        cfg.TRAIN.wd = 0.05
        cfg = copy.deepcopy(cfg)
        B, K = 3, 2
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=True)
        params = sym.init_weights(cfg, {}, {}, seed=0)
        rng = np.random.RandomState(1)
        params["trans_weight"] = (rng.randn(6, 256) * 0.002).astype(np.float32)
        params["rot_weight"][[1, 2, 3, 5, 6, 7]] = (rng.randn(6, 256) * 0.01).astype(np.float32)
        params["rot_bias"], params["trans_bias"] = (0.01 * rng.randn(8)).astype(np.float32), (0.01 * rng.randn(6)).astype(np.float32)
        mod = MutableModule(cfg, params, B)
        assert mod.net.n_regressors == K and not mod.has_decoder
        batch = {k: torch.as_tensor(np.ascontiguousarray(v)).to(DEV) for k, v in bl.items()}
        assert batch["class_index"].tolist() == [1, 0, 1]
        mod.forward_backward(batch)
        g = mod.get_grads()
        cls = bl["class_index"]
        # the executor's own head state -> the four head gradients and dz7 in float64
        fc7, fc6a = host(mod.net.fc7), host(mod.net.fc6.view(B, 256))
        d_rot, d_rn, d_t, rot_raw = host(mod.d_rot), host(mod.d_rot_norm), host(mod.d_trans), host(mod.rot_raw)
        assert np.abs(d_rn).max() > 0 and np.abs(d_t).max() > 0
        for name, dz in (("rot", d_rot), ("trans", d_t)):
            ref = G.fc_wgrad(dz, fc7, cls, K)
            inside(g[name + "_weight"], ref["dW"], "train g[{}_weight]".format(name))
            inside(g[name + "_bias"], ref["db"], "train g[{}_bias]".format(name))
            assert np.abs(g[name + "_weight"][:dz.shape[1]]).max() > 0 and np.abs(g[name + "_weight"][dz.shape[1]:]).max() > 0
        ref = G.pose_head_bwd(fc6a, fc7, rot_raw, d_rn, d_t, params["fc7_weight"], params["rot_weight"], params["trans_weight"], cls, K)
        inside(host(mod.dz7), ref["dz7"], "train dz7")
        inside(d_rot, ref["d_rot"], "train d_rot")
        wrong = G.pose_head_bwd(fc6a, fc7, rot_raw, d_rn, d_t, params["fc7_weight"], params["rot_weight"], params["trans_weight"], cls, K,
                                mutant="class_of_sample_0_for_all")
        assert R.worst_ratio(host(mod.dz7), wrong["dz7"][0], wrong["dz7"][1]) > 10.0                     # the bars can tell the heads apart
        # a batch of class 1 alone, one SGD step: class 0's rows see a zero gradient -- weight decay (and momentum) only
        pick = torch.as_tensor([0, 2, 0], device=DEV)
        batch1 = {k: v[pick].contiguous() for k, v in batch.items()}
        assert batch1["class_index"].tolist() == [1, 1, 1]
        prev = mod.get_params()
        mod.forward_backward(batch1)
        g = mod.get_grads()
        lr, momentum, wd = 1e-2, float(cfg.TRAIN.momentum), 0.05
        mod.update(lr)
        new = mod.get_params()
        for k, rows in (("rot_weight", 4), ("rot_bias", 4), ("trans_weight", 3), ("trans_bias", 3)):
            assert k not in FROZEN
            assert not bits(g[k][:rows]).any(), k                                                       # exact zeros for the absent class
            r = R.sgd_momentum(prev[k][:rows], np.zeros_like(prev[k][:rows]), np.zeros_like(prev[k][:rows]), lr, momentum,
                               wd if k.endswith("_weight") else 0.0)
            inside(new[k][:rows], r["w"], "class 0 rows of {} after the step".format(k))
            if k.endswith("_weight"):
                assert np.abs(R.f64(new[k][:rows]) - R.f64(prev[k][:rows])).max() > 10.0 * r["w"][1].max()    # the decay is visible
            else:
                same_bits(new[k][:rows], prev[k][:rows], k)                                             # no decay on a bias
            assert np.abs(R.f64(new[k][rows:]) - R.f64(prev[k][rows:])).max() > 0, k                     # class 1 moved
            assert np.abs(g[k][rows:]).max() > 0, k
    finally:
        make_test_config()
