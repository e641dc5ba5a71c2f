"""The symmetry-aware point-matching loss on the device (csrc/train.hip: dim_pm_sym_loss_grad) through ops.pm_sym_loss_grad against the
float64 restatement of tests/sym_pm_reference.py, and through MutableModule with train_iter.SE3_PM_SYM.
tests/test_sym_pm_host.py shows on the CPU that the shared inputs separate every named mutant and keep the winner of every pair more
than 100 x the two bars away from the runner-up, so the float32 arg-min must be the reference's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import sym_pm_reference as S  # noqa: E402

DEV = "cuda:0"
PRIOR = 3.25          # the loss accumulator's value before the call
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def inside(got, ref, what):
    want, bar = ref
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    assert np.all(np.isfinite(got)), what
    ratio = S.worst_ratio(got, want, bar)
    print("{}: worst error {:.3f} bars".format(what, ratio))
    assert ratio <= 1.0, "{}: {:.3g} x its bar".format(what, ratio)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(ops, inp, loss_type="L1", s=1.0, optional=True, max_sym=None, status0=0, args=S.ARGS):
    """one call on fresh outputs -> dict of host arrays (grad, and with `optional` target, best_sym, loss, status)"""
    d = {k: dev(inp[k]) for k in ("p_est", "points_model", "weights", "tgt_pose", "sym")}
    off, cls = dev(inp["sym_off"], np.int32), dev(inp["class_index"], np.int32)
    B = inp["p_est"].shape[0]
    grad = torch.full_like(d["p_est"], SENTINEL)
    out = {}
    if optional:
        out = dict(target_out=torch.full_like(d["p_est"], SENTINEL), best_sym=torch.full((B,), 99, dtype=torch.int32, device=DEV),
                   loss_sum=torch.full((1,), PRIOR, device=DEV), status=torch.full((B,), status0, dtype=torch.int32, device=DEV))
    # the workspace: exactly dim_pm_sym_workspace_bytes (one word where a refused max_sym makes that 0) between guards, at the
    # documented minimum alignment (4 mod 8), full of NaN bits
    msym = inp["max_sym"] if max_sym is None else max_sym
    work = guard_arena.workspace(max(ops.lib().dim_pm_sym_workspace_bytes(B, inp["p_est"].shape[2], msym), 4), 4, DEV)
    ops.pm_sym_loss_grad(d["p_est"], d["points_model"], d["weights"], d["tgt_pose"], d["sym"], off, cls, grad, args["norm_term"],
                         args["grad_scale"], msym, loss_type=loss_type, smooth_l1_scalar=s, workspace=work.view(), **out)
    work.check("dim_pm_sym_loss_grad workspace, max_sym = {}".format(msym))
    res = {k: host(v) for k, v in out.items()}
    res["grad"] = host(grad)
    return res


def plain_grad(ops, p_est, p_obs, w, loss_type, s, args=S.ARGS, prior=PRIOR):
    """dim_pm_loss_grad on the same estimate and weights -> grad, loss_sum"""
    grad = torch.full(p_est.shape, SENTINEL, device=DEV)
    loss = torch.full((1,), prior, device=DEV)
    ops.pm_loss_grad(dev(p_est), dev(p_obs), dev(w), grad, args["norm_term"], args["grad_scale"], loss_type=loss_type, smooth_l1_scalar=s,
                     loss_sum=loss)
    return host(grad), host(loss)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("loss_type,s", S.CASES)
@pytest.mark.parametrize("n", S.SIZES)
def test_kernel_parity(ops, n, loss_type, s):
    """three pairs with 1, 2 and 33 symmetries; the estimate sits at the symmetry sym_pm_reference.TRUE_SYM names for this case"""
    inp = S.inputs(n, S.variant_of(n, loss_type))
    ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, loss_prior=PRIOR, **S.ARGS)
    got = run(ops, inp, loss_type, s)
    what = "pm_sym n={} {}".format(n, loss_type)
    print("{}: best_sym {} (reference {})".format(what, got["best_sym"], ref["best_sym"]))
    assert np.array_equal(got["best_sym"], ref["best_sym"]) and np.array_equal(got["best_sym"], inp["true_sym"])
    assert np.all(got["status"] == 0)
    inside(got["target_out"], ref["target"], what + " target")
    inside(got["loss_sum"][0], ref["loss_sum"], what + " loss sum")
    g, _ = plain_grad(ops, inp["p_est"], got["target_out"], inp["weights"], loss_type, s)
    assert np.array_equal(bits(got["grad"]), bits(g)), what + ": grad is not dim_pm_loss_grad's for target_out"
    inside(got["grad"], ref["grad"], what + " grad")
    again = run(ops, inp, loss_type, s)
    for k in ("grad", "target_out", "best_sym"):
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), what + ": a second call changed " + k
    assert np.array_equal(bits(run(ops, inp, loss_type, s, optional=False)["grad"]), bits(got["grad"])), what + ": grad depends on the optional outputs"


def _dyadic_inputs(n, rng):
    """inputs on which every sum of the loss is exact in float32, whatever its order: a 90-degree pose with translations in eighths,
    points in 64ths, residuals k / 16 of the normalised unit (|k| <= 16): the L1 and smooth-L1 terms are multiples of 2^-7, the L2
    terms of 2^-8, all <= 1, and the 9 n = 2313 of them that dim_pm_loss_grad adds into one number, plus the prior, stay below 2^12
    -- 20 bits"""
    pose = np.zeros((3, 3, 4), np.float32)
    pose[0, :, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    pose[1, :, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    pose[2, :, :3] = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    pose[:, :, 3] = rng.integers(-8, 9, (3, 3)) / 8.0
    table = (rng.integers(-64, 65, (3 * n, 3)) / 64.0).astype(np.float32)
    res = rng.integers(-16, 17, (3, 3, n)) / 16.0
    return pose, table, res


@pytest.mark.parametrize("loss_type,s", S.CASES)
def test_identity_only_table(ops, loss_type, s):
    """With the identity alone (listed, or as an empty range) the call is dim_point_clouds + dim_pm_loss_grad bit for bit: target_out
    against the point_cloud_observed of ops.point_clouds for the same table, indices and pose, grad against ops.pm_loss_grad on it.
    The loss: dim_pm_loss_grad adds its workgroups' sums with atomics, so its own float32 sum is not one fixed number on general
    inputs; on those the loss is held to the reference's bar, and bit for bit on inputs whose sums are exact in any order."""
    n = 257
    for exact in (False, True):
        rng = np.random.default_rng(13000 + int(exact))
        if exact:
            pose, table, res = _dyadic_inputs(n, rng)
        else:
            pose, table = S._poses(rng, 3), S._f32(rng.normal(0, 0.3, (3 * n, 3)))
            res = S._residuals(rng, 9 * n, hi=S.RES_HI).reshape(3, 3, n)
        idx = np.tile(np.arange(n, dtype=np.int32), (3, 1))
        idx[:, n - 25:] = -1                                     # zero-padded slots, weight 0
        model, weights, observed = (torch.full((3, 3, n), SENTINEL, device=DEV) for _ in range(3))
        ops.point_clouds(dev(table), dev([0, n, 2 * n], np.int32), dev(idx, np.int32), dev(pose), model, weights, observed)
        model, weights, observed = host(model), host(weights), host(observed)
        p_est = S._f32(observed.astype(np.float64) + S.ARGS["norm_term"] * res)
        inp = dict(p_est=p_est, points_model=model, weights=weights, tgt_pose=pose, sym=np.eye(4, dtype=np.float32)[None, :3],
                   sym_off=np.array([0, 0, 1], np.int32), class_index=np.array([0, 1, 0], np.int32), max_sym=1)   # class 0: an empty range
        got = run(ops, inp, loss_type, s)
        what = "identity only {} exact={}".format(loss_type, exact)
        assert list(got["best_sym"]) == [0, 0, 0] and np.all(got["status"] == 0)
        assert np.array_equal(bits(got["target_out"]), bits(observed)), what + ": target_out is not dim_point_clouds' point_cloud_observed"
        g, loss = plain_grad(ops, p_est, observed, weights, loss_type, s)
        assert np.array_equal(bits(got["grad"]), bits(g)), what
        print("{}: loss {!r}, dim_pm_loss_grad {!r}".format(what, float(got["loss_sum"][0]), float(loss[0])))
        if exact:
            assert np.array_equal(bits(got["loss_sum"]), bits(loss)), what
        else:
            ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, loss_prior=PRIOR, **S.ARGS)
            inside(got["loss_sum"][0], ref["loss_sum"], what + " loss sum")
            inside(loss[0], ref["loss_sum"], what + " loss sum of dim_pm_loss_grad")


def test_duplicate_entry_tie_goes_to_the_smaller_index(ops):
    inp = S.tie_inputs()
    got = run(ops, inp)
    assert list(got["best_sym"]) == [1, 1]
    ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_prior=PRIOR, **S.ARGS)
    inside(got["target_out"], ref["target"], "tie target")
    inside(got["loss_sum"][0], ref["loss_sum"], "tie loss sum")


def test_bad_class_and_max_sym(ops):
    """a class index outside the table, and a class larger than max_sym: zero rows, best_sym -1, DIM_STATUS_BAD_CLASS OR-ed into the
    status word, no loss contribution; the other pairs keep their bits"""
    inp = S.inputs(257, 1)
    good = run(ops, inp)
    for cls, max_sym, bad in (([3, 1, -1], None, [0, 2]), ([0, 1, 2], 2, [2]), ([0, 1, 2], 32, [2])):
        case = dict(inp, class_index=np.array(cls, np.int32))
        got = run(ops, case, max_sym=max_sym, status0=1)
        ref = S.pm_sym_loss_grad(**S.kernel_args(case), max_sym=max_sym or inp["max_sym"], loss_prior=PRIOR, **S.ARGS)
        assert np.array_equal(got["best_sym"], ref["best_sym"]), (cls, max_sym, got["best_sym"])
        for b in range(3):
            if b in bad:
                assert np.all(bits(got["grad"][b]) == 0) and np.all(bits(got["target_out"][b]) == 0)
                assert got["best_sym"][b] == -1 and got["status"][b] == (1 | ops.STATUS_BAD_CLASS)
            else:
                assert np.array_equal(bits(got["grad"][b]), bits(good["grad"][b])) and got["best_sym"][b] == good["best_sym"][b]
                assert np.array_equal(bits(got["target_out"][b]), bits(good["target_out"][b])) and got["status"][b] == 1
        inside(got["loss_sum"][0], ref["loss_sum"], "bad class {} max_sym {} loss sum".format(cls, max_sym))


def test_argument_errors(ops):
    """every rejected argument returns DIM_ERR_ARG with a message that names it, before anything is enqueued: grad keeps its sentinel"""
    from lib.hip.capi import current_stream, dptr

    inp = S.inputs(3, 0)
    f32, i32 = torch.float32, torch.int32
    t = {k: dev(inp[k]) for k in ("p_est", "points_model", "weights", "tgt_pose", "sym")}
    off, cls = dev(inp["sym_off"], np.int32), dev(inp["class_index"], np.int32)
    grad = torch.full((3, 3, 3), SENTINEL, device=DEV)
    ws = ops.pm_sym_workspace(3, 3, 33, DEV)
    base = dict(p_est=dptr(t["p_est"], f32), points_model=dptr(t["points_model"], f32), weights=dptr(t["weights"], f32),
                tgt_pose=dptr(t["tgt_pose"], f32), sym=dptr(t["sym"], f32), sym_off=dptr(off, i32), n_classes=3, class_index=dptr(cls, i32),
                B=3, n_points=3, max_sym=33, norm_term=0.5, grad_scale=1.0, loss_type=0, smooth_l1_scalar=1.0, workspace=dptr(ws),
                grad=dptr(grad, f32), target_out=None, best_sym=None, loss_sum=None, status=None)
    lib = ops.lib()

    def call(**change):
        a = dict(base, **change)
        return lib.dim_pm_sym_loss_grad(*[a[k] for k in base], current_stream())

    bad = [(dict(B=0), b"B ="), (dict(n_points=0), b"n_points"), (dict(max_sym=0), b"max_sym"), (dict(max_sym=4097), b"max_sym"),
           (dict(loss_type=3), b"loss_type"), (dict(loss_type=-1), b"loss_type"), (dict(loss_type=2, smooth_l1_scalar=0.0), b"smooth_l1_scalar"),
           (dict(norm_term=0.0), b"norm_term"), (dict(norm_term=-1.0), b"norm_term")]
    bad += [({k: None}, b"null pointer") for k in ("p_est", "points_model", "weights", "tgt_pose", "sym", "sym_off", "class_index", "workspace",
                                                  "grad")]
    for change, word in bad:
        assert call(**change) == -1, change
        msg = lib.dim_last_error()
        assert msg.startswith(b"pm_sym_loss_grad") and word in msg, (change, msg)
    assert np.all(host(grad) == SENTINEL)
    assert call() == 0 and np.all(host(grad) != SENTINEL)
    assert lib.dim_pm_sym_workspace_bytes(16, 3000, 315) == 16 * 6 * 315 * 4 and lib.dim_pm_sym_workspace_bytes(0, 3000, 315) == 0
    with pytest.raises(ValueError):
        run(ops, inp, loss_type="huber")


# ------------------------------------------------------------------------------------------------ MutableModule
FLIP_Z = np.array([[-1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, 1.0, 0]])    # 180 degrees about the model's z axis


@pytest.fixture(scope="module")
def train_setup(hip_lib):
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from scene import make_train_config, make_train_scene

    cfg = make_train_config()
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=True)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    rng = np.random.RandomState(1)                       # the head weights of tests/test_gpu_train.py
    params["trans_weight"] = (rng.randn(3, 256) * 0.002).astype(np.float32)
    params["rot_weight"][1:] = (rng.randn(3, 256) * 0.01).astype(np.float32)
    params["mask_conv3_weight"] = (rng.randn(1, 770, 3, 3) * 0.02).astype(np.float32)
    return params, make_train_scene(B=2, seed=99, subdiv=3)


def _observed(pose32, model):
    """point_cloud_observed as the loader makes it from the float32 pose (dim_point_clouds' expression)"""
    T, P = pose32.astype(np.float64), model.astype(np.float64)
    return (((T[:, :, 0:1] * P[:, 0:1] + T[:, :, 1:2] * P[:, 1:2]) + T[:, :, 2:3] * P[:, 2:3]) + T[:, :, 3:4]).astype(np.float32)


def test_module_loss_does_not_depend_on_the_label_among_symmetric_poses(train_setup):
    """One batch, and the same batch with pair 0's ground truth relabelled to tgt_pose . S (S: 180 degrees about the model's z axis,
    through the origin, so that the relabelled float32 pose is the old one with signs flipped and both runs see the same two candidate
    poses bit for bit).  SE3_PM_SYM on: the point-matching loss and the pose-head gradients agree within 1e-5 of each gradient's
    largest entry (the f32 bar of tests/test_gpu_train.py) and pm_best_sym moves by exactly the relabelling.  SE3_PM_SYM off: the two
    batches differ by at least 100 x that bar -- the negative control.  SE3_PM_SYM on without symmetries: the gradients of the
    SE3_PM_SYM-off run, bit for bit."""
    from deepim.core.module import MutableModule
    from scene import make_train_config

    params, scene = train_setup
    cfg = make_train_config()
    names = ("rot_weight", "trans_weight", "fc7_weight")
    bl = dict(scene["blobs"])
    bl["class_index"] = np.asarray(bl["class_index"], np.int32)
    bl["point_cloud_observed"] = _observed(bl["tgt_pose"], bl["point_cloud_model"])
    bl2 = dict(bl)
    pose2 = bl["tgt_pose"].copy()
    pose2[0, :, :3] = bl["tgt_pose"][0, :, :3] * np.array([-1.0, -1.0, 1.0], np.float32)        # R_g . diag(-1, -1, 1); t_g stays
    assert np.array_equal(pose2[0], (bl["tgt_pose"][0].astype(np.float64) @ np.vstack([FLIP_Z, [0, 0, 0, 1]])).astype(np.float32))
    bl2["tgt_pose"], bl2["point_cloud_observed"] = pose2, _observed(pose2, bl["point_cloud_model"])
    batches = [{k: torch.as_tensor(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()} for b in (bl, bl2)]

    def runs(pm_sym, symmetries, which=(0, 1)):
        cfg.train_iter.SE3_PM_SYM = pm_sym
        try:
            mod = MutableModule(cfg, params, 2, symmetries=symmetries)
        finally:
            cfg.train_iter.SE3_PM_SYM = False
        res = []
        for i in which:
            out = mod.forward_backward(batches[i])
            g = mod.get_grads()
            res.append(dict(loss=float(mod.loss_sums[1].cpu()), best=out["pm_best_sym"].cpu().numpy().copy() if pm_sym else None,
                            all=g, **{k: g[k] for k in names}))
        return res

    def worst(a, b):
        """the largest difference of a gradient (and of the loss) in units of its largest magnitude"""
        r = {k: np.abs(a[k] - b[k]).max() / np.abs(a[k]).max() for k in names}
        r["loss"] = abs(a["loss"] - b["loss"]) / abs(a["loss"])
        return r

    on = runs(True, {"ape": {"symmetries_discrete": [np.vstack([FLIP_Z, [0, 0, 0, 1]]).reshape(-1).tolist()]}})
    off = runs(False, None)
    BAR = 1e-5
    r_on, r_off = worst(on[0], on[1]), worst(off[0], off[1])
    print("SE3_PM_SYM on : relabelled vs original {}  best_sym {} -> {}".format(r_on, on[0]["best"], on[1]["best"]))
    print("SE3_PM_SYM off: relabelled vs original {}".format(r_off))
    assert all(v <= BAR for v in r_on.values()), r_on
    assert list(on[1]["best"]) == [on[0]["best"][0] ^ 1, on[0]["best"][1]] and set(on[0]["best"]) <= {0, 1}
    assert all(v >= 100 * BAR for v in r_off.values()), r_off
    plain = runs(True, None, which=(0,))[0]
    assert list(plain["best"]) == [0, 0]
    for k, g in off[0]["all"].items():
        assert np.array_equal(bits(plain["all"][k]), bits(g)), k
    cfg.train_iter.SE3_PM_SYM, cfg.train_iter.SE3_PM_LOSS = True, False
    cfg.train_iter.SE3_DIST_LOSS = True
    try:
        with pytest.raises(Exception, match="SE3_PM_SYM"):
            MutableModule(cfg, params, 2)
    finally:
        make_train_config()
