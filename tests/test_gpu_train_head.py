"""The kernels that turn network outputs into gradients and parameters (csrc/train.hip: loss gradients, pose-head backward, small FC /
tiny deconv backward, SGD, Adam), each through its ops wrapper against the float64 restatement of tests/train_head_reference.py at
the shapes where a launch takes another path, with the worst-case float32 rounding bar the reference derives per output element.
tests/test_train_head_host.py shows on the CPU that these inputs separate every named mutant by more than 10 bars."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import train_head_reference as R  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def inside(got, ref, what):
    """got within the reference's bar on every element; the message carries the worst error in bars"""
    want, bar = ref
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    assert np.all(np.isfinite(got)), what
    ratio = R.worst_ratio(got, want, bar)
    print("{}: worst error {:.3f} bars".format(what, ratio))
    assert ratio <= 1.0, "{}: {:.3g} x its bar".format(what, ratio)


# ------------------------------------------------------------------------------------------------ flow / mask losses
@pytest.mark.parametrize("prior", [None, 3.25])
@pytest.mark.parametrize("n", R.FLOW_SIZES)
def test_flow_loss_grad(ops, n, prior):
    inp = R.flow_inputs(n)
    ref = R.flow_loss_grad(loss_prior=prior or 0.0, **inp, **R.FLOW_ARGS)
    grad = torch.full((n,), 7.0, device=DEV)
    loss = None if prior is None else torch.full((1,), prior, device=DEV)
    ops.flow_loss_grad(dev(inp["f_est"]), dev(inp["f_lab"]), dev(inp["wgt"]), grad, R.FLOW_ARGS["normalize_flow"], R.FLOW_ARGS["grad_scale"],
                       loss_sum=loss)
    inside(host(grad), ref["grad"], "flow grad n={}".format(n))
    if loss is not None:
        inside(host(loss)[0], ref["loss_sum"], "flow loss sum n={}".format(n))      # accumulates onto the prior value


def test_flow_loss_grad_rejects_ragged_count(ops):
    from lib.hip.capi import DeepIMHipError

    a = torch.zeros(6, device=DEV)
    grad = torch.full((6,), 7.0, device=DEV)
    with pytest.raises(DeepIMHipError, match="multiple of 4"):
        ops.flow_loss_grad(a, a, a, grad, 20.0, 1.0)
    assert np.all(host(grad) == 7.0)     # nothing was launched


@pytest.mark.parametrize("with_prob", [False, True])
@pytest.mark.parametrize("n", R.LOGISTIC_SIZES)
def test_logistic_grad(ops, n, with_prob):
    inp = R.logistic_inputs(n)
    ref = R.logistic_grad(inp["logits"], inp["label"], R.LOGISTIC_GS)
    grad = torch.full((n,), 7.0, device=DEV)
    prob = torch.full((n,), 7.0, device=DEV) if with_prob else None
    ops.logistic_grad(dev(inp["logits"]), dev(inp["label"]), grad, R.LOGISTIC_GS, prob=prob)
    g = host(grad)
    inside(g, ref["grad"], "logistic grad n={}".format(n))
    if with_prob:
        p = host(prob)
        inside(p, ref["prob"], "logistic prob n={}".format(n))
        x = inp["logits"]
        assert np.all(p[x == 100.0] == 1.0) and np.all(p[x == -100.0] == 0.0)       # the expf overflow side: exactly 0 / 1, no NaN
        assert np.all(p[x == 0.0] == 0.5)


# ------------------------------------------------------------------------------------------------ point-matching loss
@pytest.mark.parametrize("kind,s", R.PM_CASES)
@pytest.mark.parametrize("n", R.PM_SIZES)
def test_pm_loss_grad(ops, n, kind, s):
    inp = R.pm_inputs(n, s)
    prior = -0.5
    ref = R.pm_loss_grad(loss_type=kind, s=s, loss_prior=prior, **inp, **R.PM_ARGS)
    a, b, w = dev(inp["p_est"]), dev(inp["p_obs"]), dev(inp["wgt"])
    grad = torch.full((n,), 7.0, device=DEV)
    loss = torch.full((1,), prior, device=DEV)
    ops.pm_loss_grad(a, b, w, grad, R.PM_ARGS["norm_term"], R.PM_ARGS["grad_scale"], loss_type=kind, smooth_l1_scalar=s, loss_sum=loss)
    g = host(grad)
    inside(g, ref["grad"], "pm grad {} s={} n={}".format(kind, s, n))
    inside(host(loss)[0], ref["loss_sum"], "pm loss sum {} s={} n={}".format(kind, s, n))
    if kind != "L2":
        assert g[0] == 0.0           # the bitwise-zero residual: sign(0) = 0, and 0 in the quadratic branch
    if kind == "L1":
        g1 = torch.full((n,), 7.0, device=DEV)
        l1 = torch.full((1,), prior, device=DEV)
        ops.pm_l1_grad(a, b, w, g1, R.PM_ARGS["norm_term"], R.PM_ARGS["grad_scale"], loss_sum=l1)
        assert np.array_equal(host(g1), g)       # the L1 entry point is the general kernel with type 0
        inside(host(l1)[0], ref["loss_sum"], "pm_l1 loss sum n={}".format(n))
    no_sum = torch.full((n,), 7.0, device=DEV)
    ops.pm_loss_grad(a, b, w, no_sum, R.PM_ARGS["norm_term"], R.PM_ARGS["grad_scale"], loss_type=kind, smooth_l1_scalar=s)
    assert np.array_equal(host(no_sum), g)


def test_pm_loss_grad_rejects_bad_type_and_scalar(ops):
    from lib.hip.capi import DeepIMHipError, current_stream, dptr

    a = torch.zeros(8, device=DEV)
    grad = torch.full((8,), 7.0, device=DEV)
    f32 = torch.float32
    rc = ops.lib().dim_pm_loss_grad(dptr(a, f32), dptr(a, f32), dptr(a, f32), dptr(grad, f32), 8, 1.0, 1.0, 3, 1.0, None, current_stream())
    assert rc == -1 and b"loss_type" in ops.lib().dim_last_error()
    with pytest.raises(DeepIMHipError, match="scalar > 0"):
        ops.pm_loss_grad(a, a, a, grad, 1.0, 1.0, loss_type="smooth_L1", smooth_l1_scalar=0.0)
    assert np.all(host(grad) == 7.0)


# ------------------------------------------------------------------------------------------------ SE3_DIST_LOSS, quaternion normalise
@pytest.mark.parametrize("kind", R.LOSS_TYPES)
@pytest.mark.parametrize("B", R.SE3_BATCHES)
def test_se3_dist_loss_grad(ops, B, kind):
    inp = R.se3_inputs(B)
    ref = R.se3_dist_loss_grad(trans_type=kind, **inp, **R.SE3_ARGS)
    d_rot, d_zt, sums = dev(inp["d_rot_prior"]), dev(inp["d_zt_prior"]), dev(np.array(inp["sums_prior"]))
    p = {"trans_weight": dev(inp["trans_w"]), "trans_bias": dev(inp["trans_b"])}
    ops.se3_dist_loss_grad(dev(inp["rot_norm"]), dev(inp["rot_gt"]), dev(inp["fc7"]), p, dev(inp["zt_gt"]), d_rot, d_zt, R.SE3_ARGS["lw_rot"],
                           R.SE3_ARGS["lw_trans"], trans_loss_type=kind, smooth_l1_scalar=R.SE3_ARGS["s"], loss_sums2=sums)
    # the increments over the non-zero prior contents (float32 - float32 in float64 is exact)
    for name, got, prior in (("d_rot_norm", d_rot, inp["d_rot_prior"]), ("d_zoom_trans", d_zt, inp["d_zt_prior"])):
        want, bar = ref[name]
        inside(R.f64(host(got)) - R.f64(prior), (want - R.f64(prior), bar), "se3 {} increment {} B={}".format(name, kind, B))
    s = host(sums)
    inside(s[0], ref["rot_loss_sum"], "se3 rot loss sum B={}".format(B))
    inside(s[1], ref["trans_loss_sum"], "se3 trans loss sum {} B={}".format(kind, B))


@pytest.mark.parametrize("B", R.QUAT_BATCHES)
def test_quat_normalize(ops, B):
    inp = R.quat_inputs(B)
    y = host(ops.quat_normalize(dev(inp["rot"]), out=torch.full((B, 4), 7.0, device=DEV)))
    inside(y, R.quat_normalize(inp["rot"])["rot_norm"], "quat_normalize B={}".format(B))
    assert np.all(y[0] == 0.0)       # the all-zero row: 0 / sqrt(1e-10), not NaN


# ------------------------------------------------------------------------------------------------ pose head, small FC, tiny deconv
@pytest.mark.parametrize("B", R.POSE_BATCHES)
def test_pose_head_bwd(ops, B):
    inp = R.pose_inputs(B)
    ref = R.pose_head_bwd(**inp)
    p = {"fc7_weight": dev(inp["fc7_w"]), "rot_weight": dev(inp["rot_w"]), "trans_weight": dev(inp["trans_w"])}
    d_rot, dz7, dz6 = (torch.full(s, 7.0, device=DEV) for s in ((B, 4), (B, 256), (B, 256)))
    ops.pose_head_bwd(dev(inp["fc6a"]), dev(inp["fc7"]), dev(inp["rot_raw"]), dev(inp["d_rot_norm"]), dev(inp["d_trans"]), p, d_rot, dz7, dz6)
    for name, got in (("d_rot", d_rot), ("dz7", dz7), ("dz6", dz6)):
        inside(host(got), ref[name], "pose_head_bwd {} B={}".format(name, B))


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("B,Out,In", R.FC_SHAPES)
def test_fc_wgrad(ops, B, Out, In, with_db):
    inp = R.fc_inputs(B, Out, In)
    ref = R.fc_wgrad(**inp)
    dW = torch.full((Out, In), 7.0, device=DEV)
    db = torch.full((Out,), 7.0, device=DEV) if with_db else None
    ops.fc_wgrad(dev(inp["dz"]), dev(inp["x"]), dW, db)
    inside(host(dW), ref["dW"], "fc_wgrad dW {}".format((B, Out, In)))
    if with_db:
        inside(host(db), ref["db"], "fc_wgrad db {}".format((B, Out, In)))


@pytest.mark.parametrize("with_dx", [True, False])
@pytest.mark.parametrize("shape", R.DECONV_SHAPES)
def test_deconv4x4s2_tiny_bwd(ops, shape, with_dx):
    """x with x_cstride = Cin + 3, dy = channels [66, 66 + Cout) of a 70-channel buffer; the other channels hold a sentinel the result
    must not depend on (run twice with different sentinels: bit-identical)"""
    N, H, W, Cin, Cout, OH, OW = shape
    inp = R.deconv_inputs(*shape)
    ref = R.deconv4x4s2_tiny_bwd(inp["x"], inp["dy"], inp["w"], OH, OW)
    results = []
    for sentinel in (R.DECONV_SENTINEL, -3.0):
        xw, dyw = inp["x_wide"].copy(), inp["dy_wide"].copy()
        xw[..., Cin:] = sentinel
        dyw[..., :R.DECONV_DY_COFF] = sentinel
        dyw[..., R.DECONV_DY_COFF + Cout:] = sentinel
        dx = torch.full((N, H, W, Cin), 7.0, device=DEV) if with_dx else None
        dw, db = torch.full((Cin, Cout, 4, 4), 7.0, device=DEV), torch.full((Cout,), 7.0, device=DEV)
        ops.deconv4x4s2_tiny_bwd(dev(xw), dev(dyw), R.DECONV_DY_COFF, dev(inp["w"]), dx, dw, db, crop=1)
        results.append((host(dx) if with_dx else None, host(dw), host(db)))
    (dx0, dw0, db0), (dx1, dw1, db1) = results
    assert np.array_equal(dw0, dw1) and np.array_equal(db0, db1) and (not with_dx or np.array_equal(dx0, dx1))
    inside(dw0, ref["dW"], "tiny deconv dW {}".format(shape))
    inside(db0, ref["db"], "tiny deconv db {}".format(shape))
    if with_dx:
        inside(dx0, ref["dx"], "tiny deconv dx {}".format(shape))


# ------------------------------------------------------------------------------------------------ optimizers
PAD = 32    # floats around the updated slice (tensors of the flat vectors start on 128-byte boundaries)


def _embedded(a, fill):
    """a device vector with `a` at [PAD, PAD + n) and `fill` around it -> (whole vector, the slice view)"""
    big = torch.full((a.size + 2 * PAD,), fill, device=DEV)
    big[PAD:PAD + a.size] = dev(a)
    return big, big[PAD:PAD + a.size]


def _neighbours_untouched(big, n, fill):
    h = host(big)
    assert np.all(h[:PAD] == np.float32(fill)) and np.all(h[PAD + n:] == np.float32(fill))


@pytest.mark.parametrize("wd,rescale", R.SGD_CASES)
@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_sgd_momentum_three_steps(ops, n, wd, rescale):
    """three consecutive steps, a different lr each, non-zero momentum from the start; after every step the reference is fed the
    device's own previous weights and momentum, so each step is checked at one step's bar"""
    inp = R.opt_inputs(n)
    big_w, w = _embedded(inp["w"], 5.0)
    big_m, m = _embedded(inp["mom"], -6.0)
    w_prev, m_prev = inp["w"], inp["mom"]
    for step, (lr, g) in enumerate(zip(R.SGD_LRS, inp["grads"])):
        ref = R.sgd_momentum(w_prev, g, m_prev, lr, R.SGD_MOMENTUM, wd, rescale)
        ops.sgd_momentum(w, dev(g), m, lr, R.SGD_MOMENTUM, wd, rescale_grad=rescale)
        w_prev, m_prev = host(w).copy(), host(m).copy()
        inside(m_prev, ref["mom"], "sgd mom n={} wd={} rescale={} step {}".format(n, wd, rescale, step))
        inside(w_prev, ref["w"], "sgd w n={} wd={} rescale={} step {}".format(n, wd, rescale, step))
    _neighbours_untouched(big_w, n, 5.0)
    _neighbours_untouched(big_m, n, -6.0)


@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_adam_three_steps(ops, n):
    """wd = 0.01 (the term MutableModule.update never switches on), rescale_grad = 0.5, lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)"""
    inp = R.opt_inputs(n)
    big_w, w = _embedded(inp["w"], 5.0)
    big_m, mean = _embedded(inp["mean"], -6.0)
    big_v, var = _embedded(inp["var"], 9.0)
    prev = (inp["w"], inp["mean"], inp["var"])
    for t, (lr, g) in enumerate(zip(R.ADAM_LRS, inp["grads"]), start=1):
        lr_t = R.adam_lr_t(lr, t)
        ref = R.adam(prev[0], g, prev[1], prev[2], lr_t, **R.ADAM_ARGS)
        ops.adam(w, dev(g), mean, var, lr_t, wd=R.ADAM_ARGS["wd"], rescale_grad=R.ADAM_ARGS["rescale"])
        prev = (host(w).copy(), host(mean).copy(), host(var).copy())
        for name, got in zip(("w", "mean", "var"), prev):
            inside(got, ref[name], "adam {} n={} t={}".format(name, n, t))
    for big, fill in ((big_w, 5.0), (big_m, -6.0), (big_v, 9.0)):
        _neighbours_untouched(big, n, fill)
