"""CPU: the float64 restatements of the training-head and optimizer kernels (tests/train_head_reference.py) are pinned by torch float64
autograd of the loss / layer written independently (the optimizers: by oracle.train.sgd_step / adam_step), a float32 evaluation of
each elementwise formula stays inside its bar, and on every input set the GPU tests use every named mutant is separated from the
reference by more than 10 bars on at least one output element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_head_reference as R
from oracle import train as otrain

SEP = 10.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(R.f64(a)))


def close(a, b, rtol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= rtol * max(1.0, np.abs(b).max()), float(np.abs(a - b).max())


def separation(ref, mut):
    """the largest |mutant - reference| / bar over all outputs"""
    return max(R.worst_ratio(mut[k][0], ref[k][0], ref[k][1]) for k in ref)


# ------------------------------------------------------------------------------------------------ references vs float64 autograd
@pytest.mark.parametrize("n", R.FLOW_SIZES[:2])
def test_flow_reference_vs_autograd(n):
    inp = R.flow_inputs(n)
    ref = R.flow_loss_grad(loss_prior=3.25, **inp, **R.FLOW_ARGS)
    a = T(inp["f_est"]).requires_grad_(True)
    nf, gs = R.sc(R.FLOW_ARGS["normalize_flow"]), R.sc(R.FLOW_ARGS["grad_scale"])
    loss = (T(inp["wgt"]) * (a - T(inp["f_lab"]) / nf) ** 2).sum()
    (g,) = torch.autograd.grad(gs * loss, a)
    close(ref["grad"][0], g.numpy())
    close(ref["loss_sum"][0], 3.25 + float(loss.detach()))


def test_logistic_reference_vs_autograd():
    inp = R.logistic_inputs(257)
    ref = R.logistic_grad(inp["logits"], inp["label"], R.LOGISTIC_GS)
    x = T(inp["logits"]).requires_grad_(True)
    (g,) = torch.autograd.grad(R.sc(R.LOGISTIC_GS) * F.binary_cross_entropy_with_logits(x, T(inp["label"]), reduction="sum"), x)
    close(ref["grad"][0], g.numpy())
    close(ref["prob"][0], torch.sigmoid(x).detach().numpy())
    p = ref["prob"][0]
    assert p[5] == 1.0 or 1.0 - p[5] < 1e-40      # +100: float64 keeps 4e-44, float32 must give exactly 1
    assert 0.0 < p[6] < 1e-40                     # -100


@pytest.mark.parametrize("kind,s", R.PM_CASES)
@pytest.mark.parametrize("n", R.PM_SIZES[:2])
def test_pm_reference_vs_autograd(n, kind, s):
    inp = R.pm_inputs(n, s)
    ref = R.pm_loss_grad(loss_type=kind, s=s, loss_prior=-0.5, **inp, **R.PM_ARGS)
    a = T(inp["p_est"]).requires_grad_(True)
    norm, gs = R.sc(R.PM_ARGS["norm_term"]), R.sc(R.PM_ARGS["grad_scale"])
    loss = (T(inp["wgt"]) * otrain._elem_loss((a - T(inp["p_obs"])) / norm, kind, s)).sum()
    (g,) = torch.autograd.grad(gs * loss, a)
    close(ref["grad"][0], g.numpy())
    close(ref["loss_sum"][0], -0.5 + float(loss.detach()))


@pytest.mark.parametrize("kind", R.LOSS_TYPES)
def test_se3_dist_reference_vs_autograd(kind):
    inp = R.se3_inputs(65)
    ref = R.se3_dist_loss_grad(trans_type=kind, **inp, **R.SE3_ARGS)
    q = T(inp["rot_norm"]).requires_grad_(True)
    fc7 = T(inp["fc7"])
    tz = (fc7 @ T(inp["trans_w"]).T + T(inp["trans_b"])).requires_grad_(True)      # zoom_trans_est recomputed from fc7
    lwr, lwt, s = (R.sc(R.SE3_ARGS[k]) for k in ("lw_rot", "lw_trans", "s"))
    rot_loss = (1.0 - (T(inp["rot_gt"]) * q).sum(dim=1) ** 2).sum()
    trans_loss = otrain._elem_loss(tz - T(inp["zt_gt"]), kind, s).sum()
    gq, gz = torch.autograd.grad(lwr * rot_loss + lwt * trans_loss, (q, tz))
    close(ref["d_rot_norm"][0], R.f64(inp["d_rot_prior"]) + gq.numpy())
    close(ref["d_zoom_trans"][0], R.f64(inp["d_zt_prior"]) + gz.numpy())
    close(ref["rot_loss_sum"][0], R.sc(inp["sums_prior"][0]) + float(rot_loss.detach()))
    close(ref["trans_loss_sum"][0], R.sc(inp["sums_prior"][1]) + float(trans_loss.detach()))
    assert (R.f64(inp["rot_gt"][0]) * R.f64(inp["rot_norm"][0])).sum() < -0.5      # the antipodal row


def test_quat_normalize_reference():
    inp = R.quat_inputs(65)
    y = R.quat_normalize(inp["rot"])["rot_norm"][0]
    q = T(inp["rot"])
    close(y, (q / torch.sqrt((q * q).sum(dim=1, keepdim=True) + 1e-10)).numpy())
    assert np.all(y[0] == 0.0) and np.all(np.isfinite(y))
    assert abs(np.linalg.norm(R.f64(inp["rot"][-1])) - 1e-6) < 1e-9 and 0.09 < np.linalg.norm(y[-1]) < 0.11   # 1e-6 / sqrt(1e-12 + 1e-10)
    assert np.abs(np.linalg.norm(y[1:-1], axis=1) - 1.0).max() < 1e-9


@pytest.mark.parametrize("B", R.POSE_BATCHES)
def test_pose_head_reference_vs_autograd(B):
    """one graph, one scalar: fc6a = LeakyReLU(z6), fc7 = LeakyReLU(fc6a W7^T + c7), rot = fc7 Wr^T + cr, tz = fc7 Wt^T, with the
    constants c7 / cr chosen so that the activations are the kernel's inputs; L = sum(d_rot_norm L2Normalization(rot)) + sum(d_trans tz)"""
    inp = R.pose_inputs(B)
    ref = R.pose_head_bwd(**inp)

    def inv_lrelu(a):
        return torch.where(a < 0, a / R.SLOPE, a)

    a6, a7 = T(inp["fc6a"]), T(inp["fc7"])
    w7, wr, wt = T(inp["fc7_w"]), T(inp["rot_w"]), T(inp["trans_w"])
    z6 = inv_lrelu(a6).requires_grad_(True)
    fc6a = F.leaky_relu(z6, R.SLOPE)
    z7 = fc6a @ w7.T + (inv_lrelu(a7) - a6 @ w7.T)
    z7.retain_grad()
    fc7 = F.leaky_relu(z7, R.SLOPE)
    rot = fc7 @ wr.T + (T(inp["rot_raw"]) - a7 @ wr.T)
    rot.retain_grad()
    tz = fc7 @ wt.T
    rot_norm = rot / torch.sqrt((rot * rot).sum(dim=1, keepdim=True) + 1e-10)
    ((T(inp["d_rot_norm"]) * rot_norm).sum() + (T(inp["d_trans"]) * tz).sum()).backward()
    close(fc6a.detach().numpy(), R.f64(inp["fc6a"]), 1e-15)
    close(ref["d_rot"][0], rot.grad.numpy(), 1e-9)
    close(ref["dz7"][0], z7.grad.numpy(), 1e-9)
    close(ref["dz6"][0], z6.grad.numpy(), 1e-9)


@pytest.mark.parametrize("B,Out,In", R.FC_SHAPES)
def test_fc_wgrad_reference_vs_autograd(B, Out, In):
    inp = R.fc_inputs(B, Out, In)
    ref = R.fc_wgrad(**inp)
    W = torch.zeros(Out, In, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Out, dtype=torch.float64, requires_grad=True)
    gW, gb = torch.autograd.grad((T(inp["dz"]) * F.linear(T(inp["x"]), W, b)).sum(), (W, b))
    close(ref["dW"][0], gW.numpy())
    close(ref["db"][0], gb.numpy())


@pytest.mark.parametrize("shape", R.DECONV_SHAPES[2:])
def test_deconv_reference_vs_direct_sums(shape):
    """the autograd restatement against the scatter form written out: y[n, 2 iy + ky - crop, 2 ix + kx - crop, co] += x[n, iy, ix, ci]
    w[ci, co, ky, kx] inside the OH x OW window"""
    N, H, W, Cin, Cout, OH, OW = shape
    inp = R.deconv_inputs(*shape)
    ref = R.deconv4x4s2_tiny_bwd(inp["x"], inp["dy"], inp["w"], OH, OW)
    x, dy, w = R.f64(inp["x"]), R.f64(inp["dy"]), R.f64(inp["w"])
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for iy in range(H):
        for ix in range(W):
            for ky in range(4):
                for kx in range(4):
                    oy, ox = 2 * iy + ky - 1, 2 * ix + kx - 1
                    if 0 <= oy < OH and 0 <= ox < OW:
                        dx[:, iy, ix, :] += dy[:, oy, ox, :] @ w[:, :, ky, kx].T
                        dw[:, :, ky, kx] += x[:, iy, ix, :].T @ dy[:, oy, ox, :]
    close(ref["dx"][0], dx)
    close(ref["dW"][0], dw)
    close(ref["db"][0], dy.sum(axis=(0, 1, 2)))


def test_sgd_reference_vs_oracle():
    rng = np.random.default_rng(5)
    params = {k: rng.normal(0, 0.3, 40).astype(np.float32) for k in ("a_weight", "a_bias", "upsampling_weight")}
    grads = {k: rng.normal(0, 1, 40).astype(np.float32) for k in params}
    moms = {k: rng.normal(0, 0.01, 40) for k in params}
    frozen = ("upsampling_weight",)
    zero = {k: 0.0 for k in params}
    new, nm, _, _ = R.sgd_params_step(params, grads, moms, zero, 1e-2, 0.9, 0.05, frozen)
    # the oracle multiplies by the Python doubles, the kernel by their float32 roundings: same formula, compared at the rounded scalars
    op, om = otrain.sgd_step({k: v.copy() for k, v in params.items()}, {k: v.astype(np.float64) for k, v in grads.items()},
                             {k: v.copy() for k, v in moms.items()}, R.sc(1e-2), R.sc(0.9), R.sc(0.05))
    for k in params:
        close(nm[k], om[k])
        close(new[k].astype(np.float32), op[k], 0.0)
    np.testing.assert_array_equal(new["upsampling_weight"], params["upsampling_weight"])
    # rescale_grad multiplies the gradient: 0.125 g (exact) with rescale 1 == g with rescale 0.125
    a = R.sgd_momentum(params["a_weight"], grads["a_weight"], moms["a_weight"], 1e-2, 0.9, 0.05, 0.125)
    b = R.sgd_momentum(params["a_weight"], 0.125 * grads["a_weight"], moms["a_weight"], 1e-2, 0.9, 0.05, 1.0)
    close(a["w"][0], b["w"][0])


def test_adam_reference_vs_oracle():
    """oracle.train.adam_step evaluates the same update in float32: it has to land inside the reference's bars"""
    inp = R.opt_inputs(255)
    w, mean, var = inp["w"], inp["mean"], inp["var"]
    for t, (lr, g) in enumerate(zip(R.ADAM_LRS, inp["grads"]), start=1):
        ref = R.adam(w, g, mean, var, R.adam_lr_t(lr, t), **R.ADAM_ARGS)
        p, m, v = otrain.adam_step({"a_weight": w.copy()}, {"a_weight": g}, {"a_weight": mean.copy()}, {"a_weight": var.copy()}, t, lr,
                                   wd=R.ADAM_ARGS["wd"], rescale_grad=R.ADAM_ARGS["rescale"])
        for name, got in (("w", p), ("mean", m), ("var", v)):
            assert R.worst_ratio(got["a_weight"], *ref[name]) <= 1.0, (name, t)
        w, mean, var = p["a_weight"], m["a_weight"], v["a_weight"]


# ------------------------------------------------------------------------------------------------ float32 evaluations stay inside the bars
def test_float32_evaluations_inside_bars():
    f = np.float32
    inp = R.flow_inputs(R.FLOW_SIZES[1])
    ref = R.flow_loss_grad(**inp, **R.FLOW_ARGS)
    inv = f(1) / f(R.FLOW_ARGS["normalize_flow"])
    d = inp["f_est"] - inp["f_lab"] * inv
    assert R.worst_ratio(f(R.FLOW_ARGS["grad_scale"]) * inp["wgt"] * f(2) * d, *ref["grad"]) <= 1.0
    assert R.worst_ratio(np.sum(inp["wgt"] * d * d, dtype=f), *ref["loss_sum"]) <= 1.0
    for kind, s in R.PM_CASES:
        inp = R.pm_inputs(R.PM_SIZES[1], s)
        ref = R.pm_loss_grad(loss_type=kind, s=s, **inp, **R.PM_ARGS)
        inv, gs, s2 = f(1) / f(R.PM_ARGS["norm_term"]), f(R.PM_ARGS["grad_scale"]), f(s) * f(s)
        r = (inp["p_est"] - inp["p_obs"]) * inv
        sg = np.sign(r).astype(f)
        df = {"L1": sg, "L2": f(2) * r, "smooth_L1": np.where(np.abs(r) < f(1) / s2, s2 * r, sg)}[kind]
        assert R.worst_ratio(gs * inp["wgt"] * df * inv, *ref["grad"]) <= 1.0, (kind, s)
    inp = R.quat_inputs(65)
    q = inp["rot"]
    y = q / np.sqrt((q * q).sum(axis=1, keepdims=True, dtype=f) + f(1e-10))
    assert R.worst_ratio(y, *R.quat_normalize(q)["rot_norm"]) <= 1.0
    inp = R.opt_inputs(255)
    ref = R.sgd_momentum(inp["w"], inp["grads"][0], inp["mom"], 1e-2, 0.9, 0.05, 0.125)
    m = f(0.9) * inp["mom"] - f(1e-2) * (f(0.125) * inp["grads"][0] + f(0.05) * inp["w"])
    assert R.worst_ratio(m, *ref["mom"]) <= 1.0 and R.worst_ratio(inp["w"] + m, *ref["w"]) <= 1.0


# ------------------------------------------------------------------------------------------------ the inputs are where they claim to be
def test_inputs_keep_their_distance_from_the_discontinuities():
    thr = np.array(R.SL1_THRESHOLDS)
    for n in R.PM_SIZES:
        for _, s in R.PM_CASES:
            inp = R.pm_inputs(n, s)
            inv = np.float32(1) / np.float32(R.PM_ARGS["norm_term"])
            r32 = ((inp["p_est"] - inp["p_obs"]) * inv).astype(np.float64)          # as the kernel forms it
            r64 = (R.f64(inp["p_est"]) - R.f64(inp["p_obs"])) * float(inv)
            t = float(np.float32(1) / (np.float32(s) * np.float32(s)))
            k = min(n, 9)
            assert r32[0] == 0.0 and r64[0] == 0.0 and inp["p_est"][0] != 0.0
            want = np.array([0.0, t, 1.5 * t, 0.5 * t, 2 * t, -t, -1.5 * t, -0.5 * t, -2 * t])[:k]
            want = 2.0 * R.f64(0.5 * want)        # 1.5 t needs 25 bits: rounded once when stored, exact from there on
            assert want[1] == t and (k < 5 or (want[3] == 0.5 * t and want[4] == 2 * t))
            assert np.array_equal(r32[:k], want) and np.array_equal(r64[:k], want) and np.all(inp["wgt"][:k] != 0)
            for r in (r32[k:], r64[k:]):
                assert np.all(np.abs(r) >= R.GAP) and np.all(np.abs(np.abs(r)[:, None] - thr[None]) >= R.GAP)
            if n > 9:
                assert (inp["wgt"] == 0).any() and (inp["wgt"] != 0).any()
    for B in R.SE3_BATCHES:
        inp = R.se3_inputs(B)
        for kind in R.LOSS_TYPES:
            r, r_bar = R.se3_dist_loss_grad(trans_type=kind, **inp, **R.SE3_ARGS)["trans_residual"]
            assert np.all(np.abs(r) - r_bar >= R.GAP) and np.all(np.abs(np.abs(r)[..., None] - thr) - r_bar[..., None] >= R.GAP)
    for B in R.POSE_BATCHES:
        inp = R.pose_inputs(B)
        for a in (inp["fc6a"], inp["fc7"]):
            assert (a == 0).any() and (a > 0).any() and (a < 0).any() and np.all((a == 0) | (np.abs(a) >= R.GAP))
        assert abs(np.linalg.norm(R.f64(inp["rot_raw"][0])) - 1e-4) < 1e-8
    for n in R.LOGISTIC_SIZES:
        x = R.logistic_inputs(n)["logits"]
        assert np.all((x == 0) | (np.abs(x) >= np.float32(1e-3)))
        assert set(np.unique(R.logistic_inputs(n)["label"])) <= {0.0, 1.0}
    for n in R.FLOW_SIZES:
        assert n % 4 == 0 and set(np.unique(R.flow_inputs(n)["wgt"])) == {0.0, 1.0}
    assert R.FLOW_SIZES[1] // 4 % 256 != 0 and R.FLOW_SIZES[2] // 4 > 256 * 1024          # ragged last group; beyond the 1024-workgroup cap
    assert all(n > 128 * 256 for n in R.PM_SIZES[1:])                                       # beyond the 128-workgroup cap


# ------------------------------------------------------------------------------------------------ every mutant is separated on every input set
@pytest.mark.parametrize("mutant", R.MUTANTS["flow_loss_grad"])
@pytest.mark.parametrize("n", R.FLOW_SIZES)
def test_flow_mutants_separated(n, mutant):
    inp = R.flow_inputs(n)
    assert separation(R.flow_loss_grad(**inp, **R.FLOW_ARGS), R.flow_loss_grad(mutant=mutant, **inp, **R.FLOW_ARGS)) > SEP


@pytest.mark.parametrize("n", R.PM_SIZES)
def test_pm_mutants_separated(n):
    """sign(0) = 1 shows under L1 (the zero residual sits in smooth-L1's quadratic branch); the 1 / s threshold differs from 1 / s^2
    for s = 2, 3, where the 1.5 t residual lies between the two"""
    for kind, s in R.PM_CASES:
        inp = R.pm_inputs(n, s)
        ref = R.pm_loss_grad(loss_type=kind, s=s, **inp, **R.PM_ARGS)
        if kind == "L1":
            assert separation(ref, R.pm_loss_grad(loss_type=kind, s=s, mutant="sign0_is_1", **inp, **R.PM_ARGS)) > SEP
        if kind == "smooth_L1" and s > 1:
            assert separation(ref, R.pm_loss_grad(loss_type=kind, s=s, mutant="sl1_threshold_1_over_s", **inp, **R.PM_ARGS)) > SEP, s


@pytest.mark.parametrize("kind", R.LOSS_TYPES)
@pytest.mark.parametrize("B", R.SE3_BATCHES)
def test_se3_dist_mutants_separated(B, kind):
    inp = R.se3_inputs(B)
    ref = R.se3_dist_loss_grad(trans_type=kind, **inp, **R.SE3_ARGS)
    mut = R.se3_dist_loss_grad(trans_type=kind, mutant="overwrite_not_add", **inp, **R.SE3_ARGS)
    for k in ("d_rot_norm", "d_zoom_trans"):
        assert R.worst_ratio(mut[k][0], *ref[k]) > SEP, k


@pytest.mark.parametrize("mutant", R.MUTANTS["pose_head_bwd"])
@pytest.mark.parametrize("B", R.POSE_BATCHES)
def test_pose_head_mutants_separated(B, mutant):
    inp = R.pose_inputs(B)
    ref, mut = R.pose_head_bwd(**inp), R.pose_head_bwd(mutant=mutant, **inp)
    if mutant == "lrelu0_is_1":   # both masks
        assert R.worst_ratio(mut["dz7"][0], *ref["dz7"]) > SEP
        only6 = (ref["dz7"][0] @ R.f64(inp["fc7_w"])) * R._lrelu_d(R.f64(inp["fc6a"]), mutant)    # the second mask alone
        assert R.worst_ratio(only6, *ref["dz6"]) > SEP
    else:
        assert R.worst_ratio(mut["d_rot"][0], *ref["d_rot"]) > SEP


@pytest.mark.parametrize("shape", R.DECONV_SHAPES)
def test_deconv_mutants_separated(shape):
    inp = R.deconv_inputs(*shape)
    args = (inp["x"], inp["dy"], inp["w"], shape[5], shape[6])
    assert separation(R.deconv4x4s2_tiny_bwd(*args), R.deconv4x4s2_tiny_bwd(*args, mutant="db_window_complement")) > SEP


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@pytest.mark.parametrize("wd,rescale", R.SGD_CASES)
@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_sgd_mutants_separated(n, wd, rescale):
    """at every one of the three chained steps (the state handed on is the reference's, rounded to float32 as the device holds it)"""
    inp = R.opt_inputs(n)
    w, mom = inp["w"], inp["mom"]
    for lr, g in zip(R.SGD_LRS, inp["grads"]):
        ref = R.sgd_momentum(w, g, mom, lr, R.SGD_MOMENTUM, wd, rescale)
        assert separation(ref, R.sgd_momentum(w, g, mom, lr, R.SGD_MOMENTUM, wd, rescale, mutant="momentum_sign")) > SEP
        if wd:
            assert separation(ref, R.sgd_momentum(w, g, mom, lr, R.SGD_MOMENTUM, wd, rescale, mutant="wd_inside_momentum")) > SEP
        w, mom = _f32(ref["w"][0]), _f32(ref["mom"][0])


def test_sgd_bias_decay_mutant_separated():
    rng = np.random.default_rng(11)
    params = {k: rng.normal(0, 0.1, 64).astype(np.float32) for k in ("a_weight", "a_bias")}
    grads = {k: rng.normal(0, 1e-2, 64).astype(np.float32) for k in params}
    zero = {k: np.zeros(64) for k in params}
    ref, _, _, bars = R.sgd_params_step(params, grads, zero, zero, 1e-3, 0.975, 0.05)
    mut, _, _, _ = R.sgd_params_step(params, grads, zero, zero, 1e-3, 0.975, 0.05, mutant="wd_on_bias")
    assert R.worst_ratio(mut["a_bias"], ref["a_bias"], bars["a_bias"]) > SEP
    np.testing.assert_array_equal(mut["a_weight"], ref["a_weight"])


@pytest.mark.parametrize("mutant", R.MUTANTS["adam"])
@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_adam_mutants_separated(n, mutant):
    inp = R.opt_inputs(n)
    w, mean, var = inp["w"], inp["mean"], inp["var"]
    for t, (lr, g) in enumerate(zip(R.ADAM_LRS, inp["grads"]), start=1):
        ref = R.adam(w, g, mean, var, R.adam_lr_t(lr, t), **R.ADAM_ARGS)
        assert separation(ref, R.adam(w, g, mean, var, R.adam_lr_t(lr, t), mutant=mutant, **R.ADAM_ARGS)) > SEP, t
        w, mean, var = _f32(ref["w"][0]), _f32(ref["mean"][0]), _f32(ref["var"][0])
