"""float64 restatements of the training-head and optimizer kernels (csrc/train.hip), their rounding bars, named mutants and the seeded
inputs the CPU and GPU tests share.

Every reference takes the float32 arrays a kernel reads (scalars as the C ABI passes them: rounded to float32 first), promotes them to
float64 and evaluates the formulas of oracle/train.py / the MXNet operators cited in train.hip.  It returns {output name: (value, bar)}:
`bar` is the absolute float32 rounding bound of that output element, worked out from the actual inputs, U = 2^-24:

  elementwise   k U S       S = the sum of the magnitudes of the terms added or subtracted to form the element (a single product: its
                            magnitude), k = twice the number of float32 roundings on the longest path (stated next to every formula)
  sums          2 (n + p) U sum|term_i|     n terms added in any order (atomics included; a pre-filled accumulator is one more term),
                            p roundings inside one term; |term_i| is the product of the magnitudes of its factors, a factor that is itself
                            a difference counting as |a| + |b|.  This is twice the textbook gamma_(n - 1 + p) bound; for p = 0 it is
                            2 n U sum|term_i|
  chained       the bar of a first stage is carried through the second stage's sum|w| (dz7 -> dz6, tz -> d_zoom_trans, m / v -> w)

Discontinuities are handled by the inputs, not by the bars: every residual / activation is bitwise at its special value or >= 1e-3 away.

`mutant=NAME` evaluates a plausible wrong kernel instead (MUTANTS lists them per kernel); tests/test_train_head_host.py shows that the
shared inputs separate each one from the reference by more than 10 bars.
"""
import numpy as np

U = 2.0 ** -24
SLOPE = 0.1            # LeakyReLU slope of the pose head (act_type 'leaky', slope 0.1); derivative at 0 = SLOPE as in MXNet (x > 0 ? 1 : slope)
L2N_EPS = 1e-10        # L2Normalization(mode='instance') eps
LOSS_TYPES = ("L1", "L2", "smooth_L1")

MUTANTS = {
    "flow_loss_grad": ("no_factor_2", "inv_nf_on_estimate"),
    "pm_loss_grad": ("sl1_threshold_1_over_s", "sign0_is_1"),
    "se3_dist_loss_grad": ("overwrite_not_add",),
    "pose_head_bwd": ("lrelu0_is_1", "norm_bwd_no_projection"),
    "deconv4x4s2_tiny_bwd": ("db_window_complement",),
    "sgd_momentum": ("wd_inside_momentum", "momentum_sign"),
    "sgd_params_step": ("wd_on_bias",),
    "adam": ("no_wd", "sqrt_v_plus_eps"),
}


def f64(x):
    """a float32 device array as float64"""
    return np.asarray(x, np.float32).astype(np.float64)


def sc(x):
    """a scalar as the C ABI passes it (float), as float64"""
    return float(np.float32(x))


def _check_mutant(kernel, mutant):
    assert mutant is None or mutant in MUTANTS[kernel], (kernel, mutant)


def worst_ratio(got, want, bar):
    """max over elements of |got - want| / bar (0 / 0 = 0): <= 1 passes"""
    err = np.abs(np.asarray(got, np.float64) - want)
    bar = np.broadcast_to(np.asarray(bar, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ element losses (MakeLoss inputs)
def elem_loss(x, kind, s, mutant=None):
    """value and derivative of |x|, x^2, mx.sym.smooth_l1(x, scalar = s): 0.5 (s x)^2 where |x| < 1 / s^2, |x| - 0.5 / s^2 elsewhere;
    sign(0) = 0"""
    ax = np.abs(x)
    sg = np.sign(x)
    if mutant == "sign0_is_1":
        sg = np.where(x == 0.0, 1.0, sg)
    if kind == "L1":
        return ax, sg
    if kind == "L2":
        return x * x, 2.0 * x
    assert kind == "smooth_L1"
    s2 = s * s
    thr = 1.0 / s if mutant == "sl1_threshold_1_over_s" else 1.0 / s2
    quad = ax < thr
    return np.where(quad, 0.5 * s2 * x * x, ax - 0.5 / s2), np.where(quad, s2 * x, sg)


def _elem_mag(mag, kind, s, x):
    """(|value| bound, |derivative| bound) with the residual's magnitude bound `mag` >= |x| in place of |x|; the branch is x's own"""
    if kind == "L1":
        return mag, np.ones_like(mag)
    if kind == "L2":
        return mag * mag, 2.0 * mag
    s2 = s * s
    quad = np.abs(x) < 1.0 / s2
    return np.where(quad, 0.5 * s2 * mag * mag, mag + 0.5 / s2), np.where(quad, s2 * mag, 1.0)


# ------------------------------------------------------------------------------------------------ flow / mask losses
def flow_loss_grad(f_est, f_lab, wgt, normalize_flow, grad_scale, loss_prior=0.0, mutant=None):
    """MakeLoss(w (f_est - f / NORMALIZE_FLOW)^2, grad_scale): grad = gs w 2 (a - b inv_nf); loss_sum += sum w d^2.
    grad: roundings inv_nf, b inv_nf, a - ., gs w, . d (the factor 2 is exact) = 5 -> k = 10, S = |gs w 2| (|a| + |b inv_nf|).
    loss: n + 1 terms (the accumulator's prior value is one), p = 8 (three in each d, two products)."""
    _check_mutant("flow_loss_grad", mutant)
    a, b, w = f64(f_est), f64(f_lab), f64(wgt)
    inv, gs = 1.0 / sc(normalize_flow), sc(grad_scale)
    d = a * inv - b if mutant == "inv_nf_on_estimate" else a - b * inv
    mag = np.abs(a) + np.abs(b * inv)
    two = 1.0 if mutant == "no_factor_2" else 2.0
    grad = gs * w * two * d
    prior = sc(loss_prior)
    loss = prior + float((w * d * d).sum())
    loss_bar = 2.0 * (a.size + 1 + 8) * U * (abs(prior) + float((np.abs(w) * mag * mag).sum()))
    return {"grad": (grad, 10.0 * U * np.abs(gs * w * 2.0) * mag), "loss_sum": (loss, loss_bar)}


def logistic_grad(logits, label, gs_over_n):
    """LogisticRegressionOutput backward: grad = grad_scale / num_output (sigmoid(x) - y).  The probability goes through expf and a
    division: bar 8 U absolute; the gradient's is that times |gs_over_n| plus one ulp of the product."""
    x, y = f64(logits), f64(label)
    g = sc(gs_over_n)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
    grad = g * (p - y)
    ulp = np.spacing(np.abs(grad).astype(np.float32)).astype(np.float64)
    return {"prob": (p, np.full(p.shape, 8.0 * U)), "grad": (grad, 8.0 * U * abs(g) + ulp)}


# ------------------------------------------------------------------------------------------------ point-matching loss
def pm_loss_grad(p_est, p_obs, wgt, norm_term, grad_scale, loss_type="L1", s=1.0, loss_prior=0.0, mutant=None):
    """MakeLoss(w f((P_est - P_obs) / NORMALIZE_3D_POINT), grad_scale): grad = gs w f'(r) / norm, r = (a - b) / norm.
    roundings: 1 / norm, gs w, . f', . inv = 3 besides f' itself; f' = sign: exact (k = 6, S = |gs w inv|); f' = 2 r: a - b, . inv and the
    rounded inv = 3 more (k = 12, S = |gs w inv| 2 (|a| + |b|) inv); f' = s^2 r: s s and s2 . r on top (k = 16).
    loss: n + 1 terms, p = 8."""
    _check_mutant("pm_loss_grad", mutant)
    a, b, w = f64(p_est), f64(p_obs), f64(wgt)
    inv, gs, s = 1.0 / sc(norm_term), sc(grad_scale), sc(s)
    r = (a - b) * inv
    v, df = elem_loss(r, loss_type, s, mutant)
    mag = (np.abs(a) + np.abs(b)) * inv
    vmag, dmag = _elem_mag(mag, loss_type, s, r)
    k = {"L1": 6.0, "L2": 12.0, "smooth_L1": 16.0}[loss_type]
    grad = gs * w * df * inv
    prior = sc(loss_prior)
    loss = prior + float((w * v).sum())
    loss_bar = 2.0 * (a.size + 1 + 8) * U * (abs(prior) + float((np.abs(w) * vmag).sum()))
    return {"grad": (grad, k * U * np.abs(gs * w * inv) * dmag), "loss_sum": (loss, loss_bar)}


# ------------------------------------------------------------------------------------------------ SE3_DIST_LOSS
def se3_dist_loss_grad(rot_norm, rot_gt, fc7, trans_w, trans_b, zt_gt, d_rot_prior, d_zt_prior, lw_rot, lw_trans, trans_type="L2", s=3.0,
                       sums_prior=(0.0, 0.0), mutant=None):
    """rot_loss = 1 - (rot_gt . rot_est_norm)^2, trans_loss = f(zoom_trans_est - zoom_trans_gt) with zoom_trans_est = fc7 Wt^T + bt
    recomputed; MakeLoss(grad_scale = LW_ROT / LW_TRANS).  Both gradients are ADDED to the prior contents; loss_sums2 accumulate.
    d_rot_norm: the dot product is 4 roundings, . lw (the 2 is exact), . g_i, + prior = 7 -> k = 14, S = |prior| + 2 |lw| D |g_i|, D = sum|g q|.
    tz: a 257-term sum (bias + 256 products): 2 257 U (|bt| + sum|fc7 wt|), carried through f' (slope 0 / 2 / s^2) and lw; the residual's
    own subtraction adds 2 U (|tz| + |gt|); then lw . f' and + prior: 2 roundings -> 4 U (|prior| + |lw f'|).
    loss_sums2[0]: B + 1 terms of magnitude 1 + D^2, p = 6; [1]: 3 B + 1 terms, p = 4, plus the carried tz bars times |f'|."""
    _check_mutant("se3_dist_loss_grad", mutant)
    q, g, x, wt, bt, gt = f64(rot_norm), f64(rot_gt), f64(fc7), f64(trans_w), f64(trans_b), f64(zt_gt)
    pr, pz = f64(d_rot_prior), f64(d_zt_prior)
    lwr, lwt, s = sc(lw_rot), sc(lw_trans), sc(s)
    B = q.shape[0]
    dot = (g * q).sum(axis=1, keepdims=True)
    D = np.abs(g * q).sum(axis=1, keepdims=True)
    inc_r = -2.0 * lwr * dot * g
    tz = x @ wt.T + bt[None]
    tz_bar = 2.0 * 257.0 * U * (np.abs(x) @ np.abs(wt).T + np.abs(bt)[None])
    r = tz - gt
    r_bar = tz_bar + 2.0 * U * (np.abs(tz) + np.abs(gt))
    v, df = elem_loss(r, trans_type, s)
    slope2 = {"L1": 0.0, "L2": 2.0, "smooth_L1": s * s}[trans_type] * np.ones_like(r)   # |d f' / d r|
    if trans_type == "smooth_L1":
        slope2 = np.where(np.abs(r) < 1.0 / (s * s), slope2, 0.0)
    inc_z = lwt * df
    if mutant == "overwrite_not_add":
        pr, pz = np.zeros_like(pr), np.zeros_like(pz)
    d_rot = pr + inc_r
    d_zt = pz + inc_z
    d_rot_bar = 14.0 * U * (np.abs(pr) + 2.0 * abs(lwr) * D * np.abs(g))
    d_zt_bar = abs(lwt) * slope2 * r_bar + 4.0 * U * (np.abs(pz) + np.abs(inc_z))
    s0, s1 = sc(sums_prior[0]), sc(sums_prior[1])
    rot_sum = s0 + float((1.0 - dot * dot).sum())
    rot_sum_bar = 2.0 * (B + 1 + 6) * U * (abs(s0) + float((1.0 + D * D).sum()))
    vmag, _ = _elem_mag(np.abs(tz) + np.abs(gt), trans_type, s, r)
    trans_sum = s1 + float(v.sum())
    trans_sum_bar = float((np.abs(df) * r_bar).sum()) + 2.0 * (3 * B + 1 + 4) * U * (abs(s1) + float(vmag.sum()))
    return {"d_rot_norm": (d_rot, d_rot_bar), "d_zoom_trans": (d_zt, d_zt_bar), "rot_loss_sum": (rot_sum, rot_sum_bar),
            "trans_loss_sum": (trans_sum, trans_sum_bar), "trans_residual": (r, r_bar)}


# ------------------------------------------------------------------------------------------------ pose head
def quat_normalize(rot):
    """L2Normalization(instance): y = x / sqrt(sum x^2 + 1e-10).  roundings: x^2, three adds, + eps (and the rounded eps), sqrt, the
    division = 7 -> k = 14, S = |y| (one quotient)."""
    q = f64(rot)
    n = np.sqrt((q * q).sum(axis=1, keepdims=True) + L2N_EPS)
    y = q / n
    return {"rot_norm": (y, 14.0 * U * np.abs(y))}


def _lrelu_d(y, mutant=None):
    """LeakyReLU'(.) from the activation's own sign: 1 where y > 0, SLOPE elsewhere (y == 0 included)"""
    pos = (y >= 0.0) if mutant == "lrelu0_is_1" else (y > 0.0)
    return np.where(pos, 1.0, SLOPE)


def pose_head_bwd(fc6a, fc7, rot_raw, d_rot_norm, d_trans, fc7_w, rot_w, trans_w, mutant=None):
    """backward of rot_est_norm = L2Normalization(rot), rot = fc7 Wr^T, zoom_trans = fc7 Wt^T (inverse ZoomTrans backward = identity),
    fc7 = LeakyReLU(fc6a W7^T + b7), fc6a = LeakyReLU(z6):
      d_rot = (g - y (y . g)) / n            14 roundings on the longest path (n: 7, y . g: 4, y dot, -, /) -> k = 28,
                                             S = (|g_i| + |y_i| sum|y g|) / n
      dz7 = LeakyReLU'(fc7) (d_rot Wr + d_trans Wt)      7-term sum, p = 2 (the slope product and the rounded 0.1), d_rot's bar carried
                                                         through sum|wr|
      dz6 = LeakyReLU'(fc6a) (dz7 W7)                    256-term sum, p = 2, dz7's bar carried through sum|w7|"""
    _check_mutant("pose_head_bwd", mutant)
    a6, a7, q, g, dt = f64(fc6a), f64(fc7), f64(rot_raw), f64(d_rot_norm), f64(d_trans)
    w7, wr, wt = f64(fc7_w), f64(rot_w), f64(trans_w)
    n = np.sqrt((q * q).sum(axis=1, keepdims=True) + L2N_EPS)
    y = q / n
    ydg = (y * g).sum(axis=1, keepdims=True)
    proj = 0.0 if mutant == "norm_bwd_no_projection" else y * ydg
    d_rot = (g - proj) / n
    d_rot_bar = 28.0 * U * (np.abs(g) + np.abs(y) * np.abs(y * g).sum(axis=1, keepdims=True)) / n
    m7, m6 = _lrelu_d(a7, mutant), _lrelu_d(a6, mutant)
    dz7 = m7 * (d_rot @ wr + dt @ wt)
    mag7 = np.abs(d_rot) @ np.abs(wr) + np.abs(dt) @ np.abs(wt)
    dz7_bar = m7 * (d_rot_bar @ np.abs(wr) + 2.0 * (7 + 2) * U * mag7)
    dz6 = m6 * (dz7 @ w7)
    dz6_bar = m6 * (dz7_bar @ np.abs(w7) + 2.0 * (256 + 2) * U * (np.abs(dz7) @ np.abs(w7)))
    return {"d_rot": (d_rot, d_rot_bar), "dz7": (dz7, dz7_bar), "dz6": (dz6, dz6_bar)}


def fc_wgrad(dz, x):
    """dW[o][i] = sum_b dz[b][o] x[b][i], db[o] = sum_b dz[b][o]: B-term sums, p = 0 (fused multiply-adds)"""
    a, xx = f64(dz), f64(x)
    B = a.shape[0]
    return {"dW": (a.T @ xx, 2.0 * B * U * (np.abs(a).T @ np.abs(xx))), "db": (a.sum(axis=0), 2.0 * B * U * np.abs(a).sum(axis=0))}


def deconv4x4s2_tiny_bwd(x, dy, w_iohw, OH, OW, crop=1, mutant=None):
    """backward of Crop(Deconvolution(x, k4, s2, bias), offset (crop, crop), size OH x OW) by float64 autograd of
    sum(y dy), as oracle/train.py builds the decoder.  x (N, H, W, Cin) and dy (N, OH, OW, Cout) NHWC, w (Cin, Cout, 4, 4).
    Bars: dx is a sum of up to 16 Cout products, dW of N H W products, db of N OH OW values: 2 n U sum|term| each (p = 0: multiply-adds),
    sum|term| by the same autograd on the magnitudes."""
    _check_mutant("deconv4x4s2_tiny_bwd", mutant)
    import torch
    import torch.nn.functional as F

    def grads(xn, dyn, wn):
        xt = torch.from_numpy(np.ascontiguousarray(xn.transpose(0, 3, 1, 2))).requires_grad_(True)
        wt = torch.from_numpy(np.ascontiguousarray(wn)).requires_grad_(True)
        bt = torch.zeros(wn.shape[1], dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(xt, wt, bt, stride=2)[:, :, crop:crop + OH, crop:crop + OW]
        gx, gw, gb = torch.autograd.grad((y * torch.from_numpy(np.ascontiguousarray(dyn.transpose(0, 3, 1, 2)))).sum(), (xt, wt, bt))
        return gx.numpy().transpose(0, 2, 3, 1), gw.numpy(), gb.numpy()

    xx, g, w = f64(x), f64(dy), f64(w_iohw)
    N, H, W, _ = xx.shape
    Cout = w.shape[1]
    dx, dw, db = grads(xx, g, w)
    ax, aw, ab = grads(np.abs(xx), np.abs(g), np.abs(w))
    if mutant == "db_window_complement":
        # the bias sees every pixel of the un-cropped (2H + 2) x (2W + 2) output; dy is the gradient of the window, zero outside it
        full = np.zeros((N, 2 * H + 2, 2 * W + 2, Cout))
        full[:, crop:crop + OH, crop:crop + OW] = g
        db = full.sum(axis=(0, 1, 2)) - db
    return {"dx": (dx, 2.0 * 16 * Cout * U * ax), "dW": (dw, 2.0 * N * H * W * U * aw), "db": (db, 2.0 * N * OH * OW * U * ab)}


# ------------------------------------------------------------------------------------------------ optimizers
def sgd_momentum(w, g, mom, lr, momentum, wd, rescale=1.0, mom_bar=0.0, mutant=None):
    """mx.optimizer.SGD: mom = momentum mom - lr (rescale g + wd w); w += mom.
    mom: roundings rescale g, wd w, +, lr ., momentum mom, - = 6 -> k = 12, S = |momentum mom| + |lr rescale g| + |lr wd w|;
    w: one more -> k = 14, S + |w|.  `mom_bar` (the bar of the incoming momentum, when the caller chains steps without re-reading it)
    is carried as momentum mom_bar."""
    _check_mutant("sgd_momentum", mutant)
    w0, gg, m0 = np.asarray(w, np.float64), f64(g), np.asarray(mom, np.float64)   # float32 -> float64 is exact
    lr, mu, wd, rs = sc(lr), sc(momentum), sc(wd), sc(rescale)
    if mutant == "wd_inside_momentum":
        m = mu * (m0 - lr * wd * w0) - lr * rs * gg
    elif mutant == "momentum_sign":
        m = -mu * m0 - lr * (rs * gg + wd * w0)
    else:
        m = mu * m0 - lr * (rs * gg + wd * w0)
    S = np.abs(mu * m0) + np.abs(lr * rs * gg) + np.abs(lr * wd * w0)
    carried = abs(mu) * np.asarray(mom_bar, np.float64)
    return {"mom": (m, 12.0 * U * S + carried), "w": (w0 + m, 14.0 * U * (S + np.abs(w0)) + carried)}


def sgd_params_step(params, grads, moms, mom_bars, lr, momentum, wd, frozen=(), mutant=None):
    """one update of a parameter dict as MutableModule.update makes it: wd_mult = 0 unless the name ends with _weight (MXNet), tensors
    with lr_mult 0 (`frozen`) untouched.  -> new params (float64), new moms, new mom bars, bars of the new params"""
    _check_mutant("sgd_params_step", mutant)
    new, nm, nb, bars = {}, {}, {}, {}
    for k, w in params.items():
        if k in frozen:
            new[k], nm[k], nb[k], bars[k] = f64(w), moms[k], mom_bars[k], np.zeros(np.shape(w))
            continue
        decay = wd if (k.endswith("_weight") or mutant == "wd_on_bias") else 0.0
        r = sgd_momentum(w, grads[k], moms[k], lr, momentum, decay, 1.0, mom_bar=mom_bars[k])
        new[k], bars[k] = r["w"]
        nm[k], nb[k] = r["mom"]
    return new, nm, nb, bars


def adam_lr_t(lr, t, beta1=0.9, beta2=0.999):
    """mx.optimizer.Adam.update: the bias-corrected rate the caller hands to adam_update"""
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam(w, g, mean, var, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, rescale=1.0, mutant=None):
    """adam_update: g' = rescale g + wd w; mean = b1 mean + (1 - b1) g'; var = b2 var + (1 - b2) g'^2; w -= lr_t mean / (sqrt(var) + eps).
    g': 3 roundings, S_g = |rescale g| + |wd w|.
    mean: g' (3), 1 - b1, its product, b1 mean, + = 7 -> k = 14, S_m = |b1 mean| + (1 - b1) S_g.
    var: g' twice (6), 1 - b2, two products, b2 var, + = 11 -> k = 22, S_v = |b2 var| + (1 - b2) S_g^2.
    w: the step lr_t mean / (sqrt(var) + eps) carries mean's bar through lr_t / den and var's through d den = bar_v / (2 sqrt(var));
    sqrt, + eps, lr_t ., / add 4 roundings of the step (k = 8, S = |step|); the final subtraction 2 U (|w| + |step|)."""
    _check_mutant("adam", mutant)
    w0, gg, m0, v0 = f64(w), f64(g), f64(mean), f64(var)
    lr_t, b1, b2, eps, wd, rs = sc(lr_t), sc(beta1), sc(beta2), sc(eps), sc(wd), sc(rescale)
    gi = rs * gg + (0.0 if mutant == "no_wd" else wd * w0)
    Sg = np.abs(rs * gg) + np.abs(wd * w0)
    m = b1 * m0 + (1.0 - b1) * gi
    v = b2 * v0 + (1.0 - b2) * gi * gi
    m_bar = 14.0 * U * (np.abs(b1 * m0) + (1.0 - b1) * Sg)
    v_bar = 22.0 * U * (np.abs(b2 * v0) + (1.0 - b2) * Sg * Sg)
    den = np.sqrt(v + eps) if mutant == "sqrt_v_plus_eps" else np.sqrt(v) + eps
    step = lr_t * m / den
    den_bar = v_bar / (2.0 * np.sqrt(np.maximum(v, 1e-300)))
    step_bar = abs(lr_t) * m_bar / den + np.abs(step) * den_bar / den + 8.0 * U * np.abs(step)
    return {"mean": (m, m_bar), "var": (v, v_bar), "w": (w0 - step, step_bar + 2.0 * U * (np.abs(w0) + np.abs(step)))}


# ------------------------------------------------------------------------------------------------ shared seeded inputs
FLOW_SIZES = (4, 1020, 4 * (256 * 1024 + 37))
FLOW_ARGS = dict(normalize_flow=20.0, grad_scale=0.37)
LOGISTIC_SIZES = (1, 257, 5000)
LOGISTIC_SPECIAL = (0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0)
LOGISTIC_GS = 0.03 / 7.0
PM_SIZES = (3, 32768 + 1, 144000)
PM_CASES = (("L1", 1.0), ("L2", 1.0), ("smooth_L1", 1.0), ("smooth_L1", 2.0), ("smooth_L1", 3.0))
PM_ARGS = dict(norm_term=0.5, grad_scale=0.1 / 3000.0)      # 1 / norm_term = 2 exactly: the special residuals below stay bitwise exact
SE3_BATCHES = (1, 64, 65, 130)
SE3_ARGS = dict(lw_rot=0.8, lw_trans=1.3, s=2.0)
QUAT_BATCHES = (1, 65)
POSE_BATCHES = (1, 3, 17)
FC_SHAPES = ((1, 4, 256), (16, 3, 256), (5, 256, 256), (3, 7, 33))
DECONV_SHAPES = ((2, 8, 10, 2, 2, 15, 20), (1, 15, 20, 2, 2, 30, 40), (1, 3, 5, 1, 4, 5, 9), (2, 4, 4, 4, 1, 7, 7))   # N H W Cin Cout OH OW
DECONV_DY_CSTRIDE, DECONV_DY_COFF = 70, 66
OPT_SIZES = (1, 255, 100003)
SGD_LRS = (1e-2, 3e-3, 2e-2)
SGD_CASES = ((0.0, 1.0), (0.05, 1.0), (0.05, 0.125), (0.0, 0.125))     # (wd, rescale_grad)
SGD_MOMENTUM = 0.9
ADAM_LRS = (1e-2, 3e-3, 2e-2)
ADAM_ARGS = dict(wd=0.01, rescale=0.5)
SL1_THRESHOLDS = (1.0, 0.25, float(np.float32(1.0) / np.float32(9.0)))
GAP = 1e-3         # every residual / activation is bitwise at a special value or at least this far from it


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _residuals(rng, n, lo=0.004, hi=1.5):
    """signed residuals with |r| in [lo, hi), pushed 4 GAP away from every smooth-L1 threshold of s = 1, 2, 3"""
    r = rng.uniform(lo, hi, n)
    for t in SL1_THRESHOLDS:
        r = np.where(np.abs(r - t) < 4 * GAP, t + 4 * GAP, r)
    return r * rng.choice([-1.0, 1.0], n)


def flow_inputs(n):
    rng = np.random.default_rng(1000 + n % 997)
    w = rng.integers(0, 2, n)
    w[:2] = (1, 0)          # both weights occur at every size
    return dict(f_est=_f32(rng.normal(0, 1.0, n)), f_lab=_f32(rng.normal(0, 20.0, n)), wgt=_f32(w))


def logistic_inputs(n):
    """logits with the special values first (0, +-1e-3, +-20, +-100: the last overflow expf on one side), labels in {0, 1}"""
    rng = np.random.default_rng(2000 + n)
    x = rng.normal(0, 3.0, n)
    x = np.where(np.abs(x) < 4 * GAP, 4 * GAP, x)
    k = min(n, len(LOGISTIC_SPECIAL))
    x[:k] = LOGISTIC_SPECIAL[:k]
    return dict(logits=_f32(x), label=_f32(rng.integers(0, 2, n)))


def pm_inputs(n, s):
    """p_est, p_obs, weights.  The first elements carry the special residuals of smooth_l1(scalar = s), t = float32(1 / s^2), all with
    non-zero weight: bitwise 0 (p_est == p_obs != 0), exactly t, 1.5 t (between 1 / s^2 and 1 / s for s > 1), 0.5 t, 2 t, then their
    negatives; p_obs = 0 there and norm_term = 0.5, so (p_est - 0) * 2 is exact.  The rest: |r| in [0.004, 1.5) away from the
    thresholds of s = 1, 2, 3, weights from {0, 1, 0.375}."""
    rng = np.random.default_rng(3000 + n % 997 + int(s))
    t = float(np.float32(1.0) / (np.float32(s) * np.float32(s)))
    b = rng.normal(0, 0.3, n)
    a = b + 0.5 * _residuals(rng, n)
    w = rng.choice([0.0, 1.0, 0.375], n)
    special = [None, t, 1.5 * t, 0.5 * t, 2.0 * t, -t, -1.5 * t, -0.5 * t, -2.0 * t]
    for i, r in enumerate(special[:n]):
        if r is None:
            a[i] = b[i] = 0.3125
        else:
            a[i], b[i] = 0.5 * r, 0.0
        w[i] = (1.0, 0.375)[i % 2]
    return dict(p_est=_f32(a), p_obs=_f32(b), wgt=_f32(w))


def se3_inputs(B):
    """a pose-head state with non-zero prior gradients and loss sums; rot_gt holds the estimate's antipode in row 0 (dot < 0); the
    translation residuals keep GAP from 0 and from the smooth-L1 thresholds"""
    rng = np.random.default_rng(4000 + B)
    q = rng.normal(0, 1, (B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g = q + rng.normal(0, 0.2, (B, 4))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[0] = -g[0]
    fc7 = rng.normal(0, 0.5, (B, 256))
    fc7 = np.where(fc7 < 0, SLOPE * fc7, fc7)
    wt, bt = rng.normal(0, 0.02, (3, 256)), rng.normal(0, 0.05, 3)
    tz = f64(_f32(fc7)) @ f64(_f32(wt)).T + f64(_f32(bt))[None]
    gt = tz - _residuals(rng, 3 * B).reshape(B, 3)
    return dict(rot_norm=_f32(q), rot_gt=_f32(g), fc7=_f32(fc7), trans_w=_f32(wt), trans_b=_f32(bt), zt_gt=_f32(gt),
                d_rot_prior=_f32(rng.normal(0, 0.5, (B, 4))), d_zt_prior=_f32(rng.normal(0, 0.5, (B, 3))), sums_prior=(2.75, -1.5))


def quat_inputs(B):
    """row 0 all zero (-> 0, not NaN); the last row of norm 1e-6 (the eps dominates)"""
    rng = np.random.default_rng(5000 + B)
    q = rng.normal(0, 1, (B, 4))
    q[-1] *= 1e-6 / np.linalg.norm(q[-1])
    q[0] = 0.0
    return dict(rot=_f32(q))


def _activations(rng, shape):
    """LeakyReLU outputs of both signs, |v| >= GAP, one in sixteen exactly 0"""
    v = rng.normal(0, 0.5, shape)
    v = np.where(np.abs(v) < GAP, GAP, v)
    v = np.where(v < 0, SLOPE * np.minimum(v, -GAP / SLOPE), v)
    v[rng.random(shape) < 1.0 / 16.0] = 0.0
    return v


def pose_inputs(B):
    """fc6a / fc7 with exact zeros; rot_raw row 0 of norm 1e-4 (the 1e-10 eps is 1 % of its squared norm)"""
    rng = np.random.default_rng(6000 + B)
    q = rng.normal(0, 1, (B, 4))
    q[0] *= 1e-4 / np.linalg.norm(q[0])
    return dict(fc6a=_f32(_activations(rng, (B, 256))), fc7=_f32(_activations(rng, (B, 256))), rot_raw=_f32(q),
                d_rot_norm=_f32(rng.normal(0, 0.3, (B, 4))), d_trans=_f32(rng.normal(0, 0.3, (B, 3))),
                fc7_w=_f32(rng.normal(0, 1.0 / 16, (256, 256))), rot_w=_f32(rng.normal(0, 0.05, (4, 256))),
                trans_w=_f32(rng.normal(0, 0.05, (3, 256))))


def fc_inputs(B, Out, In):
    rng = np.random.default_rng(7000 + 131 * B + 17 * Out + In)
    return dict(dz=_f32(rng.normal(0, 1, (B, Out))), x=_f32(rng.normal(0, 1, (B, In))))


DECONV_SENTINEL = 1.0e6     # fills the channels of the wide buffers that the kernels must not read


def deconv_inputs(N, H, W, Cin, Cout, OH, OW):
    """-> x (N,H,W,Cin), dy (N,OH,OW,Cout), w (Cin,Cout,4,4), and the wide NHWC buffers the kernel reads them from: x_wide with
    x_cstride = Cin + 3, dy_wide with 70 channels and dy in [66, 66 + Cout); every other channel holds DECONV_SENTINEL"""
    rng = np.random.default_rng(8000 + 1000 * N + 100 * H + 10 * Cin + Cout)
    x, dy = _f32(rng.normal(0, 1, (N, H, W, Cin))), _f32(rng.normal(0, 1, (N, OH, OW, Cout)))
    w = _f32(rng.normal(0, 0.3, (Cin, Cout, 4, 4)))
    x_wide = np.full((N, H, W, Cin + 3), DECONV_SENTINEL, np.float32)
    x_wide[..., :Cin] = x
    dy_wide = np.full((N, OH, OW, DECONV_DY_CSTRIDE), DECONV_SENTINEL, np.float32)
    dy_wide[..., DECONV_DY_COFF:DECONV_DY_COFF + Cout] = dy
    return dict(x=x, dy=dy, w=w, x_wide=x_wide, dy_wide=dy_wide)


def opt_inputs(n, steps=3):
    """weights, `steps` gradients with magnitudes log-uniform in [1e-4, 1] (Adam's sqrt(v) then spans 3e-6 .. 3e-2 around eps), and
    non-zero optimizer states.  Element 0 is fixed (n = 1 is one of the sizes): a weight whose decay term is as large as its gradient and
    a second moment near eps^2 ... eps, where sqrt(v) + eps and sqrt(v + eps) differ most"""
    rng = np.random.default_rng(9000 + n % 997)
    g = [rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n) for _ in range(steps)]
    w, mom, mean, var = rng.normal(0, 0.3, n), rng.normal(0, 0.01, n), rng.normal(0, 1e-3, n), 10.0 ** rng.uniform(-9, -4, n)
    w[0], mom[0], mean[0], var[0] = 0.25, 0.01, 1e-3, 1e-9
    for k, v in enumerate((3e-3, -2e-3, 1e-3)[:steps]):
        g[k][0] = v
    return dict(w=_f32(w), grads=[_f32(x) for x in g], mom=_f32(mom), mean=_f32(mean), var=_f32(var))
