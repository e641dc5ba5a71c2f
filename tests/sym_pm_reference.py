"""float64 restatement of the symmetry-aware point-matching loss (csrc/train.hip: dim_pm_sym_loss_grad), its rounding bars, named mutants
and the seeded inputs the CPU and GPU tests share.  Conventions and bar formulas are those of tests/train_head_reference.py.

Per pair b of class c with the symmetry set {[Rs | ts]} (identity first; an empty range = the identity alone):
    G_s = [R_g Rs | R_g ts + t_g]     target_s = G_s x     L_s = sum_{i,k} w f((p_est - target_s) / norm)
    s*  = 0; for s = 1 .. in order: s replaces s* only if L_s is finite and L_s < L_{s*}
    grad = gs w f'((p_est - target_{s*}) / norm) / norm      loss_sum += L_{s*}

Roundings of the kernel, and the bars they give (U = 2^-24, V = 2^-53):
  target   G_s is composed in float64 from float32 factors (products exact, three additions) and applied in float64 (three products,
           three additions); ONE float32 rounding of the sum.  k = 2 for that rounding, S = sum_j |R_g| |Rs| |x| + |R_g| |ts| + |t_g|,
           plus 16 V S for the float64 steps:  bar_t = (2 U + 16 V) S.
  L_s      3 N terms w f(r), r = (a - t32) inv with t32 the float32 target: p = 8 roundings inside a term as in pm_loss_grad (a - t32,
           the rounded inv, . inv, up to four in f, the multiply-add), summed lane, wave, workgroup, tile.  Every one of these is a
           relative error of the term itself (fl(a - t32) = (a - t32)(1 + d): the subtraction of two float32 numbers is ONE rounding of
           their difference, whatever |a| + |t32| is), so the sum's bar is 2 (3 N + 8) U sum |w| f(m) with m = |r| + inv bar_t, the
           residual's magnitude with the target's rounding in it.  tests/train_head_reference.py counts a difference as |a| + |b|
           instead; that bound holds too but is ~100 x wider here (|a|, |t| ~ 1 against |r| ~ 0.01) and would hide the target's
           rounding, which is carried on its own: sum |w| |f'|(m) inv bar_t.
  loss_sum B + 1 terms (the accumulator's prior value is one): the L_{s*} bars plus 2 (B + 1) U (|prior| + sum |L_{s*}|).
  grad     pm_loss_grad's bar for (p_est, target, w), plus the target's rounding through f'' (0 | 2 | s^2 in the quadratic zone).
            The GPU test compares grad bitwise with dim_pm_loss_grad on target_out instead; this bar serves the mutants.
"""
import numpy as np

from train_head_reference import GAP, LOSS_TYPES, U, _elem_mag, _f32, _residuals, elem_loss, f64, sc, worst_ratio  # noqa: F401

V = 2.0 ** -53
MUTANTS = ("sym_after_gt", "sym_translation_dropped", "first_sym_only", "grad_from_sym0", "tie_to_last")
CHUNK = 16          # kPmSymChunk of csrc/train.hip: symmetries per workgroup of the first pass
TILE = 512          # kPmSymTile: points per workgroup of the first pass


def _sets(sym, sym_off, class_index):
    """per pair: its (S,3,4) float64 set, or None for a class index outside the table; an empty range = the identity"""
    sym, sym_off = f64(sym).reshape(-1, 3, 4), np.asarray(sym_off, np.int64)
    out = []
    for c in np.asarray(class_index, np.int64):
        if c < 0 or c >= sym_off.size - 1:
            out.append(None)
        elif sym_off[c + 1] <= sym_off[c]:
            out.append(np.eye(4)[None, :3])
        else:
            out.append(sym[sym_off[c]:sym_off[c + 1]])
    return out


def compose(pose, S, mutant=None):
    """G = pose . S: the ground truth applied AFTER the symmetry -> (R (3,3), t (3,), |.| bounds of both)"""
    Rg, tg, Rs, ts = pose[:, :3], pose[:, 3], S[:, :3], S[:, 3]
    if mutant == "sym_translation_dropped":
        ts = np.zeros(3)
    if mutant == "sym_after_gt":
        return Rs @ Rg, Rs @ tg + ts, np.abs(Rs) @ np.abs(Rg), np.abs(Rs) @ np.abs(tg) + np.abs(ts)
    return Rg @ Rs, Rg @ ts + tg, np.abs(Rg) @ np.abs(Rs), np.abs(Rg) @ np.abs(ts) + np.abs(tg)


def pm_sym_loss_grad(p_est, points_model, weights, tgt_pose, sym, sym_off, class_index, norm_term, grad_scale, loss_type="L1", s=1.0,
                     max_sym=4096, loss_prior=0.0, mutant=None):
    """-> {"best_sym": (B,) int (-1: bad class or a set above max_sym), "target": (value, bar) (B,3,N), "L": per pair (values, bars) over
    its set, "loss_sum": (value, bar), "grad": (value, bar)}"""
    assert mutant is None or mutant in MUTANTS, mutant
    a, x, w, poses = f64(p_est), f64(points_model), f64(weights), f64(tgt_pose)
    inv, gs, s = 1.0 / sc(norm_term), sc(grad_scale), sc(s)
    B, _, N = a.shape
    best = np.zeros(B, np.int64)
    target, target_bar = np.zeros_like(a), np.zeros_like(a)
    Ls, L_sel, L_sel_bar = [], [], []
    for b, S_all in enumerate(_sets(sym, sym_off, class_index)):
        if S_all is None or S_all.shape[0] > max_sym:
            best[b] = -1
            Ls.append((np.zeros(0), np.zeros(0)))
            continue
        tg, tb, L, Lb = [], [], [], []
        for S in S_all:
            Rm, tv, Ra, ta = compose(poses[b], S, mutant)
            t = Rm @ x[b] + tv[:, None]
            bar_t = (2.0 * U + 16.0 * V) * (Ra @ np.abs(x[b]) + ta[:, None])
            r = (a[b] - t) * inv
            v, _ = elem_loss(r, loss_type, s)
            vmag, dmag = _elem_mag(np.abs(r) + inv * bar_t, loss_type, s, r)
            tg.append(t); tb.append(bar_t)
            L.append(float((w[b] * v).sum()))
            Lb.append(2.0 * (3 * N + 8) * U * float((np.abs(w[b]) * vmag).sum()) + float((np.abs(w[b]) * dmag * inv * bar_t).sum()))
        k = 0
        if mutant != "first_sym_only":
            for i in range(1, len(L)):
                if np.isfinite(L[i]) and (L[i] <= L[k] if mutant == "tie_to_last" else L[i] < L[k]):
                    k = i
        best[b] = k
        kg = 0 if mutant == "grad_from_sym0" else k      # the symmetry the gradient (and target_out) is taken from
        target[b], target_bar[b] = tg[kg], tb[kg]
        Ls.append((np.array(L), np.array(Lb)))
        L_sel.append(L[k]); L_sel_bar.append(Lb[k])
    ok = best >= 0
    r = (a - target) * inv                                  # pm_loss_grad's formula and bar, on the un-rounded float64 target
    _, df = elem_loss(r, loss_type, s)
    _, dmag = _elem_mag((np.abs(a) + np.abs(target)) * inv, loss_type, s, r)
    g = (gs * w * df * inv, {"L1": 6.0, "L2": 12.0, "smooth_L1": 16.0}[loss_type] * U * np.abs(gs * w * inv) * dmag)
    slope2 = {"L1": 0.0, "L2": 2.0, "smooth_L1": s * s}[loss_type] * np.ones_like(a)
    if loss_type == "smooth_L1":
        slope2 = np.where(np.abs(r) < 1.0 / (s * s), slope2, 0.0)
    grad = np.where(ok[:, None, None], g[0], 0.0)
    grad_bar = np.where(ok[:, None, None], g[1] + np.abs(gs * w * inv) * slope2 * inv * target_bar, 0.0)
    prior = sc(loss_prior)
    loss = prior + float(np.sum(L_sel))
    loss_bar = float(np.sum(L_sel_bar)) + 2.0 * (B + 1) * U * (abs(prior) + float(np.sum(np.abs(L_sel))))
    return {"best_sym": best, "target": (target, target_bar), "L": Ls, "loss_sum": (loss, loss_bar), "grad": (grad, grad_bar)}


# ------------------------------------------------------------------------------------------------ shared seeded inputs
SIZES = (3, 257, 3000)                  # one point tile with a padded point; one tile, not a multiple of the wave; six tiles, the last partial
CASES = (("L1", 1.0), ("L2", 1.0), ("smooth_L1", 2.0))
ARGS = dict(norm_term=0.5, grad_scale=0.1 / 3000.0)
CLASSES = ("plain", "flip", "axis")     # 1, 2 and 33 symmetries
FLIP_OFFSET = (0.05, -0.1, 0.025)
AXIS_OFFSET = (0.1, -0.05, 0.15)
AXIS_STEP = 0.096                       # ceil(pi / 0.096) = 33 rotations: chunks of 16, 16 and 1
# the symmetry the estimate sits at, per variant, for the pairs of class "flip" and "axis": index 0, the last index of either set,
# and 16 = the first symmetry of the second chunk
TRUE_SYM = ((0, 0), (1, 32), (1, 16))
RES_HI = 0.03                           # residuals |r| in [0.004, 0.03) of the normalised unit: a tenth of what the nearest wrong symmetry adds


def variant_of(n, loss_type):
    """which TRUE_SYM row the GPU test runs at (n, loss type): all three occur for every size and every type"""
    return (SIZES.index(n) + LOSS_TYPES.index(loss_type)) % 3


def class_symmetries():
    from lib.utils.symmetry import rotation_about_axis

    m = np.eye(4)
    m[:3, :3] = rotation_about_axis(np.pi, (1.0, 1.0, 0.0))
    m[:3, 3] = np.asarray(FLIP_OFFSET) - m[:3, :3].dot(FLIP_OFFSET)      # 180 degrees about an axis through FLIP_OFFSET
    return {"flip": {"symmetries_discrete": [m.reshape(-1).tolist()]},
            "axis": {"symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": list(AXIS_OFFSET)}]}}


def tables(symmetries=None, classes=CLASSES, step=AXIS_STEP):
    """-> sym (Stot,3,4) float32, sym_off int32, max_sym, as MutableModule uploads them"""
    from lib.utils.symmetry import symmetry_tables

    sym, off, max_sym = symmetry_tables(classes, class_symmetries() if symmetries is None else symmetries, step)
    return _f32(sym), off, max_sym


def _poses(rng, B):
    q = rng.normal(0, 1, (B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                   2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                   2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(B, 3, 3)
    t = np.array([0.1, -0.05, 0.8]) + rng.normal(0, 0.05, (B, 3))
    return _f32(np.concatenate([Rm, t[:, :, None]], axis=2))


def _cloud(rng, B, n):
    """model points (sigma 0.3) with a zero-padded, zero-weight tail of max(1, n / 10) slots, as the loader leaves a class with fewer
    points than NUM_3D_SAMPLE"""
    x = rng.normal(0, 0.3, (B, 3, n))
    w = np.ones((B, 3, n))
    pad = max(1, n // 10)
    x[:, :, n - pad:] = 0.0
    w[:, :, n - pad:] = 0.0
    return _f32(x), _f32(w)


def _estimate(rng, x, pose, sym, sym_off, class_index, true_sym):
    """p_est = G_k x + norm * residuals, k = true_sym[b] within the pair's set"""
    B, _, n = x.shape
    a = np.zeros((B, 3, n))
    for b, S_all in enumerate(_sets(sym, sym_off, class_index)):
        Rm, tv, _, _ = compose(f64(pose)[b], S_all[true_sym[b]])
        a[b] = Rm @ f64(x)[b] + tv[:, None] + ARGS["norm_term"] * _residuals(rng, 3 * n, hi=RES_HI).reshape(3, n)
    return _f32(a)


def inputs(n, variant=0):
    """B = 3 pairs of the classes plain / flip / axis; see TRUE_SYM for `variant`"""
    rng = np.random.default_rng(11000 + 10 * n + variant)
    sym, sym_off, max_sym = tables()
    cls = np.array([0, 1, 2], np.int32)
    pose = _poses(rng, 3)
    x, w = _cloud(rng, 3, n)
    true_sym = (0,) + TRUE_SYM[variant]
    return dict(p_est=_estimate(rng, x, pose, sym, sym_off, cls, true_sym), points_model=x, weights=w, tgt_pose=pose, sym=sym,
                sym_off=sym_off, class_index=cls, max_sym=max_sym, true_sym=np.array(true_sym))


def tie_inputs(n=257):
    """one class whose set lists the flip twice, [I, S, S]: L_1 and L_2 are the same bits, the estimate sits at S -> index 1"""
    rng = np.random.default_rng(12000 + n)
    table, off, _ = tables()
    S = f64(table)[off[1] + 1]
    sym = _f32(np.stack([np.eye(4)[:3], S, S]))
    sym_off, cls = np.array([0, 3], np.int32), np.array([0, 0], np.int32)
    pose = _poses(rng, 2)
    x, w = _cloud(rng, 2, n)
    return dict(p_est=_estimate(rng, x, pose, sym, sym_off, cls, (2, 1)), points_model=x, weights=w, tgt_pose=pose, sym=sym,
                sym_off=sym_off, class_index=cls, max_sym=3, true_sym=np.array([1, 1]))


def kernel_args(inp):
    """the arrays of an input set that the reference takes"""
    return {k: inp[k] for k in ("p_est", "points_model", "weights", "tgt_pose", "sym", "sym_off", "class_index")}


def margins(ref):
    """per pair: (runner-up L - winner L) / (the sum of their two bars); inf for a set of one"""
    out = []
    for (L, Lb), k in zip(ref["L"], ref["best_sym"]):
        if L.size < 2:
            out.append(np.inf)
            continue
        others = np.delete(np.arange(L.size), k)
        j = others[np.argmin(L[others])]
        out.append((L[j] - L[k]) / (Lb[j] + Lb[k]))
    return np.array(out)
