"""CPU: the normal equations of the four Gauss-Newton pose stages against calculus.

The restatements (tests/icp_reference.py, flow_pnp_reference.py, photo_reference.py, sil_reference.py) write the Jacobian with the
formulas of the kernels; tests/gn_calculus.py states only each stage's residual in float64 torch and lets autograd differentiate it
through matrix_exp of the left twist.  For every small scene the GPU files run (gpu_batches() of test_photo_host, test_sil_host and
test_flow_pnp_host, with and without their boxes; the scenes of icp_terms_scenes) and the corrections T_0 = I, T_1, T_2 of the
restatement's own first iterations, the restatement's sums must equal autograd's: counts EQUAL, every entry of A, g and term 28 within
BAR = 64 eps64 of abs_terms (the same sum over the absolute per-point contributions), and g within the same bar of the gradient of the
robust cost itself.  The bar is derived, not tuned: a per-point term is about ten rounded operations and a float64 sum adds a few eps
per level of whatever order numpy and torch use.

No decision of any scene and correction used here or in tests/test_gpu_gn_terms.py may be borderline: the least margin is >= 1e-9 in
the units of the decision.  One decision is exempt, with the reason: photo's bilinear cell at T = I.  There every template pixel
projects onto its own centre by construction, U is the integer X up to the rounding of d (X - cx) / fx . fx / d + cx, and which of the
two cells that meet there is read is decided by that rounding, not by the scene; no seed or pose can move it.  The residual is
continuous across the boundary, the gradient is one-sided.  gn_calculus takes U with the operations of the issue's formula,
((fx px / pz + cx) - (s - 1)/2) / s, as the restatement and the kernel do, and equal counts and sums within the bar show that all
three read the same cells.  From T_1 on the cell margin is asserted like every other.

Planted defects (test_planted_defects_are_over_the_bar): each one, put into a PRIVATE copy of the restated formula below -- never into
the committed restatement -- exceeds the bar by at least 10 x; the private copy without a defect is within it."""
import functools

import numpy as np

import gn_calculus as gc
import icp_reference as ir
import icp_terms_scenes as sc
import flow_pnp_reference as fr
import photo_reference as pr
import sil_reference as sr
import test_flow_pnp_host as pnp_host
import test_photo_host as photo_host
import test_sil_host as sil_host

MIN_MARGIN = 1e-9
EYE, ZERO = np.eye(3), np.zeros(3)


def step(R, t, A, g, N):
    """one damped Gauss-Newton update as every stage takes it (icp_reference.gn_step on unpacked sums)"""
    return ir.gn_step(R, t, gc.pack(A, g, N, 0.0))[:2]


def ratio_to_bar(S, c):
    """|S - autograd's terms| in units of the bar, per term (the count is compared apart; a term nothing contributes to must be 0)"""
    diff = np.abs(np.asarray(S, np.float64) - c["terms"])
    bar = gc.BAR * c["abs_terms"]
    out = np.where(diff == 0, 0.0, diff / np.where(bar > 0, bar, np.finfo(np.float64).tiny))
    out[27] = 0.0
    return out


def grad_ratio(c):
    bar = gc.BAR * c["abs_terms"][21:27]
    diff = np.abs(c["g"] - c["grad_cost"])
    return np.where(diff == 0, 0.0, diff / np.where(bar > 0, bar, np.finfo(np.float64).tiny))


# ------------------------------------------------------------------------------------------------------------------ the cases
def photo_chain(pl, K, a, b, levels, iters):
    """the restatement's own iterations -> [(lvl, R, t, packed sums)] in the order photo_refine visits them"""
    R, t, out = EYE, ZERO, []
    for lvl in range(levels - 1, -1, -1):
        for _ in range(iters):
            A, g, N, wrr = pr.normal_equations(pl, lvl, K, R, t, a, b, photo_host.HUBER, photo_host.GATE)
            out.append((lvl, R, t, gc.pack(A, g, N, wrr)))
            R, t = step(R, t, A, g, N)
    return out


@functools.lru_cache(maxsize=None)
def photo_cases():
    """-> [(label, restatement's sums, autograd)]: both levels of GPU_LEVELS = 2 over three iterations each, level 0 alone from the
    identity (the call with levels = 1), and the two-level call with one iteration per level"""
    out = []
    for which, g in enumerate(photo_host.gpu_batches()):
        for with_bbox in (True, False):
            for b in range(len(g["pose_in"])):
                K = g["K_per_sample"][b]
                pl = pr.planes(g["image_observed"][b], g["image_rendered"][b], g["depth_rendered"][b], g["bbox"][b] if with_bbox else None,
                               photo_host.GPU_LEVELS)
                a, bias, ok = pr.gain_bias(pr.gain_sums(pl))
                assert ok
                for levels, iters in ((2, 3), (1, 3), (2, 1)):
                    for k, (lvl, R, t, S) in enumerate(photo_chain(pl, K, a, bias, levels, iters)):
                        c = gc.photo(pl, lvl, K, R, t, a, bias, photo_host.HUBER, photo_host.GATE)
                        out.append((("photo", which, with_bbox, b, levels, iters, k, lvl), S, c))
    return out


@functools.lru_cache(maxsize=None)
def sil_cases():
    out = []
    for which, g in enumerate(sil_host.gpu_batches()):
        for with_bbox in (True, False):
            for b in range(len(g["pose_in"])):
                K, d, field = g["K_per_sample"][b], g["depth_rendered"][b, 0], g["field"][b]
                box = g["bbox"][b] if with_bbox else None
                p0, _ = sr.contour_points(d, K, box)
                R, t = EYE, ZERO
                for k in range(3):
                    A, gg, N, ee, _ = sr.normal_equations(p0 @ R.T + t, field, K, sil_host.HUBER, sil_host.GATE)
                    c = gc.sil(d, field, K, R, t, sil_host.HUBER, sil_host.GATE, box)
                    out.append((("sil", which, with_bbox, b, k), gc.pack(A, gg, N, ee), c))
                    R, t = step(R, t, A, gg, N)
    return out


@functools.lru_cache(maxsize=None)
def pnp_cases():
    """warm = 2: iterations 0 and 1 are warm (every point, w = 1), iteration 2 is gated"""
    out = []
    for name, H, W, cases, rep in pnp_host.gpu_batches():
        for with_bbox in (True, False):
            for b, case in enumerate(cases):
                box = case["bbox"] if with_bbox else None
                p, uv = fr.correspondences(case["depth"], case["flow"], case["K"], rep, case["visible"], box)
                R, t = EYE, ZERO
                for k in range(3):
                    gated = k >= pnp_host.WARM
                    A, gg, N, ee = fr.normal_equations(p @ R.T + t, uv, case["K"], gated, pnp_host.HUBER, pnp_host.GATE)
                    c = gc.flow_pnp(case["depth"], case["flow"], case["K"], R, t, gated, pnp_host.HUBER, pnp_host.GATE, rep, case["visible"], box)
                    out.append((("pnp", name, rep, with_bbox, b, k), gc.pack(A, gg, N, ee), c))
                    R, t = step(R, t, A, gg, N)
    return out


@functools.lru_cache(maxsize=None)
def icp_cases():
    """the scenes of tests/test_gpu_icp_terms.py at the corrections of the float32 model's chain, through s.truth(R, t)"""
    out = []
    for s in sc.all_scenes():
        for k, (R, t) in enumerate(sc.model_chain(s)):
            truth, unit = s.truth(R, t)
            c = gc.icp(s.dr, s.do, s.K, R, t, sc.MAX_DIST, s.mask, s.bbox)
            out.append((("icp", s.name, k), truth, c))
    return out


STAGES = {"icp": icp_cases, "pnp": pnp_cases, "sil": sil_cases, "photo": photo_cases}


# ------------------------------------------------------------------------------------------------------------------ restatement == calculus
def _restatement_equals_autograd(stage):
    cases = STAGES[stage]()
    worst, worst_grad, counts = (0.0, None), (0.0, None), []
    for label, S, c in cases:
        assert int(S[27]) == c["count"], (label, S[27], c["count"])       # EQUAL
        counts.append(c["count"])
        r, rg = ratio_to_bar(S, c), grad_ratio(c)
        worst = max(worst, (float(r.max()), label), key=lambda x: x[0])
        worst_grad = max(worst_grad, (float(rg.max()), label), key=lambda x: x[0])
    print("{}: {} linearisations, {} .. {} points; restatement against autograd: worst term error / bar {:.3g} at {}; g against the "
          "gradient of the cost: {:.3g} at {}".format(stage, len(cases), min(counts), max(counts), worst[0], worst[1], worst_grad[0],
                                                      worst_grad[1]))
    assert worst[0] <= 1.0, worst
    assert worst_grad[0] <= 1.0, worst_grad
    assert max(counts) >= ir.MIN_POINTS
    return cases


def test_icp_restatement_equals_autograd():
    cases = _restatement_equals_autograd("icp")
    # and the unit of the ICP bar of tests/test_gpu_icp_terms.py is the same sum of absolute contributions
    by_label = {label: c for label, _, c in cases}
    for s in sc.all_scenes():
        unit = s.truth(EYE, ZERO)[1]
        np.testing.assert_allclose(by_label[("icp", s.name, 0)]["abs_terms"], unit, rtol=1e-12, atol=0)


def test_pnp_restatement_equals_autograd():
    cases = _restatement_equals_autograd("pnp")
    warm = [c for label, _, c in cases if label[-1] < pnp_host.WARM]
    gated = [c for label, _, c in cases if label[-1] >= pnp_host.WARM]
    assert warm and gated
    assert all(np.all(c["w"] == 1.0) for c in warm)
    assert any(np.any(c["w"] < 1.0) for c in gated) and all(np.any(c["w"] == 1.0) for c in gated)
    # the gate drops the displaced correspondences that the warm iterations still count
    assert all(g["count"] < w["count"] for g, w in zip(gated, warm[::2]))


def test_sil_restatement_equals_autograd():
    cases = _restatement_equals_autograd("sil")
    assert any(np.any(c["w"] < 1.0) and np.any(c["w"] == 1.0) for _, _, c in cases)


def test_photo_restatement_equals_autograd():
    cases = _restatement_equals_autograd("photo")
    # both pyramid levels, and on each a pair whose residuals reach the Huber branch: the weight is exercised
    for lvl in range(photo_host.GPU_LEVELS):
        at = [c for label, _, c in cases if label[-1] == lvl]
        assert at and any(np.any(c["w"] < 1.0) and np.any(c["w"] == 1.0) for c in at), lvl
    # the small window: fewer than 64 points at level 1 (no step there), enough at level 0
    small = {label[-1]: c["count"] for label, _, c in cases if label[1:6] == (0, True, 2, 2, 1)}     # levels = 2, iters = 1: lvl -> count
    assert small[1] < pr.MIN_POINTS <= small[0], small


def test_no_decision_is_borderline():
    for stage, cases in STAGES.items():
        least = {}
        for label, _, c in cases():
            for name, m in c["margins"].items():
                if stage == "photo" and name == "cell" and c["frozen"]["at_identity"]:
                    continue              # every template pixel sits on its own centre (also after a skipped step): see the docstring
                least[name] = min(least.get(name, (np.inf, None)), (m, label), key=lambda x: x[0])
                assert m >= MIN_MARGIN, (label, name, m)
        print("{}: least decision margins {}".format(stage, {k: "{:.3g} at {}".format(*v) for k, v in least.items()}))


# ------------------------------------------------------------------------------------------------------------------ planted defects
PIXEL_DEFECTS = ("fy_for_fx", "rotation_negated", "weight_on_A_only")
PHOTO_DEFECTS = ("no_s", "gpz_sign", "rotation_negated", "weight_on_A_only")


def private_pixel_terms(c, defect=None):
    """a private copy of the restated reprojection formula (Jx, Jy of flow_pnp_reference / sil_reference.normal_equations) on the
    frozen points of a gn_calculus result -> the 29 sums.  defect: one of PIXEL_DEFECTS, or "swap_edge": the residual against (ey, ex)"""
    f = c["frozen"]
    m, target, (fx, fy, cx, cy), w = f["m"], f["target"], f["cam"], c["w"]
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    tx, ty = (target[:, 1], target[:, 0]) if defect == "swap_edge" else (target[:, 0], target[:, 1])
    rx, ry = fx * mx / mz + cx - tx, fy * my / mz + cy - ty
    fxj = fy if defect == "fy_for_fx" else fx
    ax, bx, ay, by = fxj / mz, -fxj * mx / (mz * mz), fy / mz, -fy * my / (mz * mz)
    zero = np.zeros(len(m))
    Jx = np.stack([bx * my, ax * mz - bx * mx, -ax * my, ax, zero, bx], axis=1)
    Jy = np.stack([by * my - ay * mz, -by * mx, ay * mx, zero, ay, by], axis=1)
    if defect == "rotation_negated":
        Jx[:, :3], Jy[:, :3] = -Jx[:, :3], -Jy[:, :3]
    wg = np.ones(len(m)) if defect == "weight_on_A_only" else w
    A = (Jx * w[:, None]).T @ Jx + (Jy * w[:, None]).T @ Jy
    g = Jx.T @ (wg * rx) + Jy.T @ (wg * ry)
    return gc.pack(A, g, len(m), np.sum(rx * rx + ry * ry))


def private_photo_terms(c, defect=None):
    """a private copy of the restated photometric formula (photo_reference.normal_equations) on the frozen points of a gn_calculus
    result -> the 29 sums.  defect: one of PHOTO_DEFECTS"""
    f = c["frozen"]
    p, (fx, fy, cx, cy), s, w = f["m"], f["cam"], f["s"], c["w"]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    U, V = f["level_pixel"](p)
    ax, ay = U - f["xf"], V - f["yf"]
    i00, i01, i10, i11 = f["cell"]
    r = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11) - f["tv"]
    sg = 1.0 if defect == "no_s" else s
    gx = ((1.0 - ay) * (i01 - i00) + ay * (i11 - i10)) / sg
    gy = ((1.0 - ax) * (i10 - i00) + ax * (i11 - i01)) / sg
    gpz = -(gx * fx * px + gy * fy * py) / (pz * pz)
    gp = np.stack([gx * (fx / pz), gy * (fy / pz), -gpz if defect == "gpz_sign" else gpz], axis=1)
    rot = np.cross(p, gp)
    J = np.concatenate([-rot if defect == "rotation_negated" else rot, gp], axis=1)
    wg = np.ones(len(p)) if defect == "weight_on_A_only" else w
    return gc.pack((J * w[:, None]).T @ J, (J * wg[:, None]).T @ r, len(r), np.sum(w * r * r))


def test_planted_defects_are_over_the_bar():
    over = {}

    def plant(name, private, cases, defects):
        clean = max(float(ratio_to_bar(private(c), c).max()) for c in cases)
        assert clean <= 1.0, (name, clean)                      # the private copy itself is within the bar
        for d in defects:
            over[(name, d)] = max(float(ratio_to_bar(private(c, d), c).max()) for c in cases)

    gated = [c for label, _, c in pnp_cases() if label[-1] >= pnp_host.WARM]
    plant("pnp", private_pixel_terms, gated, PIXEL_DEFECTS)
    plant("sil", private_pixel_terms, [c for _, _, c in sil_cases() if c["count"] >= sr.MIN_POINTS], PIXEL_DEFECTS + ("swap_edge",))
    level1 = [c for label, _, c in photo_cases() if label[-1] == 1]
    level0 = [c for label, _, c in photo_cases() if label[-1] == 0]
    plant("photo level 1", private_photo_terms, level1, PHOTO_DEFECTS)
    plant("photo level 0", private_photo_terms, level0, PHOTO_DEFECTS[1:])
    # at level 0 s = 1: the dropped division is no defect there, which is why level 1 has to be pinned
    assert max(float(ratio_to_bar(private_photo_terms(c, "no_s"), c).max()) for c in level0) <= 1.0
    print("planted defect: worst term error / bar")
    for key, v in over.items():
        print("   {:14s} {:18s} {:.3g}".format(key[0], key[1], v))
        assert v >= 10.0, (key, v)
