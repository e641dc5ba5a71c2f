"""The accumulate kernels of flow PnP, the silhouette polish and the photometric polish (csrc/flow_pnp.hip, sil.hip, photo.hip) term by
term against calculus: the 29 sums the device leaves in its workspace (tests/gn_terms_io.py: how they are read, with no library change)
against tests/gn_calculus.py, float64 autograd of each stage's residual, at the device's own corrections T_k.

For iters = 1, 2, 3 the block-order sum of run k + 1's partials is compared with gn_calculus at T_k (T_0 = I, T_k = the state of run
k read as float64): the count EQUAL, every other term within 64 eps64 x abs_terms -- these kernels are float64 per point; the lane
loop, the block_sum tree and the 16 partials add up to about 25 roundings -- the stats rows bit-equal to what the device's sums give,
every partial finite, the NaN-filled guard arena around the workspace intact.  tests/test_gn_calculus_host.py shows on the CPU that
the restatements meet the same bar on the same frames, that no decision of theirs is borderline, and that planted slips of the
derivation are 1e11 x over it; the margins are asserted again here at the device's corrections.  ICP is not repeated: its per-lane
float32 sums have their own bar in tests/test_gpu_icp_terms.py, whose `truth` the host file ties to autograd.

Photo's coarse level can never be read directly (every call ends at level 0), so it is pinned through one solve: levels = 2, iters = 1
leaves the level-0 sums at T_1 and the state T_2; the step xi_2 recovered from those sums (the algebra of icp_reference.gn_step, taken
in the kernel's own operation order by gn_terms_io.step_in_kernel_order so that it can be undone to the last bits) is undone, and the
device's T_1 must equal gn_step(I, autograd's level-1 sums) within the solve tolerance of tests/test_gpu_icp_terms.py,
1e3 eps64 cond(A) (|xi| + max|.|).  Where that tolerance exceeds 1e-6 the check would be vacuous; the test prints it and fails
rather than pass silently."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gn_calculus as gc  # noqa: E402
import guard_arena  # noqa: E402
import icp_reference as ir  # noqa: E402
import photo_reference as pr  # noqa: E402
import sil_reference as sr  # noqa: E402
import test_flow_pnp_host as pnp_host  # noqa: E402
import test_photo_host as photo_host  # noqa: E402
import test_sil_host as sil_host  # noqa: E402
from gn_terms_io import N_TERMS, bits, block_order_sum, split_workspace, state_of, stats_of  # noqa: E402
from gn_terms_io import step_in_kernel_order, undo_step_exactly  # noqa: E402
from test_gn_calculus_host import MIN_MARGIN, ratio_to_bar  # noqa: E402

DEV = "cuda:0"
EPS64 = float(np.finfo(np.float64).eps)
EYE, ZERO = np.eye(3), np.zeros(3)


def ops():
    from lib.hip import ops as o

    return o


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def _outputs(B, rows):
    return (torch.full((B, rows, 2), float("nan"), dtype=torch.float32, device=DEV), torch.zeros((B,), dtype=torch.int32, device=DEV))


def _read(work, B, stats, status, what):
    work.check(what)
    state, partial = split_workspace(work.view().cpu().numpy(), B)
    return dict(stats=stats.cpu().numpy(), status=status.cpu().numpy(), state=state, partial=partial)


def _check_margins(c, what, cell_exempt=False):
    for name, m in c["margins"].items():
        if not (cell_exempt and name == "cell"):     # photo's cell at T = I: tests/test_gn_calculus_host.py says why
            assert m >= MIN_MARGIN, (what, name, m)


def _terms_within_bar(c, partial, what, worst):
    """the device's partials of one pair against autograd at the same correction -> S, the block-order sums"""
    assert np.all(np.isfinite(partial[:, :N_TERMS])), what
    S = block_order_sum(partial)
    assert S[27] == c["count"], (what, S[27], c["count"])
    ratio = ratio_to_bar(S, c)
    print("{}: N = {:.0f}, device against autograd: worst term error / bar {:.3g} (term {})".format(what, S[27], ratio.max(), int(np.argmax(ratio))))
    worst.append(float(ratio.max()))
    assert ratio.max() <= 1.0, (what, int(np.argmax(ratio)), float(ratio.max()))
    return S


def _chain(runs, B, calc, what, cell_exempt_at_identity=False):
    """runs: the calls with iters = 1, 2, 3; calc(b, R, t, k) -> gn_calculus at the correction (R, t) of iteration k"""
    worst = []
    for b in range(B):
        R, t = EYE, ZERO
        for k, run in enumerate(runs):
            c = calc(b, R, t, k)
            at_identity = np.array_equal(R, EYE) and not np.any(t)
            _check_margins(c, (what, b, k), cell_exempt_at_identity and at_identity)
            S = _terms_within_bar(c, run["partial"][b], (what, b, k), worst)
            for later in runs[k:]:      # row k of every run that has it: bit for bit what the device's own sums give
                assert np.array_equal(bits(later["stats"][b, k]), bits(stats_of(S))), (what, b, k, later["stats"][b], stats_of(S))
            moved = S[27] >= ir.MIN_POINTS
            Rn, tn, updated = state_of(run, b)
            if not moved:               # a skipped step leaves the correction
                assert np.array_equal(Rn, R) and np.array_equal(tn, t), (what, b, k)
            else:
                assert updated == 1.0 and not np.array_equal(tn, t), (what, b, k)
            R, t = Rn, tn
    print("{}: worst term error / bar over {} linearisations: {:.3g}".format(what, len(worst), max(worst)))


# ------------------------------------------------------------------------------------------------------------------ flow PnP
@functools.lru_cache(maxsize=None)
def _pnp_batches():
    return [b for b in pnp_host.gpu_batches() if not b[4]]      # (dy, dx) flow: the 48x64 batch of three and the 37x50 batch of two


def _run_pnp(batch, iters, with_bbox):
    name, H, W, cases, rep = batch
    B = len(cases)
    stats, status = _outputs(B, iters)
    work = guard_arena.workspace(ops().lib().dim_flow_pnp_workspace_bytes(B, H, W), 8, DEV)
    Ks = np.stack([c["K"] for c in cases]).reshape(B, 9)
    ops().flow_pnp(_dev(np.stack([c["depth"] for c in cases])[:, None]), _dev(np.stack([c["flow"] for c in cases])),
                   _dev(np.stack([c["pose_src"] for c in cases])), Ks[0].reshape(3, 3), iters, pnp_host.WARM, pnp_host.HUBER, pnp_host.GATE,
                   standard_rep=rep, valid=_dev(np.stack([c["visible"] for c in cases])[:, None]),
                   bbox=_dev(np.stack([c["bbox"] for c in cases]), torch.int32) if with_bbox else None, K_per_sample=_dev(Ks), stats=stats,
                   status=status, workspace=work.view())
    return _read(work, B, stats, status, "dim_flow_pnp workspace, {}".format(name))


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("which", [0, 1])
def test_flow_pnp_terms(hip_lib, which, with_bbox):
    """warm = 2: iterations 0 and 1 take every point with w = 1, iteration 2 is gated and Huber-weighted"""
    batch = _pnp_batches()[which]
    name, H, W, cases, rep = batch
    assert not np.array_equal(cases[0]["K"], cases[1]["K"])

    def calc(b, R, t, k):
        c = cases[b]
        return gc.flow_pnp(c["depth"], c["flow"], c["K"], R, t, k >= pnp_host.WARM, pnp_host.HUBER, pnp_host.GATE, rep, c["visible"],
                           c["bbox"] if with_bbox else None)

    _chain([_run_pnp(batch, n, with_bbox) for n in (1, 2, 3)], len(cases), calc, "pnp {} bbox={}".format(name, with_bbox))


# ------------------------------------------------------------------------------------------------------------------ silhouette
def _run_sil(g, iters, with_bbox):
    B = len(g["pose_in"])
    stats, status = _outputs(B, iters)
    work = guard_arena.workspace(ops().lib().dim_sil_workspace_bytes(B, g["H"], g["W"]), 8, DEV)
    ops().sil_refine(_dev(g["depth_rendered"]), _dev(g["field"], torch.int32), _dev(g["pose_in"]), g["K"], iters, sil_host.HUBER, sil_host.GATE,
                     bbox=_dev(g["bbox"], torch.int32) if with_bbox else None, K_per_sample=_dev(g["K_per_sample"]), stats=stats, status=status,
                     workspace=work.view())
    return _read(work, B, stats, status, "dim_sil_refine workspace, {} x {}".format(g["H"], g["W"]))


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("which", [0, 1])
def test_sil_terms(hip_lib, which, with_bbox):
    """the field is the restatement's (tests/test_gpu_sil.py shows the device builds the same one)"""
    g = sil_host.gpu_batches()[which]

    def calc(b, R, t, k):
        return gc.sil(g["depth_rendered"][b, 0], g["field"][b], g["K_per_sample"][b], R, t, sil_host.HUBER, sil_host.GATE,
                      g["bbox"][b] if with_bbox else None)

    runs = [_run_sil(g, n, with_bbox) for n in (1, 2, 3)]
    _chain(runs, len(g["pose_in"]), calc, "sil {}x{} bbox={}".format(g["H"], g["W"], with_bbox))
    if which == 0 and with_bbox:        # the left third of pair 2's render: fewer than 64 contour points, never a step
        assert runs[2]["status"].tolist() == [0, 0, sr.STATUS_SIL_FEW_POINTS] and runs[2]["state"][2, 12] == 0.0


# ------------------------------------------------------------------------------------------------------------------ photo
def _run_photo(g, levels, iters, with_bbox):
    """-> the run, and per pair what the device itself built for the accumulate kernel: the planes of every level and (a, b)"""
    B, H, W = len(g["pose_in"]), g["H"], g["W"]
    stats, status = _outputs(B, levels * iters)
    work = guard_arena.workspace(ops().lib().dim_photo_workspace_bytes(B, H, W, levels), 16, DEV)
    ops().photo_refine(_dev(g["image_observed"]), _dev(g["image_rendered"]), _dev(g["depth_rendered"]), _dev(g["pose_in"]), g["K"], levels, iters,
                       photo_host.HUBER, photo_host.GATE, bbox=_dev(g["bbox"], torch.int32) if with_bbox else None,
                       K_per_sample=_dev(g["K_per_sample"]), stats=stats, status=status, workspace=work.view())
    run = _read(work, B, stats, status, "dim_photo_refine workspace, {} x {}, {} levels".format(H, W, levels))
    planes, gains = ops().photo_workspace_views(work.view(), B, H, W, levels)
    planes = {k: [p.cpu().numpy() for p in v] for k, v in planes.items()}
    run["gain"] = gains.cpu().numpy()
    run["planes"] = [{"obs": [p[b] for p in planes["obs"]], "ren": [p[b] for p in planes["ren"]], "depth": [p[b] for p in planes["depth"]],
                      "valid": [p[b] > 0.5 for p in planes["valid"]]} for b in range(B)]
    return run


def _photo_calc(g, run, lvl):
    def calc(b, R, t, k):
        a, bias, ok = run["gain"][b, 5:8]
        assert ok == 1.0
        return gc.photo(run["planes"][b], lvl, g["K_per_sample"][b], R, t, float(a), float(bias), photo_host.HUBER, photo_host.GATE)

    return calc


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("which", [0, 1])
def test_photo_terms_level_0(hip_lib, which, with_bbox):
    """levels = 1: the planes and the gain row are the device's own (tests/test_gpu_photo.py pins them against the restatement)"""
    g = photo_host.gpu_batches()[which]
    runs = [_run_photo(g, 1, n, with_bbox) for n in (1, 2, 3)]
    for later in runs[1:]:
        assert np.array_equal(bits(later["gain"]), bits(runs[0]["gain"]))
    _chain(runs, len(g["pose_in"]), _photo_calc(g, runs[0], 0), "photo {}x{} bbox={}".format(g["H"], g["W"], with_bbox),
           cell_exempt_at_identity=True)


@functools.lru_cache(maxsize=None)
def _coarse(which, with_bbox):
    """one call with levels = 2, iters = 1 -> the run and, per pair, the device's T_1 recovered from it: its state T_2 with the step
    of its own level-0 sums undone, R_1 = dR^-1 R_2, t_1 = dR^-1 (t_2 - v)"""
    g = photo_host.gpu_batches()[which]
    run = _run_photo(g, 2, 1, with_bbox)
    pairs = []
    for b in range(len(g["pose_in"])):
        S0 = block_order_sum(run["partial"][b])
        R2, t2, _ = state_of(run, b)
        step = step_in_kernel_order(S0)
        assert step is not None, (which, with_bbox, b)       # level 0 steps on every pair
        dR, v, xi2 = step
        R1, t1 = undo_step_exactly(dR, v, R2, t2)
        # how much of the state the recovered T_1 gives back, bit for bit, under the kernel's own product (Rw R, Rw t + v, left to right)
        Rr = np.array([[dR[i, 0] * R1[0, j] + dR[i, 1] * R1[1, j] + dR[i, 2] * R1[2, j] for j in range(3)] for i in range(3)])
        tr = np.array([dR[i, 0] * t1[0] + dR[i, 1] * t1[1] + dR[i, 2] * t1[2] + v[i] for i in range(3)])
        replayed = int(np.sum(bits(Rr) == bits(R2))) + int(np.sum(bits(tr) == bits(t2)))
        pairs.append(dict(S0=S0, R2=R2, t2=t2, dR=dR, v=v, xi2=xi2, R1=R1, t1=t1, replayed=replayed,
                          small=which == 0 and with_bbox and b == 2))     # 54 template pixels at level 1: counted, flagged, no step
    return g, run, pairs


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("which", [0, 1])
def test_photo_coarse_level_through_one_solve(hip_lib, which, with_bbox):
    g, run, pairs = _coarse(which, with_bbox)
    calc1, calc0 = _photo_calc(g, run, 1), _photo_calc(g, run, 0)
    for b, p in enumerate(pairs):
        what = ("photo coarse {}x{} bbox={}".format(g["H"], g["W"], with_bbox), b)
        # one step from the identity on autograd's level-1 sums
        c1 = calc1(b, EYE, ZERO, 0)
        _check_margins(c1, what, cell_exempt=True)
        assert run["stats"][b, 0, 0] == c1["count"], (what, run["stats"][b, 0], c1["count"])
        assert (c1["count"] < ir.MIN_POINTS) == p["small"], (what, c1["count"])
        # the rms of the level-1 row, a float32 of the device's level-1 sums, against autograd's: one float32 ulp
        want = np.sqrt(c1["s28"] / c1["count"])
        assert abs(run["stats"][b, 0, 1] - want) <= 2.0 ** -23 * want, (what, run["stats"][b, 0, 1], want)
        Ra, ta, xi1 = ir.gn_step(EYE, ZERO, c1["terms"])
        if p["small"]:
            # the step is skipped, T_1 = I exactly: the state is one level-0 step from the identity (the solve check of
            # tests/test_gpu_icp_terms.py), and the level-0 sums are compared at the identity
            assert xi1 is None and run["status"][b] == pr.STATUS_PHOTO_FEW_POINTS
            tol0 = 1e3 * EPS64 * np.linalg.cond(ir.unpack_sums(p["S0"])[0])
            assert np.abs(p["R2"] - p["dR"]).max() <= tol0 * (np.linalg.norm(p["xi2"]) + np.abs(p["dR"]).max()), what
            assert np.abs(p["t2"] - p["v"]).max() <= tol0 * (np.linalg.norm(p["xi2"]) + np.abs(p["v"]).max()), what
            c0 = calc0(b, EYE, ZERO, 1)
            _check_margins(c0, what, cell_exempt=True)
            _terms_within_bar(c0, run["partial"][b], what + ("level 0 at the identity",), [])
        else:
            assert run["status"][b] == 0
            cond = np.linalg.cond(c1["A"])
            tol = 1e3 * EPS64 * cond
            tol_R, tol_t = tol * (np.linalg.norm(xi1) + np.abs(Ra).max()), tol * (np.linalg.norm(xi1) + np.abs(ta).max())
            vacuous = max(tol_R, tol_t) > 1e-6
            print("{}: level 1 N = {}, cond(A) {:.3g}, |dR| {:.3g} (tolerance {:.3g}), |dt| {:.3g} (tolerance {:.3g}){}".format(
                what, c1["count"], cond, np.abs(p["R1"] - Ra).max(), tol_R, np.abs(p["t1"] - ta).max(), tol_t,
                " -- VACUOUS: the tolerance is above 1e-6" if vacuous else ""))
            assert not vacuous, (what, cond, tol_R, tol_t)
            assert np.abs(p["R1"] - Ra).max() <= tol_R and np.abs(p["t1"] - ta).max() <= tol_t, what
        assert np.array_equal(bits(run["stats"][b, 1]), bits(stats_of(p["S0"]))), what


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("which", [0, 1])
def test_photo_level_0_sums_after_the_coarse_step(hip_lib, which, with_bbox):
    """The level-0 sums of the two-level call against autograd at the recovered T_1, with the per-term bar of this file.

    g moves with the linearisation point by A dxi, and |A| dxi with dxi = 4 eps in every component of the twist is 63 to 90 bars of
    g on these pairs (printed below): T_1 has to be recovered to a small fraction of an eps.  Hence _coarse takes the level-0 step
    with the kernel's own operations in the kernel's own order (gn_terms_io.step_in_kernel_order) and undoes it in rational
    arithmetic, rounded once (undo_step_exactly).  What remains is the kernel's own rounding of T_2 = fl(dR T_1), which nothing can
    undo.  Measured on the MI355X, worst term error / bar per pair: 48x64 0.35, 0.40 and (without boxes) 0.17; 37x50 with boxes
    0.41, 0.44, without 0.33, 0.86; every worst term in g (25, 26) or term 28.  With icp_reference.gn_step (numpy's dot products:
    another association, xi off by cond(A) eps) and a float64 undo by the transpose the same pairs gave 0.43 .. 1.91, over the bar
    on three of them, while the kernel at corrections read exactly from the state stays <= 0.21 (test_photo_terms_level_0)."""
    g, run, pairs = _coarse(which, with_bbox)
    calc0 = _photo_calc(g, run, 0)
    worst = []
    for b, p in enumerate(pairs):
        if p["small"]:
            continue            # compared at the identity, exactly, in test_photo_coarse_level_through_one_solve
        what = ("photo level 0 after the coarse step {}x{} bbox={}".format(g["H"], g["W"], with_bbox), b)
        c0 = calc0(b, p["R1"], p["t1"], 1)
        _check_margins(c0, what)
        moves = (np.abs(c0["A"]) @ np.full(6, 4 * EPS64)) / (gc.BAR * c0["abs_terms"][21:27])
        print("{}: 4 eps in T_1 move g by up to {:.3g} of its bar; the recovered T_1 replays {} of the 12 entries of T_2 bit for bit".format(
            what, moves.max(), p["replayed"]))
        _terms_within_bar(c0, run["partial"][b], what, worst)
    print("photo level 0 after the coarse step: worst term error / bar {:.3g}".format(max(worst)))
