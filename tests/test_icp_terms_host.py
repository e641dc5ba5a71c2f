"""CPU: the inputs and the bar of tests/test_gpu_icp_terms.py, fixed before the device is trusted with them.

The scenes (tests/icp_terms_scenes.py) are analytic depth maps.  For every scene and every iteration the GPU file reads, this file
asserts in float64 that no gate decision is borderline -- so the GPU file can demand EQUAL inlier counts -- and that the float32
model of tests/icp_reference.py (icp.hip operation by operation, per-lane float32 sums in grid-stride order) finds the same inliers.

The bar: the error of a sum is |S_k - S_k(float64)| / sum over the inliers of |contribution_k|, the float64 taken from the same
float32 inputs (depths, K, and R, t as the kernel casts them), so it measures arithmetic only.  The GPU file allows BAR_FACTOR x the
float32 model's worst error over the 27 matrix and vector terms, per scene and iteration.  test_planted_defects_are_over_the_bar
shows that six planted defects are over that bar on some term of some scene, that the seventh (the dropped normal flip) cannot show
in any sum at all, and lists the ones that the pose check of tests/test_gpu_icp.py (2e-5 rad, 2e-6 m, counts within 0.1 %, rms within
0.1 %, after one iteration) lets through on at least one scene."""
import numpy as np
import pytest

import icp_reference as ir
import icp_terms_scenes as sc
from test_split_terms import BAR_FACTOR

SCENES = {s.name: s for s in sc.all_scenes()}


def _check_margins(s, R, t, mask_margin=True):
    """-> float64 sums, unit, float32 model partials; asserts the margins at the correction (R, t)"""
    m = {}
    truth, unit = s.truth(R, t, margins=m)
    part, _ = s.partial(R, t, np.float32)
    where = (s.name, m)
    assert m["round_px"] >= 1e-2, where                  # u, v: the nearest rounding boundary, pixels
    assert m["jump"] >= 1e-2, where                      # neighbour depth jumps: distance from max_dist, in max_dist
    assert m["dist"] >= 1e-2, where                      # |p - q|: the same
    assert m["nn"] >= 1e-12, where                       # |a x b|^2 against 1e-20
    assert m["flip"] >= 1e-2, where                      # |n . q| (metres; q is about 1 m away) against 0
    assert not mask_margin or m.get("mask", 1.0) >= 1e-2, where   # mask values against 0.5
    assert part[:, 27].sum() == truth[27], where         # the float32 model finds the same inliers
    return truth, unit, part


@pytest.fixture(scope="module")
def chains():
    return {name: sc.model_chain(s) for name, s in SCENES.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_gate_decision_is_borderline(chains, name):
    s = SCENES[name]
    for k, (R, t) in enumerate(chains[name]):
        truth, unit, part = _check_margins(s, R, t)
        assert truth[27] >= ir.MIN_POINTS, (name, k)
        assert np.linalg.cond(ir.unpack_sums(truth)[0]) < 1e5, (name, k)
        assert np.all(sc.term_error(part.sum(axis=0), truth, unit) < 1e-2), (name, k)    # the model is a model of the same sums


def test_the_frames_take_every_lane_path():
    boxes = {s.name: (lambda b: (b[1] - b[0] + 1) * (b[3] - b[2] + 1))(ir.clamp_bbox(s.bbox, s.H, s.W)) for s in SCENES.values()}
    assert boxes["f12-cut"] < 256 < boxes["f24a-plain"] < ir.LANES                  # less than a workgroup; some workgroups idle
    assert ir.LANES < boxes["f72-plain"] < 2 * ir.LANES                              # some lanes take two points
    assert 2 * ir.LANES < boxes["f96-cut"] < boxes["f96-plain"] == 3 * ir.LANES       # three
    assert SCENES["f37-plain"].W % 2 == 1 or SCENES["f37-plain"].H % 2 == 1          # an odd stride


def test_points_leave_their_own_pixel(chains):
    """at the identity a source point projects onto its own pixel by construction; from the first update on, in at least two scenes,
    at least a third of them associate with another pixel"""
    moved = {}
    for name, s in SCENES.items():
        src = ir.source_points(s.dr, s.K, s.bbox)
        fx, fy, cx, cy = ir._camera(s.K)

        def pixel(p):
            return np.floor(fx * p[:, 0] / p[:, 2] + cx + 0.5), np.floor(fy * p[:, 1] / p[:, 2] + cy + 0.5)

        u0, v0 = pixel(src)
        share = []
        for R, t in chains[name]:
            u, v = pixel(ir.move_points(src, R, t))
            share.append(float(np.mean((u != u0) | (v != v0))))
        assert share[0] == 0.0
        moved[name] = min(share[1:])
    assert sum(m >= 1.0 / 3.0 for m in moved.values()) >= 2, moved


def test_mask_and_box_cut_something(chains):
    for b in sc.BASES:
        plain, cut = SCENES[b[0] + "-plain"], SCENES[b[0] + "-cut"]
        n_plain, n_cut, n_box = (s.truth(np.eye(3), np.zeros(3))[0][27] for s in (plain, cut, sc.Scene("", cut.K, cut.dr, cut.do, bbox=cut.bbox)))
        assert n_cut < n_box < n_plain, b[0]
        assert np.count_nonzero(cut.dr > 0) == cut.dr.size and np.any((cut.mask > 0) & (cut.mask < 1))
        # the distance gate removes the deep patch and nothing else does
        gated = ir.point_terms(ir.source_points(plain.dr, plain.K), plain.do, plain.K, sc.MAX_DIST, defect="rr_before_gate")[0]
        assert np.count_nonzero(gated[:, 27] == 0) >= 4, b[0]


# ------------------------------------------------------------------------------------------------------------------ the bar
def _old_pose_check_passes(S, truth):
    """the checks of test_hip_matches_restatement_mixed_K on one iteration from the identity"""
    Ra, ta, xa = ir.gn_step(np.eye(3), np.zeros(3), S)
    Rb, tb, xb = ir.gn_step(np.eye(3), np.zeros(3), truth)
    if xa is None or xb is None:
        return False
    M = Ra @ Rb.T
    sin = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    rms_a, rms_b = np.sqrt(S[28] / S[27]), np.sqrt(truth[28] / truth[27])
    return bool(np.arctan2(sin, (np.trace(M) - 1.0) / 2.0) <= 2e-5 and np.linalg.norm(ta - tb) <= 2e-6
                and abs(S[27] - truth[27]) <= 1e-3 * truth[27] and abs(rms_a - rms_b) <= 1e-3 * rms_b + 1e-7)


# the defects that the old pose check lets through on at least one scene (the others it catches on every scene here): the border gate
# wherever the box keeps column W - 1 out.  (The dropped normal flip passes every check there is: see below.)
PASSES_OLD_POSE_CHECK = {"border_u"}


def test_planted_defects_are_over_the_bar(chains):
    names = sorted(SCENES)
    over = {d: 0.0 for d in ir.DEFECTS + ("mask_pair0",) if d != "no_flip"}
    passes_old = set()
    for name in names:
        s = SCENES[name]
        for k, (R, t) in enumerate(chains[name]):
            truth, unit = s.truth(R, t)
            part, _ = s.partial(R, t, np.float32)
            bar = BAR_FACTOR * sc.term_error(part.sum(axis=0), truth, unit)[:27].max()
            assert bar > 0
            planted = {d: s.partial(R, t, np.float32, defect=d)[0].sum(axis=0) for d in ir.DEFECTS}
            if s.mask is not None and name[:-4] in sc.BATCH[1:]:   # pair 1, 2 of the batch read the mask plane of pair 0
                planted["mask_pair0"] = s.partial(R, t, np.float32, mask=SCENES[sc.BATCH[0] + "-cut"].mask)[0].sum(axis=0)
            # the flip cannot show in any sum: J and r are both odd in n, every term is a product of two of them
            assert np.array_equal(planted.pop("no_flip"), part.sum(axis=0)), (name, k)
            for d, S in planted.items():
                err = sc.term_error(S, truth, unit)
                over[d] = max(over[d], float(np.delete(err, 27).max() / bar))
                if k == 0 and _old_pose_check_passes(S, truth):
                    passes_old.add(d)
    print("planted defect: worst term error / bar (best scene):", {d: "%.3g" % v for d, v in over.items()})
    print("planted defects that pass the old pose check on some scene:", sorted(passes_old))
    for d, v in over.items():
        assert v > 1.0, (d, v)
    assert passes_old == PASSES_OLD_POSE_CHECK


# ------------------------------------------------------------------------------------------------------------------ special scenes
def _count(s, R=np.eye(3), t=np.zeros(3)):
    return int(s.truth(R, t)[0][27])


def test_gate_variants_have_the_expected_inliers():
    for s, n in sc.gate_variants():
        with np.errstate(invalid="ignore"):
            # the mask values 0.49 and 0.5 are inputs compared with a constant: no arithmetic can move them
            _check_margins(s, np.eye(3), np.zeros(3), mask_margin=False)
            assert _count(s) == n, s.name
    assert _count(sc.tiny_frame()) == 1


def test_boxes():
    for name, box in sc.BOXES.items():
        s = sc.box_scene(name)
        if name == "inverted":
            assert _count(s) == 0
            continue
        _check_margins(s, np.eye(3), np.zeros(3))
        x0, x1, y0, y1 = ir.clamp_bbox(s.bbox, s.H, s.W)
        assert 0 < _count(s) <= (x1 - x0 + 1) * (y1 - y0 + 1) < s.H * s.W, name
    assert _count(sc.box_scene("one-row")) < ir.MIN_POINTS


def test_threshold_pair():
    s64, s63 = sc.threshold_pair()
    for s, n in ((s64, 64), (s63, 63)):
        truth, _, part = _check_margins(s, np.eye(3), np.zeros(3))
        assert truth[27] == n == ir.MIN_POINTS - (s is s63)
        assert (ir.gn_step(np.eye(3), np.zeros(3), part.sum(axis=0))[2] is not None) == (n == 64)


def test_update_then_skip():
    s = sc.update_then_skip()
    _, _, part = _check_margins(s, np.eye(3), np.zeros(3))
    assert part[:, 27].sum() >= ir.MIN_POINTS
    R, t, xi = ir.gn_step(np.eye(3), np.zeros(3), part.sum(axis=0))
    assert xi is not None
    truth, _, _ = _check_margins(s, R, t)
    assert truth[27] < ir.MIN_POINTS


def test_zero_residual_is_exact_in_float32():
    s = sc.zero_residual()
    part, terms = s.partial(np.eye(3), np.zeros(3), np.float32)
    assert part[:, 27].sum() >= ir.MIN_POINTS and np.all(terms[:, 21:27] == 0) and np.all(terms[:, 28] == 0)
    R, t, xi = ir.gn_step(np.eye(3), np.zeros(3), part.sum(axis=0))
    assert np.all(xi == 0) and np.array_equal(R, np.eye(3)) and np.all(t == 0)


def test_camera_rule():
    K = sc.camera(24, 32, 40.0)
    assert ir.camera_ok(K)
    for (i, j), bad in (((0, 0), 0.0), ((0, 0), -3.0), ((1, 1), np.nan), ((0, 2), np.inf), ((1, 2), -np.inf), ((1, 1), 0.0)):
        Kb = K.copy()
        Kb[i, j] = bad
        assert not ir.camera_ok(Kb)
        assert len(ir.source_points(np.ones((24, 32), np.float32), Kb)) == 0
    Kb = K.copy()
    Kb[2, 2], Kb[0, 1] = np.nan, np.inf      # entries the kernel never reads
    assert ir.camera_ok(Kb)


def test_point_terms_sum_to_the_normal_equations():
    s = SCENES["f37-cut"]
    p = ir.move_points(ir.source_points(s.dr, s.K, s.bbox), ir.rodrigues([0.01, -0.02, 0.015]), [0.002, -0.001, 0.003])
    terms, idx = ir.point_terms(p, s.do, s.K, sc.MAX_DIST, s.mask)
    A, g, N, rr = ir.normal_equations(p, s.do, s.K, sc.MAX_DIST, s.mask)
    assert N == len(terms) == len(idx) and len(np.unique(idx)) == N
    A0, g0, N0, rr0 = _matrix_form(p, s.do, s.K, sc.MAX_DIST, s.mask)
    assert N == N0 and np.array_equal(A, A.T) and np.all(terms[:, 27] == 1)
    np.testing.assert_allclose(A, A0, rtol=1e-12, atol=1e-14 * N)
    np.testing.assert_allclose(g, g0, rtol=1e-12, atol=1e-14 * N)
    np.testing.assert_allclose(rr, rr0, rtol=1e-12)


def _matrix_form(p, depth_observed, K, max_dist, mask_observed=None):
    """the normal equations as matrix products over whole points (what normal_equations was before it was built on point_terms)"""
    H, W = depth_observed.shape
    fx, fy, cx, cy = ir._camera(K)
    D = np.asarray(depth_observed, np.float64)

    def back(u, v):
        z = D[v, u]
        return np.stack([z * (u - cx) / fx, z * (v - cy) / fy, z], axis=1), z

    p = p[p[:, 2] > 0]
    u = np.floor(fx * p[:, 0] / p[:, 2] + cx + 0.5)
    v = np.floor(fy * p[:, 1] / p[:, 2] + cy + 0.5)
    ok = (u >= 1) & (u <= W - 2) & (v >= 1) & (v <= H - 2)
    p, u, v = p[ok], u[ok].astype(np.int64), v[ok].astype(np.int64)
    ok = D[v, u] > 0
    if mask_observed is not None:
        ok &= np.asarray(mask_observed, np.float64)[v, u] >= 0.5
    p, u, v = p[ok], u[ok], v[ok]
    q, zq = back(u, v)
    nb = []
    ok = np.ones(len(p), bool)
    for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        qn, zn = back(u + du, v + dv)
        ok &= (zn > 0) & (np.abs(zn - zq) < max_dist)
        nb.append(qn)
    n = np.cross(nb[0] - nb[1], nb[2] - nb[3])
    nn = np.sum(n * n, axis=1)
    ok &= nn > 1e-20
    p, q, n, nn = p[ok], q[ok], n[ok], nn[ok]
    n = n / np.sqrt(nn)[:, None]
    n = np.where((np.sum(n * q, axis=1) > 0)[:, None], -n, n)
    e = p - q
    ok = np.sum(e * e, axis=1) <= max_dist * max_dist
    p, n, e = p[ok], n[ok], e[ok]
    r = np.sum(n * e, axis=1)
    J = np.concatenate([np.cross(p, n), n], axis=1)
    return J.T @ J, J.T @ r, int(len(r)), float(np.sum(r * r))
