"""The depth ICP kernels term by term (csrc/icp.hip icp_accumulate_kernel, csrc/twist_solve.h gn_solve_kernel) on small analytic frames.

How the terms are read, with no library change: the stage's workspace is [state B x 16 doubles = R, t, updated, pad][partial B x 16
workgroups x 32 doubles, terms 0..28].  After a call with iters = n the partials hold the sums of iteration n - 1, taken at the
correction T_{n-1}, and the state holds T_n; replays are bit-identical, so the runs with iters = 1, 2, 3 give T_k (state of run k) and
the 29 sums at T_k (partials of run k + 1).  The accumulate kernel is compared at a known T_k with tests/icp_reference.py (float64 on
the same float32 inputs; bar: BAR_FACTOR x the worst term error of the float32 model, tests/test_icp_terms_host.py), the solve kernel
from the device's own sums.  The inlier counts must be EQUAL: the host file shows that no gate decision of these scenes is borderline.
The workspace is a guard arena full of NaN bits at the minimum alignment; the pad doubles may keep their fill and are not read."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import icp_reference as ir  # noqa: E402
import icp_terms_scenes as sc  # noqa: E402
from gn_terms_io import bits as _bits, block_order_sum as _block_order_sum, split_workspace  # noqa: E402
from gn_terms_io import state_of as _state, stats_of as _stats_of  # noqa: E402
from test_split_terms import BAR_FACTOR  # noqa: E402

DEV = "cuda:0"
EPS64 = float(np.finfo(np.float64).eps)
SCENES = {s.name: s for s in sc.all_scenes()}


def _run(hip_lib, scenes, iters, use_mask=None, use_bbox=None, per_pair_K=None):
    """one dim_icp_refine call on a batch of scenes of one frame size.  The three switches default to what the first scene carries.
    -> dict: pose (B,3,4), stats (B,iters,2), status (B,), state (B,16) and partial (B,16,32) float64 as the call left them"""
    from lib.hip import ops

    B, s0 = len(scenes), scenes[0]
    H, W = s0.H, s0.W
    use_mask = s0.mask is not None if use_mask is None else use_mask
    use_bbox = s0.bbox is not None if use_bbox is None else use_bbox
    per_pair_K = s0.per_pair_K if per_pair_K is None else per_pair_K

    def dev(a, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)

    dr = dev(np.stack([s.dr for s in scenes])[:, None])
    do = dev(np.stack([s.do for s in scenes])[:, None])
    mask = dev(np.stack([s.mask for s in scenes])[:, None]) if use_mask else None
    bbox = dev(np.stack([s.bbox for s in scenes]), torch.int32) if use_bbox else None
    # with K per pair the host K is another camera: nothing may read it
    Kp = dev(np.stack([s.K for s in scenes]).reshape(B, 9)) if per_pair_K else None
    K_host = s0.K * np.float32(1.7) if per_pair_K else s0.K
    pose_in = np.stack([s.pose_in for s in scenes])
    stats = torch.full((B, max(iters, 1), 2), float("nan"), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    work = guard_arena.workspace(hip_lib.dim_icp_workspace_bytes(B, H, W), 8, DEV)
    out = ops.icp_refine(dr, do, dev(pose_in), K_host, iters, sc.MAX_DIST, mask_observed=mask, bbox=bbox, K_per_sample=Kp, stats=stats,
                         status=status, workspace=work.view())
    work.check("dim_icp_refine workspace, {} x {}, B = {}".format(H, W, B))
    ws = work.view().cpu().numpy().copy()
    state, partial = split_workspace(ws, B)
    return dict(pose=out.cpu().numpy(), stats=stats.cpu().numpy(), status=status.cpu().numpy(), state=state, partial=partial)


def _terms_within_bar(s, R, t, partial, what):
    """the device's partials of one pair at the correction (R, t) against the reference: counts equal (per workgroup too), every
    other sum within the bar -> S (block-order sum), ratio of the device's worst term error to the float32 model's"""
    truth, unit = s.truth(R, t)
    model, _ = s.partial(R, t, np.float32)
    S = _block_order_sum(partial)
    assert S[27] == truth[27], (what, S[27], truth[27])
    np.testing.assert_array_equal(partial[:, 27], model[:, 27], err_msg=str(what))        # which lane takes which point
    worst_model = sc.term_error(model.sum(axis=0), truth, unit)[:27].max()
    err = np.delete(sc.term_error(S, truth, unit), 27)
    print("{}: N = {:.0f}, device worst term error {:.3g}, model {:.3g}, ratio {:.3g}".format(what, S[27], err.max(), worst_model,
                                                                                             err.max() / worst_model if worst_model else np.nan))
    assert np.all(np.isfinite(partial[:, :ir.N_TERMS]))
    assert err.max() <= BAR_FACTOR * worst_model, (what, int(np.argmax(err)), err.max(), worst_model)
    return S, err.max() / worst_model if worst_model else 0.0


# ------------------------------------------------------------------------------------------------------------------ terms and solve
@pytest.mark.parametrize("name", sorted(SCENES))
def test_terms_and_solve(hip_lib, name):
    s = SCENES[name]
    runs = [_run(hip_lib, [s], n) for n in (1, 2, 3)]
    R, t = np.eye(3), np.zeros(3)
    for k in range(3):
        run = runs[k]
        S, _ = _terms_within_bar(s, R, t, run["partial"][0], (name, k))
        # stats (B, iters, 2): row k of every run that has it, bit for bit what the block-order sums give after the float32 cast
        for later in runs[k:]:
            assert np.array_equal(_bits(later["stats"][0, k]), _bits(_stats_of(S))), (name, k, later["stats"][0], _stats_of(S))
        # the solve, from the device's own sums
        R1, t1, xi = ir.gn_step(R, t, S)
        assert xi is not None and run["status"][0] == 0
        Rd, td, updated = _state(run)
        tol = 1e3 * EPS64 * np.linalg.cond(ir.unpack_sums(S)[0])
        print("{} k={}: solve |dR| {:.3g} |dt| {:.3g}, tolerance {:.3g} (|xi| {:.3g})".format(
            name, k, np.abs(Rd - R1).max(), np.abs(td - t1).max(), tol * (np.linalg.norm(xi) + 1.0), np.linalg.norm(xi)))
        assert updated == 1.0
        assert np.abs(Rd - R1).max() <= tol * (np.linalg.norm(xi) + np.abs(R1).max()), (name, k)
        assert np.abs(td - t1).max() <= tol * (np.linalg.norm(xi) + np.abs(t1).max()), (name, k)
        R, t = Rd, td
    # pose_out = float32(T_3 pose_in) from the device's state, within one float32 ulp per entry
    T0 = s.pose_in.astype(np.float64)
    want = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + t)[:, None]], axis=1)
    got = runs[2]["pose"][0]
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))), (name, got, want)
    assert np.abs(got - s.pose_in).max() > 1e-4      # a general pose_in, and the ICP moved it


@pytest.mark.parametrize("name", ["f24a", "f72"])
def test_each_argument_alone(hip_lib, name):
    """mask_observed, bbox and K_per_sample one at a time (the scenes above switch them together)"""
    cut = SCENES[name + "-cut"]
    for what, kw in (("mask", dict(use_mask=True, use_bbox=False, per_pair_K=False)), ("bbox", dict(use_mask=False, use_bbox=True, per_pair_K=False)),
                     ("K", dict(use_mask=False, use_bbox=False, per_pair_K=True))):
        ref = sc.Scene(cut.name, cut.K, cut.dr, cut.do, mask=cut.mask if kw["use_mask"] else None, bbox=cut.bbox if kw["use_bbox"] else None)
        run = _run(hip_lib, [cut], 1, **kw)
        _terms_within_bar(ref, np.eye(3), np.zeros(3), run["partial"][0], (name, what))


# ------------------------------------------------------------------------------------------------------------------ gates
def test_hand_built_gates(hip_lib):
    variants = sc.gate_variants()
    for i in range(0, len(variants), 4):
        chunk = variants[i:i + 4]
        scenes = [s for s, _ in chunk]
        for s in scenes:   # a mixed chunk: the pairs without a mask get ones
            s.mask = np.ones((s.H, s.W), np.float32) if s.mask is None and any(o.mask is not None for o in scenes) else s.mask
        run = _run(hip_lib, scenes, 1)
        for b, (s, n) in enumerate(chunk):
            with np.errstate(invalid="ignore"):
                truth, unit = s.truth(np.eye(3), np.zeros(3))
                S = _block_order_sum(run["partial"][b])
                assert S[27] == truth[27] == n, (s.name, S[27], truth[27], n)
                if n > 1:     # a whole frame of points: the sums pin WHICH ones (a point is 1/48 of a unit, the bar 1e-6 of it)
                    _terms_within_bar(s, np.eye(3), np.zeros(3), run["partial"][b], s.name)
            assert run["status"][b] == ir.STATUS_ICP_FEW_POINTS and run["state"][b, 12] == 0.0
            assert np.array_equal(_bits(run["pose"][b]), _bits(s.pose_in)), s.name
            assert run["stats"][b, 0].tolist() == [n, float(_stats_of(S)[1])], s.name


def test_3x3_frame(hip_lib):
    s = sc.tiny_frame()
    run = _run(hip_lib, [s], 2)
    S = _block_order_sum(run["partial"][0])
    assert S[27] == 1 == s.truth(np.eye(3), np.zeros(3))[0][27]
    assert run["status"][0] == ir.STATUS_ICP_FEW_POINTS and run["stats"][0, :, 0].tolist() == [1, 1]
    assert np.array_equal(_bits(run["pose"][0]), _bits(s.pose_in))


@pytest.mark.parametrize("box", sorted(sc.BOXES))
def test_boxes(hip_lib, box):
    s = sc.box_scene(box)
    if box == "inverted":
        run = _run(hip_lib, [s], 3)
        assert np.all(run["partial"][0][:, :ir.N_TERMS] == 0)
        assert run["status"][0] == ir.STATUS_ICP_FEW_POINTS and np.all(run["stats"][0] == 0)
        assert np.array_equal(_bits(run["pose"][0]), _bits(s.pose_in))
        return
    run = _run(hip_lib, [s], 1)
    _terms_within_bar(s, np.eye(3), np.zeros(3), run["partial"][0], s.name)


def test_invalid_camera_flags_its_pair_only(hip_lib):
    a, b, c = (sc.make(n, "cut") for n in sc.BATCH)
    bad = []
    for (i, j), v in (((0, 0), 0.0), ((1, 1), np.nan), ((0, 2), np.inf)):
        s = sc.make("f24a", "cut")
        s.K = s.K.copy()
        s.K[i, j] = v
        bad.append(s)
    for scenes in ([a, bad[0], b, bad[1]], [bad[2], c]):
        run = _run(hip_lib, scenes, 3)
        for i, s in enumerate(scenes):
            if any(s is x for x in bad):
                assert run["status"][i] == ir.STATUS_ICP_FEW_POINTS and np.all(run["stats"][i] == 0), i
                assert np.all(run["partial"][i][:, :ir.N_TERMS] == 0)
                assert np.array_equal(_bits(run["pose"][i]), _bits(s.pose_in))
            else:
                solo = _run(hip_lib, [s], 3)
                assert solo["status"][0] == 0 == run["status"][i]
                for key in ("pose", "stats"):
                    assert np.array_equal(_bits(run[key][i]), _bits(solo[key][0])), (i, key)
                assert np.array_equal(_bits(run["partial"][i][:, :ir.N_TERMS]), _bits(solo["partial"][0][:, :ir.N_TERMS])), i
                assert np.array_equal(_bits(run["state"][i][:13]), _bits(solo["state"][0][:13])), i


# ------------------------------------------------------------------------------------------------------------------ the solve's edges
def test_threshold_of_64_points(hip_lib):
    s64, s63 = sc.threshold_pair()
    r64, r63 = _run(hip_lib, [s64], 1), _run(hip_lib, [s63], 1)
    assert _block_order_sum(r64["partial"][0])[27] == 64 and _block_order_sum(r63["partial"][0])[27] == 63
    R, t, updated = _state(r63)
    assert r63["status"][0] == ir.STATUS_ICP_FEW_POINTS and updated == 0.0
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert np.array_equal(_bits(r63["pose"][0]), _bits(s63.pose_in))
    R, t, updated = _state(r64)
    assert r64["status"][0] == 0 and updated == 1.0 and np.abs(t).max() > 1e-5
    assert np.abs(r64["pose"][0] - s64.pose_in).max() > 1e-5


def test_update_then_skip(hip_lib):
    s = sc.update_then_skip()
    r1, r2 = _run(hip_lib, [s], 1), _run(hip_lib, [s], 2)
    assert r1["status"][0] == 0 and r1["state"][0, 12] == 1.0 and r1["stats"][0, 0, 0] >= ir.MIN_POINTS
    R1, t1, _ = _state(r1)
    N1 = _block_order_sum(r2["partial"][0])[27]
    assert N1 == s.truth(R1, t1)[0][27] < ir.MIN_POINTS
    assert r2["stats"][0, 1, 0] == N1 and np.array_equal(_bits(r2["stats"][0, 0]), _bits(r1["stats"][0, 0]))
    assert r2["status"][0] == ir.STATUS_ICP_FEW_POINTS
    assert r2["state"][0, 12] == 1.0                                                       # updated stays
    assert np.array_equal(_bits(r2["state"][0, :13]), _bits(r1["state"][0, :13]))          # the skipped step leaves T_1
    assert np.array_equal(_bits(r2["pose"][0]), _bits(r1["pose"][0]))                      # T_1 pose_in, not the input
    assert np.abs(r2["pose"][0] - s.pose_in).max() > 1e-4


def test_zero_residual(hip_lib):
    s = sc.zero_residual()
    run = _run(hip_lib, [s], 2)
    S = _block_order_sum(run["partial"][0])
    assert S[27] >= ir.MIN_POINTS and np.all(S[21:27] == 0) and S[28] == 0
    R, t, updated = _state(run)
    assert updated == 1.0 and run["status"][0] == 0
    assert np.array_equal(R, np.eye(3)) and np.all(t == 0)           # xi = 0 through the small-angle Rodrigues branch
    assert np.all(run["stats"][0, :, 1] == 0) and np.all(run["stats"][0, :, 0] == S[27])
    assert np.array_equal(_bits(run["pose"][0]), _bits(s.pose_in))


def test_batch_independence(hip_lib):
    scenes = [sc.make(n, "cut") for n in sc.BATCH]
    for iters in (1, 3):
        run = _run(hip_lib, scenes, iters)
        for b, s in enumerate(scenes):
            solo = _run(hip_lib, [s], iters)
            for key in ("pose", "stats", "status"):
                assert np.array_equal(run[key][b], solo[key][0]), (b, key)
            assert np.array_equal(_bits(run["pose"][b]), _bits(solo["pose"][0]))
            assert np.array_equal(_bits(run["partial"][b][:, :ir.N_TERMS]), _bits(solo["partial"][0][:, :ir.N_TERMS])), b
            assert np.array_equal(_bits(run["state"][b][:13]), _bits(solo["state"][0][:13])), b
    # and the planes are the pairs' own: pair 1 with the mask of pair 0 counts other points
    other = sc.make(sc.BATCH[1], "cut")
    other.mask = scenes[0].mask
    assert other.truth(np.eye(3), np.zeros(3))[0][27] != run["stats"][1, 0, 0]
