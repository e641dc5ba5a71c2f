"""The kernels for one object seen by several calibrated cameras: dim_views_from_rig, dim_views_consensus (csrc/views.hip) and the joint
Gauss-Newton solve gn_solve_views_kernel (csrc/twist_solve.h) behind dim_icp_refine_views, dim_sil_refine_views and
dim_photo_refine_views, against tests/views_reference.py.

The joint solve is read as tests/test_gpu_icp_terms.py reads the single-view one: the workspace is [state B x 16][partial B x 16 x 32]
[group state G x 16] doubles; after a call with iters = n the partials hold the sums of iteration n - 1, taken at the state rows after
n - 1 steps, and the state rows hold the corrections after n steps.  The solve is compared from the device's own sums.  Workspaces are
guard arenas full of NaN bits at the minimum alignment."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import icp_reference as ir  # noqa: E402
import icp_terms_scenes as sc  # noqa: E402
import views_reference as vr  # noqa: E402
import views_scenes as vs  # noqa: E402
from test_views_host import CONSENSUS_TABLE, FATAL, consensus_case  # noqa: E402

DEV = "cuda:0"
EPS64 = float(np.finfo(np.float64).eps)
FEW = ir.STATUS_ICP_FEW_POINTS


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _block_order_sum(partial):
    S = np.zeros(ir.N_TERMS)
    for k in range(16):
        S = S + partial[k, :ir.N_TERMS]
    return S


def _state(row):
    return row[:9].reshape(3, 3).copy(), row[9:12].copy(), row[12]


# ------------------------------------------------------------------------------------------------------------------ rules 1 and 2
SHAPES = [(1, 1), (1, 3), (3, 2), (2, 16)]


@pytest.mark.parametrize("G,V", SHAPES)
def test_views_from_rig(hip_lib, G, V):
    from lib.hip import ops

    X, T = vs.rig(G * 17 + V, G * V), vs.rig_poses(V, G)
    out = guard_arena.dense((G * V, 3, 4), DEV)
    ops.views_from_rig(_dev(T), _dev(X), V, pose_views=out.tensor)
    out.check("dim_views_from_rig {} x {}".format(G, V))
    want = vr.views_from_rig(T, X, V)
    assert np.all(vr.ulp_close(out.inside(), want))


def _consensus(score, status, pose, X, V, in_place=False, null_status=False):
    from lib.hip import ops

    B, G = len(pose), len(pose) // V
    choice, rig, views, st_out = (guard_arena.dense((G,), DEV, torch.int32), guard_arena.dense((G, 3, 4), DEV),
                                  guard_arena.dense((B, 3, 4), DEV), _dev(np.full(B, 1 << 20), torch.int32))
    pose_d = _dev(pose)
    ops.views_consensus(_dev(score), pose_d, _dev(X), V, status=None if null_status else _dev(status, torch.int32), fatal_mask=FATAL,
                        choice=choice.tensor, pose_rig=rig.tensor, pose_views=pose_d if in_place else views.tensor, status_out=st_out)
    for a in (choice, rig) + (() if in_place else (views,)):
        a.check("dim_views_consensus {} x {}".format(G, V))
    torch.cuda.synchronize()
    return choice.inside(), rig.inside(), pose_d.cpu().numpy() if in_place else views.inside(), st_out.cpu().numpy()


def _assert_consensus(got, score, status, pose, X, V):
    choice, rig, views, st_out = got
    r_choice, r_rig, r_views, r_bits = vr.consensus(score, status, FATAL, pose, X, V)
    assert choice.tolist() == r_choice.tolist()
    assert np.all(vr.ulp_close(rig, r_rig)) and np.all(vr.ulp_close(views, r_views))
    assert st_out.tolist() == ((1 << 20) | r_bits).tolist()              # OR-ed in, nothing else touched
    for g, c in enumerate(r_choice):
        b = g * V + max(int(c), 0)
        assert _same_bits(views[b], pose[b]), (g, c)                     # the chosen row is kept


@pytest.mark.parametrize("V", [1, 3])
def test_consensus_table(hip_lib, V):
    rows = [r for r in range(len(CONSENSUS_TABLE)) if len(CONSENSUS_TABLE[r][0]) == V]
    cases = [consensus_case(CONSENSUS_TABLE[r][0], CONSENSUS_TABLE[r][1], r) for r in rows]
    score, status, pose, X = (np.concatenate([c[i] for c in cases]) for i in range(4))
    got = _consensus(score, status, pose, X, V)
    assert got[0].tolist() == [CONSENSUS_TABLE[r][2] for r in rows]
    _assert_consensus(got, score, status, pose, X, V)
    _assert_consensus(_consensus(score, status, pose, X, V, null_status=True), score, None, pose, X, V)
    in_place = _consensus(score, status, pose, X, V, in_place=True)       # pose_views may be pose itself
    assert _same_bits(in_place[2], got[2]) and _same_bits(in_place[1], got[1])


@pytest.mark.parametrize("G,V", SHAPES)
def test_consensus_shapes(hip_lib, G, V):
    rng = np.random.default_rng(G * 100 + V)
    B = G * V
    score = rng.uniform(-1, 1, B).astype(np.float32)
    score[rng.uniform(size=B) < 0.2] = np.nan
    if V > 1:
        score[1] = score[0]                                               # a tie in group 0
    status = np.where(rng.uniform(size=B) < 0.2, 4, 32).astype(np.int32)
    pose, X = vs.rig(3, B), vs.rig(4, B)
    pose[:, 2, 3] += 1.0
    _assert_consensus(_consensus(score, status, pose, X, V), score, status, pose, X, V)


def test_views_argument_errors(hip_lib):
    z = _dev(np.zeros((4, 3, 4)))
    i4 = _dev(np.zeros(4), torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for G, V in ((0, 2), (2, 0), (2, 17), (-1, 1)):
        assert hip_lib.dim_views_from_rig(p(z), p(z), G, V, p(z), None) == -1
        assert hip_lib.dim_views_consensus(p(z), p(i4), 0, p(z), p(z), G, V, p(i4), p(z), p(z), p(i4), None) == -1
    assert hip_lib.dim_views_from_rig(None, p(z), 2, 2, p(z), None) == -1
    assert hip_lib.dim_views_from_rig(p(z), None, 2, 2, p(z), None) == -1
    assert hip_lib.dim_views_from_rig(p(z), p(z), 2, 2, None, None) == -1
    for k in (0, 3, 4, 7, 8, 9):                                          # score, pose, cam_T_rig, choice, pose_rig, pose_views
        args = [p(z), p(i4), 0, p(z), p(z), 2, 2, p(i4), p(z), p(z), p(i4), None]
        args[k] = None
        assert hip_lib.dim_views_consensus(*args) == -1, k
    assert b"null pointer" in hip_lib.dim_last_error()


# ------------------------------------------------------------------------------------------------------------------ the joint ICP solve
def _icp_inputs(scenes):
    B, s0 = len(scenes), scenes[0]
    use_mask, use_bbox, per_pair_K = s0.mask is not None, s0.bbox is not None, s0.per_pair_K
    t = dict(dr=_dev(np.stack([s.dr for s in scenes])[:, None]), do=_dev(np.stack([s.do for s in scenes])[:, None]),
             mask=_dev(np.stack([s.mask for s in scenes])[:, None]) if use_mask else None,
             bbox=_dev(np.stack([s.bbox for s in scenes]), torch.int32) if use_bbox else None,
             Kp=_dev(np.stack([s.K for s in scenes]).reshape(B, 9)) if per_pair_K else None,
             K_host=s0.K * np.float32(1.7) if per_pair_K else s0.K, pose_in=_dev(np.stack([s.pose_in for s in scenes])))
    return t


def _run_views(hip_lib, scenes, X, V, iters, pose_rig_in=None, dirty=None):
    """one dim_icp_refine_views call -> dict of numpy arrays: pose (B,3,4), pose_rig (G,3,4), stats, stats_group, status, state (B,16),
    partial (B,16,32), gstate (G,16).  dirty: a previous result whose outputs and workspace this call starts from"""
    from lib.hip import ops

    B, G, s0 = len(scenes), len(scenes) // V, scenes[0]
    H, W = s0.H, s0.W
    t = _icp_inputs(scenes)
    rig_in = vs.rig_poses(7, G) if pose_rig_in is None else pose_rig_in
    nan = float("nan")
    stats = torch.full((B, max(iters, 1), 2), nan, dtype=torch.float32, device=DEV)
    stats_group = torch.full((G, max(iters, 1), 2), nan, dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    nbytes = hip_lib.dim_icp_views_workspace_bytes(B, H, W, V)
    assert nbytes == hip_lib.dim_icp_workspace_bytes(B, H, W) + G * 16 * 8
    work = guard_arena.workspace(nbytes, 8, DEV)
    pose_out, rig_out = guard_arena.dense((B, 3, 4), DEV), guard_arena.dense((G, 3, 4), DEV)
    if dirty is not None:
        work.fill_from(_dev(dirty["workspace"], torch.float64))
        pose_out.tensor.copy_(_dev(dirty["pose"]))
        rig_out.tensor.copy_(_dev(dirty["pose_rig"]))
        stats.fill_(float(dirty["stats"][0, 0, 1]))
        stats_group.fill_(float(dirty["stats_group"][0, 0, 0]))
        status.copy_(_dev(dirty["status"], torch.int32))
    ops.icp_refine_views(t["dr"], t["do"], t["pose_in"], t["K_host"], iters, sc.MAX_DIST, _dev(X), V, _dev(rig_in), mask_observed=t["mask"],
                         bbox=t["bbox"], K_per_sample=t["Kp"], pose_out=pose_out.tensor, pose_rig_out=rig_out.tensor, stats=stats,
                         stats_group=stats_group, status=status, workspace=work.view())
    for a, what in ((work, "workspace"), (pose_out, "pose_out"), (rig_out, "pose_rig_out")):
        a.check("dim_icp_refine_views {}, B = {}, V = {}".format(what, B, V))
    ws = work.view().cpu().numpy().copy()
    return dict(pose=pose_out.inside(), pose_rig=rig_out.inside(), stats=stats.cpu().numpy(), stats_group=stats_group.cpu().numpy(),
                status=status.cpu().numpy(), state=ws[:16 * B].reshape(B, 16), partial=ws[16 * B:16 * B + 512 * B].reshape(B, 16, 32),
                gstate=ws[528 * B:].reshape(G, 16), workspace=ws, pose_rig_in=rig_in, pose_in=t["pose_in"].cpu().numpy())


def _run_single(hip_lib, scenes, iters):
    from lib.hip import ops

    B, s0 = len(scenes), scenes[0]
    t = _icp_inputs(scenes)
    stats = torch.full((B, max(iters, 1), 2), float("nan"), dtype=torch.float32, device=DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    work = guard_arena.workspace(hip_lib.dim_icp_workspace_bytes(B, s0.H, s0.W), 8, DEV)
    out = ops.icp_refine(t["dr"], t["do"], t["pose_in"], t["K_host"], iters, sc.MAX_DIST, mask_observed=t["mask"], bbox=t["bbox"],
                         K_per_sample=t["Kp"], stats=stats, status=status, workspace=work.view())
    work.check("dim_icp_refine workspace")
    return dict(pose=out.cpu().numpy(), stats=stats.cpu().numpy(), status=status.cpu().numpy())


def _assert_outputs_from_state(run, X, V):
    """pose_out and pose_rig_out within one float32 ulp of the float64 product of the device's own state rows"""
    B = len(run["pose"])
    for b in range(B):
        R, t, stepped = _state(run["state"][b])
        assert stepped == run["gstate"][b // V][12]
        want = vr.mul(vr.mat(R, t), run["pose_in"][b])
        assert np.all(vr.ulp_close(run["pose"][b], want)), b
    for g in range(B // V):
        R, t, _ = _state(run["gstate"][g])
        assert np.all(vr.ulp_close(run["pose_rig"][g], vr.mul(vr.mat(R, t), run["pose_rig_in"][g]))), g


def _assert_chain(runs, X, V, skip_views=()):
    """runs[k]: the call with iters = k + 1.  Every group's chain of joint steps from the device's own sums; skip_views: views whose
    sums the reference leaves out (they must be zero on the device)"""
    B, n = len(runs[0]["pose"]), len(runs)
    X64 = X.astype(np.float64)
    for g in range(B // V):
        rows = list(range(g * V, (g + 1) * V))
        R, t = np.eye(3), np.zeros(3)
        for k in range(n):
            run = runs[k]
            sums = np.stack([_block_order_sum(run["partial"][b]) for b in rows])
            assert np.all(np.isfinite(sums))
            N = rr = 0.0
            for v, b in enumerate(rows):
                want = vr.group_stats(sums[v, 27], sums[v, 28])
                for later in runs[k:]:                                    # bit-equal to the block-order sums, in every run that has the row
                    assert _same_bits(later["stats"][b, k], want), (g, v, k)
                N, rr = N + sums[v, 27], rr + sums[v, 28]
                if v in skip_views:
                    assert np.all(sums[v] == 0)
            for later in runs[k:]:                                        # bit-equal to the v-order sums
                assert _same_bits(later["stats_group"][g, k], vr.group_stats(N, rr)), (g, k)
            keep = [v for v in range(V) if v not in skip_views]
            R1, t1, xi = vr.views_step(R, t, sums[keep], X64[rows][keep])
            assert xi is not None and np.all(run["status"][rows] == 0), (g, k)
            Rd, td, stepped = _state(run["gstate"][g])
            tol = 1e3 * EPS64 * np.linalg.cond(vr.fuse(sums[keep], X64[rows][keep])[0])
            print("group {} k={}: |dR| {:.3g} |dt| {:.3g}, tolerance {:.3g}, |xi| {:.3g}".format(
                g, k, np.abs(Rd - R1).max(), np.abs(td - t1).max(), tol * (np.linalg.norm(xi) + 1.0), np.linalg.norm(xi)))
            assert stepped == 1.0
            assert np.abs(Rd - R1).max() <= tol * (np.linalg.norm(xi) + np.abs(R1).max()), (g, k)
            assert np.abs(td - t1).max() <= tol * (np.linalg.norm(xi) + np.abs(t1).max()), (g, k)
            for v, b in enumerate(rows):
                Rs, ts, s_stepped = _state(run["state"][b])
                Rw, tw = vr.conjugate(X64[b], R1, t1)                     # the reference's state row, by the same rule
                assert s_stepped == 1.0
                assert np.abs(Rs - Rw).max() <= tol * (np.linalg.norm(xi) + np.abs(Rw).max()), (g, v, k)
                assert np.abs(ts - tw).max() <= tol * (np.linalg.norm(xi) + np.abs(tw).max()), (g, v, k)
                Rc, tc = vr.conjugate(X64[b], Rd, td)                     # and the conjugate of the device's own D, to float64 rounding
                assert np.abs(Rs - Rc).max() <= 64 * EPS64 and np.abs(ts - tc).max() <= 64 * EPS64 * max(1.0, np.abs(tc).max()), (g, v, k)
            R, t = Rd, td
    _assert_outputs_from_state(runs[-1], X, V)


@pytest.mark.parametrize("G,V", [(1, 3), (2, 2), (1, 1)])
def test_joint_solve_from_the_device_sums(hip_lib, G, V):
    scenes, X = vs.batch_scenes(G * V), vs.rig(10 * G + V, G * V)
    runs = [_run_views(hip_lib, scenes, X, V, n) for n in (1, 2, 3)]
    _assert_chain(runs, X, V)
    assert np.abs(runs[2]["pose"] - runs[2]["pose_in"]).max() > 1e-4 and np.abs(runs[2]["pose_rig"] - runs[2]["pose_rig_in"]).max() > 1e-4
    # a second call on dirty outputs and a dirty workspace gives the same bits
    again = _run_views(hip_lib, scenes, X, V, 3, dirty=runs[1])
    for key in ("pose", "pose_rig", "stats", "stats_group", "status"):
        assert _same_bits(again[key], runs[2][key]), key
    assert _same_bits(again["state"][:, :13], runs[2]["state"][:, :13]) and _same_bits(again["gstate"][:, :13], runs[2]["gstate"][:, :13])


def test_zero_iterations_copies_both_poses(hip_lib):
    scenes, X = vs.batch_scenes(4), vs.rig(5, 4)
    run = _run_views(hip_lib, scenes, X, 2, 0)
    assert _same_bits(run["pose"], run["pose_in"]) and _same_bits(run["pose_rig"], run["pose_rig_in"])
    assert np.all(run["status"] == 0)


# ------------------------------------------------------------------------------------------------------------------ V = 1, X = identity
def test_one_view_identity_icp_is_the_single_view_entry(hip_lib):
    scenes = vs.batch_scenes(3)
    for iters in (1, 3):
        joint, single = _run_views(hip_lib, scenes, vs.identity_rig(3), 1, iters), _run_single(hip_lib, scenes, iters)
        for key in ("pose", "stats", "status"):
            assert _same_bits(joint[key], single[key]), (key, iters)
        assert _same_bits(joint["stats_group"], joint["stats"])
        assert _same_bits(joint["state"][:, :13], joint["gstate"][:, :13])
    # a pair below the bound: the same flag, the input pose
    s63 = sc.threshold_pair()[1]
    joint, single = _run_views(hip_lib, [s63], vs.identity_rig(1), 1, 2), _run_single(hip_lib, [s63], 2)
    assert joint["status"].tolist() == single["status"].tolist() == [FEW]
    assert _same_bits(joint["pose"], single["pose"]) and _same_bits(joint["pose"][0], s63.pose_in)


def test_one_view_identity_sil_is_the_single_view_entry(hip_lib):
    import test_sil_host as host
    from lib.hip import ops

    g = host.gpu_batches()[0]
    B, _, H, W = g["depth_rendered"].shape
    dep, mask, pose_in, Kps = (_dev(g[k]) for k in ("depth_rendered", "mask", "pose_in", "K_per_sample"))
    bbox = _dev(g["bbox"], torch.int32)
    field = ops.sil_edge_field(mask, host.RADIUS)
    iters = max(host.GPU_ITERS)
    out = {}
    for joint in (False, True):
        stats = torch.zeros((B, iters, 2), dtype=torch.float32, device=DEV)
        status = torch.zeros((B,), dtype=torch.int32, device=DEV)
        if joint:
            nbytes = hip_lib.dim_sil_views_workspace_bytes(B, H, W, 1)
            assert nbytes == hip_lib.dim_sil_workspace_bytes(B, H, W) + B * 16 * 8
            work = guard_arena.workspace(nbytes, 8, DEV)
            stats_group = torch.zeros((B, iters, 2), dtype=torch.float32, device=DEV)
            pose, rig = ops.sil_refine_views(dep, field, pose_in, g["K"], iters, host.HUBER, host.GATE, _dev(vs.identity_rig(B)), 1, pose_in,
                                             bbox=bbox, K_per_sample=Kps, stats=stats, stats_group=stats_group, status=status,
                                             workspace=work.view())
            work.check("dim_sil_refine_views workspace")
            assert _same_bits(rig.cpu().numpy(), pose.cpu().numpy())      # X = I: the rig pose is the sample's
            assert _same_bits(stats_group.cpu().numpy(), stats.cpu().numpy())
        else:
            pose = ops.sil_refine(dep, field, pose_in, g["K"], iters, host.HUBER, host.GATE, bbox=bbox, K_per_sample=Kps, stats=stats,
                                  status=status)
        out[joint] = (pose.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy())
    for a, b in zip(out[True], out[False]):
        assert _same_bits(a, b)
    assert np.abs(out[True][0] - g["pose_in"]).max() > 1e-5


def test_one_view_identity_photo_is_the_single_view_entry(hip_lib):
    import test_photo_host as host
    from lib.hip import ops

    g = host.gpu_batches()[1]                                             # 37 x 50: the smaller frame
    B, _, H, W = g["depth_rendered"].shape
    obs, ren, dep, pose_in, Kps = (_dev(g[k]) for k in ("image_observed", "image_rendered", "depth_rendered", "pose_in", "K_per_sample"))
    bbox = _dev(g["bbox"], torch.int32)
    levels, iters = host.GPU_LEVELS, host.GPU_ITERS
    out = {}
    for joint in (False, True):
        stats = torch.zeros((B, levels * iters, 2), dtype=torch.float32, device=DEV)
        status = torch.zeros((B,), dtype=torch.int32, device=DEV)
        if joint:
            nbytes = hip_lib.dim_photo_views_workspace_bytes(B, H, W, levels, 1)
            assert nbytes == hip_lib.dim_photo_workspace_bytes(B, H, W, levels) + B * 16 * 8
            work = guard_arena.workspace(nbytes, 16, DEV)
            stats_group = torch.zeros((B, levels * iters, 2), dtype=torch.float32, device=DEV)
            pose, rig = ops.photo_refine_views(obs, ren, dep, pose_in, g["K"], levels, iters, host.HUBER, host.GATE, _dev(vs.identity_rig(B)), 1,
                                               pose_in, bbox=bbox, K_per_sample=Kps, stats=stats, stats_group=stats_group, status=status,
                                               workspace=work.view())
            work.check("dim_photo_refine_views workspace")
            assert _same_bits(rig.cpu().numpy(), pose.cpu().numpy())
            assert _same_bits(stats_group.cpu().numpy(), stats.cpu().numpy())
        else:
            pose = ops.photo_refine(obs, ren, dep, pose_in, g["K"], levels, iters, host.HUBER, host.GATE, bbox=bbox, K_per_sample=Kps,
                                    stats=stats, status=status)
        out[joint] = (pose.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy())
    for a, b in zip(out[True], out[False]):
        assert _same_bits(a, b)
    assert np.abs(out[True][0] - g["pose_in"]).max() > 1e-5


# ------------------------------------------------------------------------------------------------------------------ the bound is the group's
def test_group_threshold(hip_lib):
    scenes, X = vs.threshold_views()
    iters = vs.THRESHOLD_ITERS
    model = vs.float32_model_chain(scenes, X, iters)
    run = _run_views(hip_lib, scenes, X, 2, iters)
    counts = run["stats"][:, :, 0]
    print("counts per view and iteration", counts.tolist(), "group", run["stats_group"][:, :, 0].tolist())
    assert np.array_equal(counts, model["stats"][:, :, 0])                # no gate decision is borderline: the counts are the model's
    assert counts.min() >= 32 and counts.max() <= 63
    assert np.all(run["stats_group"][0, :, 0] >= ir.MIN_POINTS)
    assert run["status"].tolist() == [0, 0] and run["gstate"][0, 12] == 1.0
    assert np.abs(run["pose"] - run["pose_in"]).max() > 1e-5
    _assert_outputs_from_state(run, X, 2)
    for v, s in enumerate(scenes):                                        # either view alone: flagged, and its input pose
        solo = _run_single(hip_lib, [s], iters)
        assert solo["status"].tolist() == [FEW] and solo["stats"][0, :, 0].tolist() == vs.single_view_counts(s, iters)
        assert _same_bits(solo["pose"][0], s.pose_in)


# ------------------------------------------------------------------------------------------------------------------ an empty view
@pytest.mark.parametrize("how", ["empty-box", "bad-K"])
def test_empty_view_contributes_nothing_and_moves_with_the_group(hip_lib, how):
    scenes, X = vs.batch_scenes(3), vs.rig(31, 3)
    if how == "empty-box":
        vs.empty_box(scenes[1])
    else:
        scenes[1].K = scenes[1].K.copy()
        scenes[1].K[0, 0] = 0.0
    runs = [_run_views(hip_lib, scenes, X, 3, n) for n in (1, 2, 3)]
    _assert_chain(runs, X, 3, skip_views=(1,))                            # the step is the reference's over views 0 and 2
    last = runs[2]
    assert np.all(last["stats"][1] == 0) and np.all(last["partial"][1][:, :ir.N_TERMS] == 0)
    assert np.abs(last["pose"][1] - last["pose_in"][1]).max() > 1e-4      # ... and the empty view's pose still moves with the group
    seen = vr.mul(X[1], last["pose_rig"][0])                              # consistent with the rig correction, not with its own data
    moved = vr.mul(vr.mat(*_state(last["state"][1])[:2]), last["pose_in"][1])
    assert np.all(vr.ulp_close(last["pose"][1], moved))
    D = vr.mat(*_state(last["gstate"][0])[:2])
    assert np.abs(vr.mat(*_state(last["state"][1])[:2]) - vr.mul(X[1], vr.mul(D, vr.inverse(X[1])))).max() <= 64 * EPS64
    assert np.all(np.isfinite(seen))


# ------------------------------------------------------------------------------------------------------------------ a group that never steps
def test_group_that_never_steps_and_group_independence(hip_lib):
    G, V = 3, 2
    scenes, X, rig_in = vs.batch_scenes(G * V), vs.rig(41, G * V), vs.rig_poses(9, G)
    for s in scenes[2:4]:                                                 # group 1: both views empty
        vs.empty_box(s)
    run = _run_views(hip_lib, scenes, X, V, 3, pose_rig_in=rig_in)
    assert run["status"].tolist() == [0, 0, FEW, FEW, 0, 0]
    assert _same_bits(run["pose"][2:4], run["pose_in"][2:4]) and _same_bits(run["pose_rig"][1], rig_in[1])
    assert run["gstate"][1, 12] == 0.0 and np.all(run["stats"][2:4] == 0) and np.all(run["stats_group"][1] == 0)
    for g in (0, 2):                                                      # the other groups: the bits of the group alone
        rows = slice(g * V, (g + 1) * V)
        solo = _run_views(hip_lib, scenes[rows], X[rows], V, 3, pose_rig_in=rig_in[g:g + 1])
        for key in ("pose", "stats", "status"):
            assert _same_bits(run[key][rows], solo[key]), (g, key)
        assert _same_bits(run["pose_rig"][g], solo["pose_rig"][0]) and _same_bits(run["stats_group"][g], solo["stats_group"][0])
        assert _same_bits(run["partial"][rows][:, :, :ir.N_TERMS], solo["partial"][:, :, :ir.N_TERMS])
        assert np.abs(run["pose"][rows] - run["pose_in"][rows]).max() > 1e-4


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_stage_argument_errors_return_before_a_launch(hip_lib):
    scenes = vs.batch_scenes(4)
    t = _icp_inputs(scenes)
    B, H, W = 4, scenes[0].H, scenes[0].W
    X, rig_in = _dev(vs.rig(1, 4)), _dev(vs.rig_poses(1, 2))
    work = guard_arena.workspace(hip_lib.dim_icp_views_workspace_bytes(B, H, W, 2), 8, DEV)
    pose_out, rig_out = guard_arena.dense((B, 3, 4), DEV), guard_arena.dense((2, 3, 4), DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    K9 = np.ascontiguousarray(scenes[0].K.reshape(9))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def call(**kw):
        a = dict(dr=p(t["dr"]), do=p(t["do"]), mask=p(t["mask"]), bbox=p(t["bbox"]), pose_in=p(t["pose_in"]), K9=K9.ctypes.data, Kp=p(t["Kp"]),
                 B=B, H=H, W=W, iters=2, max_dist=sc.MAX_DIST, work=p(work.view()), pose_out=p(pose_out.tensor), stats=None,
                 status=p(status), X=p(X), V=2, rig_in=p(rig_in), rig_out=p(rig_out.tensor), stats_group=None)
        a.update(kw)
        return hip_lib.dim_icp_refine_views(a["dr"], a["do"], a["mask"], a["bbox"], a["pose_in"], a["K9"], a["Kp"], a["B"], a["H"], a["W"],
                                            a["iters"], a["max_dist"], a["work"], a["pose_out"], a["stats"], a["status"], a["X"], a["V"],
                                            a["rig_in"], a["rig_out"], a["stats_group"], None)

    bad = [dict(V=0), dict(V=-1), dict(V=17), dict(V=3), dict(X=None), dict(rig_in=None), dict(rig_out=None),            # the views' own
           dict(B=0), dict(iters=-1), dict(max_dist=0.0), dict(H=2), dict(dr=None), dict(pose_in=None), dict(work=None),  # the single-view entry's
           dict(pose_out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for fn, args in ((hip_lib.dim_icp_views_workspace_bytes, (B, H, W)), (hip_lib.dim_sil_views_workspace_bytes, (B, H, W)),
                     (hip_lib.dim_photo_views_workspace_bytes, (B, 48, 64, 2))):
        assert fn(*args, 0) == 0 and fn(*args, 2) > 0
    torch.cuda.synchronize()
    for a in (work, pose_out, rig_out):                                   # nothing ran: every buffer keeps its fill
        a.check("argument errors")
    assert np.all(np.isnan(work.view().cpu().numpy())) and np.all(np.isnan(pose_out.inside())) and np.all(np.isnan(rig_out.inside()))
    assert status.cpu().tolist() == [0] * B
    assert call() == 0                                                    # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert np.all(np.isfinite(pose_out.inside()))
