"""dim_icp_refine_rig (gn_rig_group_kernel and gn_rig_solve_kernel of csrc/twist_solve.h) against tests/rig_reference.py, read as
tests/test_gpu_views_kernels.py reads the joint solve: the workspace is [state B x 16][partial B x 16 x 32][group state G x 16]
[rig state V x 16][per group V x 104 + 8] doubles; after a call with iters = n the partials hold the sums of iteration n - 1, taken at
the state rows after n - 1 steps, and the states hold the corrections after n steps.  Every step is compared from the device's own
sums and its own previous state.  Workspaces are guard arenas full of NaN bits at the minimum alignment; frames are 24 x 32."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import icp_reference as ir  # noqa: E402
import icp_terms_scenes as sc  # noqa: E402
import rig_reference as rr  # noqa: E402
import views_reference as vr  # noqa: E402
import views_scenes as vs  # noqa: E402
from test_gpu_views_kernels import DEV, EPS64, FEW, _block_order_sum, _dev, _icp_inputs, _run_views, _same_bits, _state  # noqa: E402

HELD = rr.STATUS_VIEWS_CALIB_HELD
SHAPES = [(1, 1), (1, 2), (2, 2), (1, 3), (3, 2), (2, 8), (1, 16)]


def _tiled_rig(seed, G, V):
    return np.tile(vs.rig(seed, V), (G, 1, 1))


def _run_rig(hip_lib, scenes, X, V, iters, pose_rig_in=None, dirty=None):
    """one dim_icp_refine_rig call -> dict of numpy arrays: the outputs, and the workspace cut into state (B,16), partial (B,16,32),
    gstate (G,16), rstate (V,16).  dirty: a previous result whose outputs and workspace this call starts from"""
    from lib.hip import ops

    B, G, s0 = len(scenes), len(scenes) // V, scenes[0]
    H, W = s0.H, s0.W
    t = _icp_inputs(scenes)
    rig_in = vs.rig_poses(7, G) if pose_rig_in is None else pose_rig_in
    n = max(iters, 1)
    full = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    stats, stats_group, stats_view = full(B, n, 2), full(G, n, 2), full(V, n, 2)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    nbytes = hip_lib.dim_icp_rig_workspace_bytes(B, H, W, V)
    assert nbytes == hip_lib.dim_icp_views_workspace_bytes(B, H, W, V) + 8 * (16 * V + G * (104 * V + 8))
    work = guard_arena.workspace(nbytes, 8, DEV)
    pose_out, rig_out, cam_out = guard_arena.dense((B, 3, 4), DEV), guard_arena.dense((G, 3, 4), DEV), guard_arena.dense((B, 3, 4), DEV)
    if dirty is not None:
        work.fill_from(_dev(dirty["workspace"], torch.float64))
        pose_out.tensor.copy_(_dev(dirty["pose"]))
        rig_out.tensor.copy_(_dev(dirty["pose_rig"]))
        cam_out.tensor.copy_(_dev(dirty["cam"]))
        for a in (stats, stats_group, stats_view):
            a.fill_(float(dirty["stats"][0, 0, 1]))
        status.copy_(_dev(dirty["status_in"], torch.int32))
    ops.icp_refine_rig(t["dr"], t["do"], t["pose_in"], t["K_host"], iters, sc.MAX_DIST, _dev(X), V, _dev(rig_in), mask_observed=t["mask"],
                       bbox=t["bbox"], K_per_sample=t["Kp"], pose_out=pose_out.tensor, pose_rig_out=rig_out.tensor,
                       cam_T_rig_out=cam_out.tensor, stats=stats, stats_group=stats_group, stats_view=stats_view, status=status,
                       workspace=work.view())
    for a, what in ((work, "workspace"), (pose_out, "pose_out"), (rig_out, "pose_rig_out"), (cam_out, "cam_T_rig_out")):
        a.check("dim_icp_refine_rig {}, B = {}, V = {}".format(what, B, V))
    ws = work.view().cpu().numpy().copy()
    o = 528 * B
    return dict(pose=pose_out.inside(), pose_rig=rig_out.inside(), cam=cam_out.inside(), stats=stats.cpu().numpy(),
                stats_group=stats_group.cpu().numpy(), stats_view=stats_view.cpu().numpy(), status=status.cpu().numpy(),
                state=ws[:16 * B].reshape(B, 16), partial=ws[16 * B:o].reshape(B, 16, 32), gstate=ws[o:o + 16 * G].reshape(G, 16),
                rstate=ws[o + 16 * G:o + 16 * (G + V)].reshape(V, 16), workspace=ws, pose_rig_in=rig_in, pose_in=t["pose_in"].cpu().numpy(),
                status_in=np.zeros(B, np.int32))


def _device_state(run):
    """C, D, moved as the device holds them after a call"""
    C = [_state(r)[:2] for r in run["rstate"]]
    D = [_state(r)[:2] for r in run["gstate"]]
    return C, D, run["rstate"][:, 12] != 0


def _close(got, want, tol, scale):
    return np.abs(got - want).max() <= tol * (scale + np.abs(want).max())


def _assert_rig_chain(runs, X, V):
    """runs[k]: the call with iters = k + 1 -> the status bits the reference expects after the last"""
    B, n = len(runs[0]["pose"]), len(runs)
    G = B // V
    X64 = X[:V].astype(np.float64)
    C, D, moved = [rr.IDENTITY] * V, [rr.IDENTITY] * G, np.zeros(V, bool)
    stepped, status = np.zeros(G, bool), np.zeros(B, np.int64)
    for k in range(n):
        run = runs[k]
        sums = np.stack([_block_order_sum(run["partial"][b]) for b in range(B)]).reshape(G, V, ir.N_TERMS)
        assert np.all(np.isfinite(sums))
        for b in range(B):                                                # bit-equal to the block-order sums
            for later in runs[k:]:
                assert _same_bits(later["stats"][b, k], vr.group_stats(sums[b // V, b % V, 27], sums[b // V, b % V, 28])), (b, k)
        for g in range(G):                                                # ... and to the ordered sums over v and over g
            N = rr_ = 0.0
            for v in range(V):
                N, rr_ = N + sums[g, v, 27], rr_ + sums[g, v, 28]
            for later in runs[k:]:
                assert _same_bits(later["stats_group"][g, k], vr.group_stats(N, rr_)), (g, k)
        for v in range(V):
            N = rr_ = 0.0
            for g in range(G):
                N, rr_ = N + sums[g, v, 27], rr_ + sums[g, v, 28]
            for later in runs[k:]:
                assert _same_bits(later["stats_view"][v, k], vr.group_stats(N, rr_)), (v, k)
        step = rr.rig_step(sums, X64, C, D, moved)
        status, stepped = status | step["bits"], stepped | step["stepped"]
        bk = step["blocks"]
        Hfull, rfull = rr.dense_system(bk)
        tol = 1e3 * EPS64 * (np.linalg.cond(Hfull) if len(Hfull) else 1.0)
        sol = np.linalg.norm(np.linalg.solve(Hfull, rfull)) if len(Hfull) else 0.0
        Cd, Dd, moved_d = _device_state(run)
        print("k={}: free {} active {} tolerance {:.3g} |x| {:.3g}; worst |dC| {:.3g} |dD| {:.3g}".format(
            k, bk["fl"], bk["gl"], tol * (sol + 1), sol,
            max(np.abs(vr.mat(*Cd[v]) - vr.mat(*step["C"][v])).max() for v in range(V)),
            max(np.abs(vr.mat(*Dd[g]) - vr.mat(*step["D"][g])).max() for g in range(G))))
        assert moved_d.tolist() == step["moved"].tolist() and (run["gstate"][:, 12] != 0).tolist() == stepped.tolist()
        assert run["status"].tolist() == status.tolist(), k
        for v in range(V):
            assert _close(Cd[v][0], step["C"][v][0], tol, sol) and _close(Cd[v][1], step["C"][v][1], tol, sol), (v, k)
        assert np.array_equal(Cd[0][0], np.eye(3)) and np.array_equal(Cd[0][1], np.zeros(3)) and not moved_d[0]
        for g in range(G):
            assert _close(Dd[g][0], step["D"][g][0], tol, sol) and _close(Dd[g][1], step["D"][g][1], tol, sol), (g, k)
        Xc_ref, Xc_dev = rr.current_extrinsics(X64, step["C"], step["moved"]), rr.current_extrinsics(X64, Cd, moved_d)
        for b in range(B):
            g, v = b // V, b % V
            Rs, ts, flag = _state(run["state"][b])
            Rw, tw = rr.state_row(Xc_ref[v], step["D"][g], X64[v])
            assert flag == float(stepped[g])
            assert _close(Rs, Rw, tol, sol) and _close(ts, tw, tol, sol), (b, k)
            Rc, tc = rr.state_row(Xc_dev[v], Dd[g], X64[v])               # and the rule on the device's own C and D, to float64 rounding
            assert np.abs(Rs - Rc).max() <= 64 * EPS64 and np.abs(ts - tc).max() <= 64 * EPS64 * max(1.0, np.abs(tc).max()), (b, k)
        C, D, moved = Cd, Dd, moved_d
    _assert_outputs_from_state(runs[-1], X, V)
    return status


def _assert_outputs_from_state(run, X, V):
    """the three outputs within one float32 ulp of the float64 products of the device's own state; the untouched ones bit for bit"""
    B = len(run["pose"])
    Cd, Dd, moved = _device_state(run)
    Xc = rr.current_extrinsics(X[:V].astype(np.float64), Cd, moved)
    for b in range(B):
        g, v = b // V, b % V
        R, t, stepped = _state(run["state"][b])
        if stepped:
            assert np.all(vr.ulp_close(run["pose"][b], vr.mul(vr.mat(R, t), run["pose_in"][b]))), b
        else:
            assert _same_bits(run["pose"][b], run["pose_in"][b]), b
        if moved[v]:
            assert np.all(vr.ulp_close(run["cam"][b], Xc[v])), b
        else:
            assert _same_bits(run["cam"][b], X[v]), b
    for g in range(B // V):
        if run["gstate"][g, 12]:
            assert np.all(vr.ulp_close(run["pose_rig"][g], vr.mul(vr.mat(*Dd[g]), run["pose_rig_in"][g]))), g
        else:
            assert _same_bits(run["pose_rig"][g], run["pose_rig_in"][g]), g


OUTPUTS = ("pose", "pose_rig", "cam", "stats", "stats_group", "stats_view", "status")


@pytest.mark.parametrize("G,V", SHAPES)
def test_rig_chain_from_the_device_sums(hip_lib, G, V):
    scenes, X = vs.batch_scenes(G * V), _tiled_rig(10 * G + V, G, V)
    runs = [_run_rig(hip_lib, scenes, X, V, n) for n in (1, 2, 3)]
    status = _assert_rig_chain(runs, X, V)
    assert not np.any(status), status                                     # every group active, every view free, every system positive definite
    last = runs[2]
    assert last["rstate"][1:, 12].tolist() == [1.0] * (V - 1)
    assert np.abs(last["pose"] - last["pose_in"]).max() > 1e-4
    if V > 1:
        assert np.abs(last["cam"][1] - X[1]).max() > 1e-5
    for g in range(G):                                                    # camera 0 keeps its bits; the rig is repeated for every group
        assert _same_bits(last["cam"][g * V], X[0])
        assert _same_bits(last["cam"][g * V:(g + 1) * V], last["cam"][:V])
    again = _run_rig(hip_lib, scenes, X, V, 3, dirty=runs[1])             # dirty outputs and a dirty workspace: the same bits
    for key in OUTPUTS:
        assert _same_bits(again[key], last[key]), key
    for key in ("state", "gstate", "rstate"):
        assert _same_bits(again[key][:, :13], last[key][:, :13]), key


def test_one_view_is_the_joint_entry(hip_lib):
    scenes, X = vs.batch_scenes(3), _tiled_rig(3, 3, 1)
    rig_in = vs.rig_poses(5, 3)
    for iters in (0, 1, 3):
        rig, joint = _run_rig(hip_lib, scenes, X, 1, iters, pose_rig_in=rig_in), _run_views(hip_lib, scenes, X, 1, iters, pose_rig_in=rig_in)
        for key in ("pose", "pose_rig", "status") + (("stats", "stats_group") if iters else ()):
            assert _same_bits(rig[key], joint[key]), (key, iters)
        assert _same_bits(rig["cam"], X)
        if iters:
            assert _same_bits(rig["state"][:, :13], joint["state"][:, :13]) and _same_bits(rig["gstate"][:, :13], joint["gstate"][:, :13])
    assert np.abs(rig["pose"] - rig["pose_in"]).max() > 1e-4


def test_view_with_an_empty_box_is_held(hip_lib):
    G, V = 2, 3
    scenes, X = vs.batch_scenes(G * V), _tiled_rig(31, G, V)
    for g in range(G):
        vs.empty_box(scenes[g * V + 1])
    runs = [_run_rig(hip_lib, scenes, X, V, n) for n in (1, 2, 3)]
    status = _assert_rig_chain(runs, X, V)
    assert status.tolist() == [0, HELD, 0] * G
    last = runs[2]
    assert last["rstate"][:, 12].tolist() == [0.0, 0.0, 1.0]              # view 2 is calibrated, view 1 never
    for g in range(G):
        b = g * V + 1
        assert _same_bits(last["cam"][b], X[1]) and np.all(last["stats"][b] == 0)
        assert np.abs(last["pose"][b] - last["pose_in"][b]).max() > 1e-4  # ... and its samples move with their groups
        D = vr.mat(*_state(last["gstate"][g])[:2])
        want = vr.mul(X[1], vr.mul(D, vr.inverse(X[1])))
        assert np.abs(vr.mat(*_state(last["state"][b])[:2]) - want).max() <= 64 * EPS64
    assert np.all(last["stats_view"][1] == 0)


def _window_scene(box):
    s = sc.make("f24a", "plain")
    s.bbox = np.array(box, np.int32)
    return s


def test_group_below_the_threshold_is_inactive(hip_lib):
    G, V = 2, 2
    whole = (0, 31, 0, 23)
    scenes = [_window_scene(whole), _window_scene(whole), _window_scene(vs.THRESHOLD_BOXES[0]), vs.empty_box(_window_scene(whole))]
    X, rig_in = _tiled_rig(8, G, V), vs.rig_poses(9, G)
    runs = [_run_rig(hip_lib, scenes, X, V, n, pose_rig_in=rig_in) for n in (1, 2)]
    status = _assert_rig_chain(runs, X, V)
    last = runs[1]
    assert 0 < last["stats_group"][1, 0, 0] < ir.MIN_POINTS <= last["stats_group"][0, 0, 0]
    assert status.tolist() == [0, 0, FEW, FEW]                            # only its samples; view 1 is free through group 0
    assert _same_bits(last["pose"][2:], last["pose_in"][2:]) and _same_bits(last["pose_rig"][1], rig_in[1])
    assert last["gstate"][:, 12].tolist() == [1.0, 0.0] and last["rstate"][1, 12] == 1.0
    assert np.abs(last["pose"][:2] - last["pose_in"][:2]).max() > 1e-4
    # the inactive group's state rows still follow the calibrated camera: X'_1 X_1^-1, not the identity
    assert np.abs(vr.mat(*_state(last["state"][3])[:2]) - np.eye(3, 4)).max() > 1e-6


def test_view_is_free_only_through_groups_the_gauge_camera_sees(hip_lib):
    G, V = 2, 2
    scenes, X = vs.batch_scenes(G * V), _tiled_rig(12, G, V)
    vs.empty_box(scenes[0])                                               # group 0: camera 0 sees nothing, camera 1 alone carries it
    runs = [_run_rig(hip_lib, scenes, X, V, n) for n in (1, 2)]
    assert _assert_rig_chain(runs, X, V).tolist() == [0] * 4 and runs[1]["rstate"][1, 12] == 1.0
    vs.empty_box(scenes[2])                                               # group 1 as well: no group ties camera 1 to the gauge
    runs = [_run_rig(hip_lib, scenes, X, V, n) for n in (1, 2)]
    assert _assert_rig_chain(runs, X, V).tolist() == [0, HELD] * 2
    assert runs[1]["rstate"][1, 12] == 0.0 and runs[1]["gstate"][:, 12].tolist() == [1.0, 1.0]
    assert _same_bits(runs[1]["cam"], X)


def test_zero_iterations_copies_the_three_inputs(hip_lib):
    scenes, X = vs.batch_scenes(4), _tiled_rig(5, 2, 2)
    run = _run_rig(hip_lib, scenes, X, 2, 0)
    assert _same_bits(run["pose"], run["pose_in"]) and _same_bits(run["pose_rig"], run["pose_rig_in"]) and _same_bits(run["cam"], X)
    assert np.all(run["status"] == 0) and np.all(np.isnan(run["workspace"]))


def test_argument_errors_return_before_a_launch(hip_lib):
    scenes = vs.batch_scenes(4)
    t = _icp_inputs(scenes)
    B, H, W = 4, scenes[0].H, scenes[0].W
    X, rig_in = _dev(_tiled_rig(1, 2, 2)), _dev(vs.rig_poses(1, 2))
    work = guard_arena.workspace(hip_lib.dim_icp_rig_workspace_bytes(B, H, W, 2), 8, DEV)
    pose_out, rig_out, cam_out = guard_arena.dense((B, 3, 4), DEV), guard_arena.dense((2, 3, 4), DEV), guard_arena.dense((B, 3, 4), DEV)
    status = torch.zeros((B,), dtype=torch.int32, device=DEV)
    K9 = np.ascontiguousarray(scenes[0].K.reshape(9))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def call(**kw):
        a = dict(dr=p(t["dr"]), do=p(t["do"]), mask=p(t["mask"]), bbox=p(t["bbox"]), pose_in=p(t["pose_in"]), K9=K9.ctypes.data, Kp=p(t["Kp"]),
                 B=B, H=H, W=W, iters=2, max_dist=sc.MAX_DIST, work=p(work.view()), pose_out=p(pose_out.tensor), stats=None,
                 status=p(status), X=p(X), V=2, rig_in=p(rig_in), rig_out=p(rig_out.tensor), stats_group=None, cam_out=p(cam_out.tensor),
                 stats_view=None)
        a.update(kw)
        return hip_lib.dim_icp_refine_rig(a["dr"], a["do"], a["mask"], a["bbox"], a["pose_in"], a["K9"], a["Kp"], a["B"], a["H"], a["W"],
                                          a["iters"], a["max_dist"], a["work"], a["pose_out"], a["stats"], a["status"], a["X"], a["V"],
                                          a["rig_in"], a["rig_out"], a["stats_group"], a["cam_out"], a["stats_view"], None)

    bad = [dict(cam_out=None), dict(cam_out=None, iters=0), dict(V=0), dict(V=-1), dict(V=17), dict(V=3), dict(X=None), dict(rig_in=None),
           dict(rig_out=None), dict(B=0), dict(iters=-1), dict(max_dist=0.0), dict(H=2), dict(dr=None), dict(pose_in=None), dict(work=None),
           dict(pose_out=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert hip_lib.dim_icp_rig_workspace_bytes(B, H, W, 0) == 0 and hip_lib.dim_icp_rig_workspace_bytes(0, H, W, 2) == 0
    torch.cuda.synchronize()
    for a in (work, pose_out, rig_out, cam_out):                          # nothing ran: every buffer keeps its fill
        a.check("argument errors")
    assert np.all(np.isnan(work.view().cpu().numpy()))
    assert all(np.all(np.isnan(a.inside())) for a in (pose_out, rig_out, cam_out)) and status.cpu().tolist() == [0] * B
    assert call() == 0                                                    # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert np.all(np.isfinite(pose_out.inside())) and np.all(np.isfinite(cam_out.inside()))
