"""CPU: what the bars of tests/test_gpu_pose_algebra.py rest on, shown before any GPU run.

* oracle.transform3d (float32 numpy) against the float64 autograd reference on the new Transform3D cases: what one float32
  evaluation alone is off by (3.4e-7 forward, 2.0e-6 / 1.2e-6 d_rot / d_trans here), which the GPU bars (2e-6, 1e-5) are 5x to 8x of.
* the SE(3) table reaches all four branches of mat2quat_d for every rot_coord, and Shepperd's selection agrees with the oracle's
  eigenvector mat2quat on it.
* each planted fault misses the GPU bars by at least 100x on the new cases -- and four of them change nothing at all on the one
  input set the suite had before."""
import numpy as np
import pytest

import pose_algebra_reference as R
from oracle import transform3d as ot3d

SEP = 100.0


def _f32(setting):
    m, s = R.SETTINGS[setting]
    return np.asarray(m, np.float32), np.asarray(s, np.float32)


# ------------------------------------------------------------------------------------------------ Transform3D
def test_oracle_transform3d_agrees_with_autograd_on_general_poses():
    worst = dict(fwd=0.0, d_rot=0.0, d_trans=0.0, restated_fwd=0.0, restated_grad=0.0)
    for B, N in R.T3D_SHAPES:
        inp = R.t3d_inputs(B, N)
        for setting in R.SETTINGS:
            m, s = _f32(setting)
            for coord in R.COORDS:
                out, d_rot, d_trans = R.t3d_case_reference(B, N, coord, setting)
                o = ot3d.forward(inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
                r, t = ot3d.backward(inp["out_grad"], inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
                worst["fwd"] = max(worst["fwd"], float(np.abs(o - out).max()))
                worst["d_rot"] = max(worst["d_rot"], R.grad_err(r, d_rot))
                worst["d_trans"] = max(worst["d_trans"], R.grad_err(t, d_trans))
                # the float64 restatement that the negative controls mutate is itself the definition: only the float32 rounding of
                # the unit quaternions (|q|^2 - 1 ~ 1e-7, the Ns factors of quat2mat_backward) separates its gradient from autograd's
                ro, rr, rt = R.t3d_restated(inp, coord, setting)
                worst["restated_fwd"] = max(worst["restated_fwd"], float(np.abs(ro - out).max()))
                worst["restated_grad"] = max(worst["restated_grad"], R.grad_err(rr, d_rot), R.grad_err(rt, d_trans))
    print("oracle.transform3d vs float64 autograd: forward {fwd:.3g} abs, d_rot {d_rot:.3g}, d_trans {d_trans:.3g} of the sample's "
          "largest entry; float64 restatement: forward {restated_fwd:.3g}, gradients {restated_grad:.3g}".format(**worst))
    assert worst["fwd"] <= 1e-6
    assert worst["d_rot"] <= 5e-6 and worst["d_trans"] <= 5e-6
    assert worst["restated_fwd"] <= 1e-12 and worst["restated_grad"] <= 1e-6


def test_restatement_is_the_oracle_on_the_quaternion_norm_cases():
    """off the unit sphere the Ns factors make the reference's gradient differ from the true one, so the float32 oracle is the
    reference there; the restatement takes the same branches"""
    inp = R.t3d_norm_inputs()
    far_f, far_b = np.abs(inp["delta"]) > 1e-2, np.abs(inp["delta"]) > 1e-4
    assert far_f.sum() == 2 and far_b.sum() == 6
    for setting in R.SETTINGS:
        m, s = _f32(setting)
        for coord in R.COORDS:
            o = ot3d.forward(inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
            r, t = ot3d.backward(inp["out_grad"], inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
            ro, rr, rt = R.t3d_restated(inp, coord, setting)
            assert np.abs(o - ro).max() <= 1e-6
            assert (r[far_b] == 0).all() and (rr[far_b] == 0).all()
            assert R.grad_err(r[~far_b], rr[~far_b]) <= 5e-6 and R.grad_err(t, rt) <= 5e-6
            assert np.abs(t).min() > 0


# ------------------------------------------------------------------------------------------------ SE(3) table
@pytest.mark.parametrize("coord", R.COORDS)
def test_se3_table_reaches_every_quaternion_branch(coord):
    ref = R.se3_delta_ref(coord, "unit")
    hit = np.bincount([R.quat_branch(M) for M in ref["R"]], minlength=4)
    print("{}: rows per branch (tr, M00, M11, M22) = {}".format(coord, hit.tolist()))
    assert (hit > 0).all()


def test_se3_table_layout():
    tab = R.se3_table()
    assert tab["src"].shape == (130, 3, 4) and R.N_ROWS == 130
    same = [i for i in range(130) if np.array_equal(tab["src"][i], tab["tgt"][i])]
    assert len(same) == len(R.AXES) and all(tab["angle"][i] == 0.0 for i in same)
    assert (tab["angle"] <= 1e-3).sum() == 4 * len(R.AXES)
    # built rows really are at their angle (float32 rounding of the poses moves it by ~1e-7)
    for i in np.flatnonzero(~np.isnan(tab["angle"])):
        M = tab["src"][i, :, :3].astype(np.float64).T @ tab["tgt"][i, :, :3].astype(np.float64)
        sin_a = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
        assert abs(np.arctan2(sin_a, 0.5 * (np.trace(M) - 1.0)) - tab["angle"][i]) < 1e-6


def test_shepperd_agrees_with_the_eigenvector_mat2quat():
    tab = R.se3_table()
    small = tab["angle"] <= 1e-3
    for coord in R.COORDS:
        ref = R.se3_delta_ref(coord, "unit")
        got = np.array([R.shepperd(M) for M in ref["R"]])
        assert (got[:, 0] >= 0).all()
        strict = np.abs(got - ref["q"]).max(1)
        err = R.quat_err(got, ref["q"], free_sign_below=1e-7)
        flipped = np.flatnonzero(strict > 1e-3)
        print("{}: Shepperd vs eigenvector mat2quat: {:.3g} abs on all rows, {:.3g} on the rows with angle <= 1e-3; sign differs on rows {} "
              "(angles {})".format(coord, err.max(), err[small].max(), flipped.tolist(), tab["angle"][flipped].tolist()))
        assert (np.abs(ref["q"][flipped, 0]) < 1e-7).all()           # a global sign only where w is rounding noise (exact pi)
        assert err.max() <= 5e-8
        if coord != "NAIVE":    # NAIVE's residual is rounded to float32 by the reference; its small-angle figure is only recorded
            assert err[small].max() <= 1.3e-11


def test_euler_lock_rows_take_the_lock_branch():
    tab = R.euler_table()
    assert tab["lock"].sum() == len(R.LOCK) and tab["src"].shape[0] == R.N_EULER + len(R.LOCK)
    near = np.abs(np.abs(tab["se3"][:R.N_EULER, 1].astype(np.float64)) - np.pi / 2) < 1.001e-3
    assert near[::5].all() and near.sum() >= R.N_EULER // 5
    for coord in R.COORDS:
        ref = R.se3_delta_ref(coord, "unit", "euler")
        cy = np.hypot(ref["R"][:, 0, 0], ref["R"][:, 1, 0])
        assert (cy[tab["lock"]] <= 4 * np.finfo(float).eps).all() and (cy[~tab["lock"]] > 1e-7).all()
        assert (ref["e"][tab["lock"], 2] == 0.0).all()
        # the residual of a lock row is the target's float32 matrix itself: nothing was rounded on the way
        assert np.array_equal(ref["R"][tab["lock"]], tab["tgt"][tab["lock"], :, :3].astype(np.float64))


def test_pose_to_KT_reference_bound_is_not_vacuous():
    tab = R.se3_table()
    for K in (R.K_LINEMOD, R.K_SKEW):
        ref, bound = R.pose_to_KT_ref(tab["src"], tab["tgt"], K)
        assert ref.shape == (130, 3, 4) and (bound > 0).all()
        assert (bound <= 1e-6 * 900 * 3).all()                         # |K| row sums < 900, |M| entries < 3 (two translations)
    a, _ = R.pose_to_KT_ref(tab["src"], tab["tgt"], R.K_LINEMOD)
    b, bound = R.pose_to_KT_ref(tab["src"], tab["tgt"], R.K_SKEW)
    assert (np.abs(a - b)[:, 0] > 100 * bound[:, 0]).any()            # dropping K01 is seen


# ------------------------------------------------------------------------------------------------ negative controls
def _t3d_miss(fault, coords, settings, shapes=R.T3D_SHAPES):
    """-> the largest miss, in GPU bars, of the mutated restatement against the float64 autograd reference, per (coord, setting)"""
    miss = {}
    for coord in coords:
        for setting in settings:
            worst = 0.0
            for B, N in shapes:
                inp = R.t3d_inputs(B, N)
                out, d_rot, d_trans = R.t3d_case_reference(B, N, coord, setting)
                mo, mr, mt = R.t3d_restated(inp, coord, setting, fault)
                worst = max(worst, np.abs(mo - out).max() / R.T3D_FWD_BAR, R.grad_err(mr, d_rot) / R.T3D_GRAD_BAR,
                            R.grad_err(mt, d_trans) / R.T3D_GRAD_BAR)
            miss[coord, setting] = worst
    return miss


# where each fault can act at all: NAIVE has no Rs^T, no stds and no x/z terms; CAMERA_NEW no x/z terms; stds = 1 hides (c)
FAULT_SCOPE = {
    "Rs_not_transposed": (("MODEL", "CAMERA", "CAMERA_NEW"), ("unit", "golden")),
    "pose_of_sample_0": (R.COORDS, ("unit", "golden")),
    "stds_one_in_backward": (("MODEL", "CAMERA", "CAMERA_NEW"), ("golden",)),
    "no_xy_over_z": (("MODEL", "CAMERA"), ("unit", "golden")),
    "tail_points_dropped": (R.COORDS, ("unit", "golden")),
}


@pytest.mark.parametrize("fault", R.T3D_FAULTS)
def test_planted_transform3d_fault_misses_the_gpu_bars(fault):
    coords, settings = FAULT_SCOPE[fault]
    miss = _t3d_miss(fault, coords, settings)
    print("{}: misses the GPU bars by {}".format(fault, {k: "{:.3g}x".format(v) for k, v in miss.items()}))
    assert min(miss.values()) >= SEP
    if fault == "tail_points_dropped":
        # every Npts off a multiple of 256 sees it on its own, the sub-wave and sub-block ones included
        for B, N in R.T3D_SHAPES:
            if N % 256:
                assert min(_t3d_miss(fault, ("CAMERA",), ("unit",), ((B, N),)).values()) >= SEP, (B, N)


def test_planted_always_w_branch_misses_the_quaternion_bar():
    for coord in R.COORDS:
        ref = R.se3_delta_ref(coord, "unit")
        with np.errstate(invalid="ignore"):     # NAIVE at exactly pi: the float32 residual leaves 0 / 0, which misses any bar
            err = R.quat_err(np.array([R.shepperd(M, always_w=True) for M in ref["R"]]), ref["q"])
        err = np.where(np.isnan(err), np.inf, err)
        print("{}: always-w mat2quat misses the 2e-6 bar by {:.3g}x".format(coord, err.max() / 2e-6))
        assert err.max() >= SEP * 2e-6


def test_the_old_input_set_could_not_see_faults_a_to_d():
    """the gap: one shared symmetric pose with T = (0, 0, 1), means 0 and stds 1 -- every fault below leaves every number as it was"""
    inp = R.old_inputs()
    for coord in R.COORDS:
        clean = R.t3d_restated(inp, coord, "unit")
        for fault in ("Rs_not_transposed", "pose_of_sample_0", "stds_one_in_backward", "no_xy_over_z"):
            for a, b in zip(clean, R.t3d_restated(inp, coord, "unit", fault)):
                assert np.array_equal(a, b), (coord, fault)
    # ... and its Npts = 3000 is the only one it had: (e) is visible there, but no Npts below one block or one wave ever ran
    assert R.grad_err(R.t3d_restated(inp, "CAMERA", "unit", "tail_points_dropped")[1], R.t3d_restated(inp, "CAMERA", "unit")[1]) > 0
