"""The pose algebra of csrc/se3.hip (se3_compose / se3_delta* / pose_to_KT / transform3d_fwd / transform3d_bwd) on general poses and
at the edges: every sample its own pose, non-trivial T_means / T_stds for every rot_coord, Npts below a wave, below a block and off
a multiple of 256, three thread blocks of poses, every branch of mat2quat_d, rotations of 0, 1e-7 rad and pi, the gimbal lock.
References, case tables and bars: tests/pose_algebra_reference.py; tests/test_pose_algebra_host.py shows on the CPU what each bar is
a multiple of and that each planted fault misses it by more than 100x."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pose_algebra_reference as R  # noqa: E402
from oracle import transform3d as ot3d  # noqa: E402

DEV = "cuda:0"
SMALL = 1e-3       # "tiny rotation": the rows of the SE(3) table at or below this angle


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from lib.hip import ops as o

    return o


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)      # a copy: the tables are read-only


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def f32_ms(setting):
    m, s = R.SETTINGS[setting]
    return np.asarray(m, np.float32), np.asarray(s, np.float32)


def t3d_run(ops, inp, coord, setting):
    m, s = f32_ms(setting)
    a = {k: dev(inp[k]) for k in ("pts", "rot", "trans", "pose_src", "out_grad")}
    out = ops.transform3d_fwd(a["pts"], a["rot"], a["trans"], a["pose_src"], coord, m, s)
    d_rot, d_trans = ops.transform3d_bwd(a["out_grad"], a["pts"], a["rot"], a["trans"], a["pose_src"], coord, m, s)
    return host(out).astype(np.float64), host(d_rot).astype(np.float64), host(d_trans).astype(np.float64)


# ------------------------------------------------------------------------------------------------ Transform3D
@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("coord", R.COORDS)
@pytest.mark.parametrize("B,N", R.T3D_SHAPES)
def test_transform3d_vs_float64_autograd(ops, B, N, coord, setting):
    """forward 2e-6 abs, gradients 1e-5 of the sample's largest reference entry.  The float32 numpy oracle alone is at 3.4e-7 /
    2.0e-6 / 1.2e-6 (forward / d_rot / d_trans) on these cases (test_pose_algebra_host.py prints it); the kernels measured
    3.4e-7 / 1.4e-6 / 1.7e-6 on an MI355X."""
    inp = R.t3d_inputs(B, N)
    ref_out, ref_rot, ref_trans = R.t3d_case_reference(B, N, coord, setting)
    out, d_rot, d_trans = t3d_run(ops, inp, coord, setting)
    e_f, e_r, e_t = np.abs(out - ref_out).max(), R.grad_err(d_rot, ref_rot), R.grad_err(d_trans, ref_trans)
    print("transform3d B={} N={} {} {}: forward {:.3g} abs, d_rot {:.3g}, d_trans {:.3g} rel".format(B, N, coord, setting, e_f, e_r, e_t))
    assert np.isfinite(out).all() and np.isfinite(d_rot).all() and np.isfinite(d_trans).all()
    assert e_f <= R.T3D_FWD_BAR
    assert e_r <= R.T3D_GRAD_BAR
    assert e_t <= R.T3D_GRAD_BAR


@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("coord", R.COORDS)
def test_transform3d_quaternion_norm_branches(ops, coord, setting):
    """|q|^2 - 1 in {+-5e-5, +-2e-4, +-5e-3, +-2e-2}: the forward takes the identity beyond 1e-2, the backward gives d_rot = 0 beyond
    1e-4 and still d_trans.  Off the unit sphere the reference's Ns factors are not the true gradient, so the float32 oracle is the
    reference, not autograd; both sides are one float32 evaluation of the same formulas, which the 10x bars of the test above cover."""
    inp = R.t3d_norm_inputs()
    m, s = f32_ms(setting)
    out, d_rot, d_trans = t3d_run(ops, inp, coord, setting)
    ref_out = ot3d.forward(inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
    ref_rot, ref_trans = ot3d.backward(inp["out_grad"], inp["pts"], inp["rot"], inp["trans"], inp["pose_src"], m, s, coord)
    far_f, far_b = np.abs(inp["delta"]) > 1e-2, np.abs(inp["delta"]) > 1e-4
    assert np.abs(out - ref_out).max() <= R.T3D_FWD_BAR
    # identity rotation: the output is what a delta quaternion (1, 0, 0, 0) gives
    ident = dict(inp, rot=np.tile(np.array([1, 0, 0, 0], np.float32), (len(far_f), 1)))
    assert np.abs(out[far_f] - R.t3d_reference(ident, coord, setting)[0][far_f]).max() <= R.T3D_FWD_BAR
    assert (d_rot[far_b] == 0).all()
    assert (ref_rot[~far_b] != 0).any(axis=1).all() and R.grad_err(d_rot[~far_b], ref_rot[~far_b]) <= R.T3D_GRAD_BAR
    assert (d_trans != 0).all() and R.grad_err(d_trans, ref_trans) <= R.T3D_GRAD_BAR


# ------------------------------------------------------------------------------------------------ SE(3), quaternion deltas
def se3_run(ops, tab, coord, setting):
    m, s = f32_ms(setting)
    src, tgt, se3 = dev(tab["src"]), dev(tab["tgt"]), dev(tab["se3"])
    out64 = torch.full(src.shape, 7.0, dtype=torch.float64, device=DEV)
    out = ops.se3_compose(src, se3, coord, m, s, out_f64=out64)
    rot, trans = ops.se3_delta(src, tgt, coord, m, s)
    rmat, trans_m = ops.se3_delta_matrix(src, tgt, coord, m, s)
    return dict(out=host(out), out64=host(out64), rot=host(rot), trans=host(trans), rmat=host(rmat), trans_m=host(trans_m))


@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("coord", R.COORDS)
def test_se3_compose_and_delta_on_the_table(ops, coord, setting):
    tab = R.se3_table()
    got = se3_run(ops, tab, coord, setting)
    again = se3_run(ops, tab, coord, setting)
    for k in got:                                            # a second call repeats bit for bit
        assert np.array_equal(got[k], again[k]), k
    # ---- compose
    ref_c = R.se3_compose_ref(coord, setting)
    e64, e32 = np.abs(got["out64"] - ref_c).max(), np.abs(got["out"] - ref_c).max()
    assert e64 <= (1e-6 if coord == "NAIVE" else 1e-12)
    assert e32 <= 2e-6
    assert np.array_equal(got["out"], got["out64"].astype(np.float32))
    # ---- delta
    ref = R.se3_delta_ref(coord, setting)
    q = got["rot"].astype(np.float64)
    assert (q[:, 0] >= 0).all()
    e_q = R.quat_err(q, ref["q"], free_sign_below=1e-6)
    e_R, e_t = np.abs(got["rmat"] - ref["R"]).max(), np.abs(got["trans"] - ref["t"]).max()
    assert e_q.max() <= 2e-6 and e_R <= 2e-6 and e_t <= 2e-6
    assert np.array_equal(got["trans_m"], got["trans"])
    small = tab["angle"] <= SMALL
    e_small = np.abs(q[small, 1:] - ref["q"][small, 1:]).max()
    print("se3 {} {}: compose f64 {:.3g}, f32 {:.3g}; delta quat {:.3g}, matrix {:.3g}, trans {:.3g}; vector part at angle <= 1e-3: {:.3g}"
          .format(coord, setting, e64, e32, e_q.max(), e_R, e_t, e_small))
    # tiny rotations: reference-alone 1.3e-11 plus 3e-11 of float32 output rounding of a vector part <= 5e-4; NAIVE's reference
    # rounds its residual to float32 and keeps 2e-6
    assert e_small <= (2e-6 if coord == "NAIVE" else 1e-9)
    if coord != "NAIVE" and setting == "unit":
        same = tab["angle"] == 0.0                           # src == tgt bit for bit
        assert same.sum() == len(R.AXES) and (got["trans"][same] == 0.0).all()


@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("coord", R.COORDS)
def test_se3_round_trip(ops, coord, setting):
    """se3_compose(src, se3_delta(src, tgt)) = tgt, without any oracle"""
    tab = R.se3_table()
    m, s = f32_ms(setting)
    src, tgt = dev(tab["src"]), dev(tab["tgt"])
    rot, trans = ops.se3_delta(src, tgt, coord, m, s)
    back = host(ops.se3_compose(src, torch.cat([rot, trans], dim=1).contiguous(), coord, m, s)).astype(np.float64)
    want = tab["tgt"].astype(np.float64)
    err = np.abs(back - want) / np.maximum(1.0, np.abs(want))
    print("se3 round trip {} {}: {:.3g}".format(coord, setting, err.max()))
    assert err.max() <= 2e-6


@pytest.mark.parametrize("coord", R.COORDS)
def test_se3_compose_zero_quaternion_stays_in_its_row(ops, coord):
    tab = R.se3_table()
    m, s = f32_ms("golden")
    bad = 70                                                 # in the second block
    se3 = tab["se3"].copy()
    se3[bad, :4] = 0.0
    src = dev(tab["src"])
    o64a = torch.empty(src.shape, dtype=torch.float64, device=DEV)
    o64b = torch.empty(src.shape, dtype=torch.float64, device=DEV)
    clean = host(ops.se3_compose(src, dev(tab["se3"]), coord, m, s, out_f64=o64a))
    got = host(ops.se3_compose(src, dev(se3), coord, m, s, out_f64=o64b))
    keep = np.arange(R.N_ROWS) != bad
    assert np.array_equal(got[keep], clean[keep]) and np.array_equal(host(o64b)[keep], host(o64a)[keep])
    assert not np.isfinite(got[bad, :, :3]).any() and not np.isfinite(host(o64b)[bad, :, :3]).any()
    with np.errstate(invalid="ignore", divide="ignore"):     # ... as numpy does: 0 / |0| in RT_transform
        ref = R.ose3.RT_transform(tab["src"][bad].astype(np.float64), se3[bad, :4].astype(np.float64), se3[bad, 4:].astype(np.float64),
                                  *R.ms("golden"), coord)
    assert not np.isfinite(np.asarray(ref)[:, :3]).any()


# ------------------------------------------------------------------------------------------------ SE(3), Euler deltas
@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("coord", R.COORDS)
def test_se3_euler_compose_and_delta(ops, coord, setting):
    tab = R.euler_table()
    m, s = f32_ms(setting)
    src, tgt = dev(tab["src"]), dev(tab["tgt"])
    out64 = torch.empty(src.shape, dtype=torch.float64, device=DEV)
    out = host(ops.se3_compose_euler(src, dev(tab["se3"]), coord, m, s, out_f64=out64))
    ref_c = R.se3_compose_ref(coord, setting, "euler")
    e64, e32 = np.abs(host(out64) - ref_c).max(), np.abs(out - ref_c).max()
    assert e64 <= (1e-6 if coord == "NAIVE" else 1e-12)
    assert e32 <= 2e-6
    eul, trans = ops.se3_delta_euler(src, tgt, coord, m, s)
    eul, trans = host(eul), host(trans)
    ref = R.se3_delta_ref(coord, setting, "euler")
    e_e, e_t = np.abs(eul - ref["e"]).max(), np.abs(trans - ref["t"]).max()
    print("se3 euler {} {}: compose f64 {:.3g}, f32 {:.3g}; delta angles {:.3g}, trans {:.3g}".format(coord, setting, e64, e32, e_e, e_t))
    assert e_e <= 4e-6 and e_t <= 2e-6
    lock = tab["lock"]
    assert (eul[lock, 2] == 0.0).all() and not (eul[~lock, 2] == 0.0).any()
    assert np.abs(eul[lock, :2] - ref["e"][lock, :2]).max() <= 4e-6


# ------------------------------------------------------------------------------------------------ pose_to_KT
@pytest.mark.parametrize("K", [R.K_LINEMOD, R.K_SKEW], ids=["linemod", "skew"])
def test_pose_to_KT(ops, K):
    tab = R.se3_table()
    ref, bound = R.pose_to_KT_ref(tab["src"], tab["tgt"], K)
    got = host(ops.pose_to_KT(dev(tab["src"]), dev(tab["tgt"]), K)).astype(np.float64)
    assert got.shape == (R.N_ROWS, 3, 4)
    ratio = np.abs(got - ref) / bound
    print("pose_to_KT: worst error {:.3g} of its bound".format(ratio.max()))
    assert ratio.max() <= 1.0
