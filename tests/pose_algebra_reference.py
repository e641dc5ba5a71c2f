"""References and deterministic case tables for the pose algebra of csrc/se3.hip (test-only; numpy / torch on the CPU).

Transform3D: the forward DEFINITION in torch float64 (q -> R with s = 2/|q|^2, the translation rules of T_transform, NAIVE as
Rd (Rs p + Ts) + td) and its gradient from autograd -- not a restated backward.  A second, plain numpy restatement of the formulas the
kernels evaluate (`t3d_restated`) exists only to be mutated: each named fault of T3D_FAULTS is one mistake such a kernel can make.

SE(3): oracle/se3.py on the float32-rounded inputs in float64, `quat_branch` (which of tr, M00, M11, M22 wins in mat2quat_d of
csrc/twist_solve.h) and `shepperd`, a numpy restatement of that selection.

Every table is a pure function of its seed, built once per process and returned read-only."""
import functools

import numpy as np
import torch

from oracle import se3 as ose3

COORDS = ("MODEL", "CAMERA", "CAMERA_NEW", "NAIVE")
# (T_means, T_stds): the trivial pair and the one tests/golden/se3_golden.npz carries as T_means2 / T_stds2
SETTINGS = {"unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "golden": ((0.01, -0.02, 0.03), (0.5, 2.0, 1.5))}

f32, f64 = np.float32, np.float64


def ms(setting):
    """the kernels take T_means / T_stds as float32: -> the float32 values, widened"""
    m, s = SETTINGS[setting]
    return np.asarray(m, f32).astype(f64), np.asarray(s, f32).astype(f64)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def rand_pose(rng):
    """drawn like tests/golden/make_golden.rand_pose: a uniform rotation, T = (+-0.2, +-0.15, 0.5..1.3)"""
    q = rng.normal(size=4)
    R = ose3.quat2mat(q / np.linalg.norm(q))
    t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.15, 0.15), rng.uniform(0.5, 1.3)])
    return np.concatenate([R, t[:, None]], axis=1)


def axis_angle(axis, angle):
    """Rodrigues, float64"""
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    Wx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Wx + (1.0 - np.cos(angle)) * (Wx @ Wx)


# ================================================================================================ Transform3D
T3D_SHAPES = tuple((5, n) for n in (1, 63, 64, 65, 255, 256, 257, 1000, 3000)) + ((70, 65),)
T3D_FWD_BAR = 2e-6     # absolute
T3D_GRAD_BAR = 1e-5    # of the sample's largest reference entry
NORM_DELTAS = (5e-5, -5e-5, 2e-4, -2e-4, 5e-3, -5e-3, 2e-2, -2e-2)   # |q|^2 - 1; thresholds 1e-4 (backward) and 1e-2 (forward)


def _t3d_draw(rng, B, N):
    pts = ((rng.random((B, 3, N)) - 0.5) * 0.2).astype(f32)
    rot = rng.normal(size=(B, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(f32)      # unit quaternions rounded to float32
    trans = ((rng.random((B, 3)) - 0.5) * 0.2).astype(f32)
    pose_src = np.stack([rand_pose(rng) for _ in range(B)]).astype(f32)       # every sample its own pose
    out_grad = (rng.normal(size=(B, 3, N)) / N).astype(f32)
    return dict(pts=pts, rot=rot, trans=trans, pose_src=pose_src, out_grad=out_grad)


@functools.lru_cache(maxsize=None)
def t3d_inputs(B, N):
    return _frozen(_t3d_draw(np.random.default_rng(7100 + 1000 * B + N), B, N))


@functools.lru_cache(maxsize=None)
def t3d_norm_inputs():
    """B = 8, Npts = 65; sample i has |q_i|^2 - 1 = NORM_DELTAS[i]"""
    d = _t3d_draw(np.random.default_rng(7301), len(NORM_DELTAS), 65)
    q = d["rot"].astype(f64)
    q *= np.sqrt((1.0 + np.array(NORM_DELTAS)) / (q * q).sum(1))[:, None]
    d["rot"] = q.astype(f32)
    d["delta"] = np.array(NORM_DELTAS)
    got = (d["rot"].astype(f64) ** 2).sum(1) - 1.0
    assert np.abs(got - d["delta"]).max() < 1e-6          # float32 rounding of q moves |q|^2 by ~1e-7: far from flipping a branch
    return _frozen(d)


def old_inputs():
    """the one input set of tests/test_gpu_ops.py::test_transform3d, in this module's layout (means 0, stds 1 there)"""
    from test_oracle_transform3d import _inputs

    pts, rot, trans, pose_src = _inputs()
    g = np.random.RandomState(3).randn(*pts.shape).astype(f32) / pts.shape[2]
    return dict(pts=pts, rot=rot, trans=trans, pose_src=pose_src, out_grad=g)


def _quat_to_rot(q):
    w, x, y, z = q.unbind(1)
    s = 2.0 / (q * q).sum(1)
    X, Y, Z = x * s, y * s, z * s
    rows = [1.0 - (y * Y + z * Z), x * Y - w * Z, x * Z + w * Y,
            x * Y + w * Z, 1.0 - (x * X + z * Z), y * Z - w * X,
            x * Z - w * Y, y * Z + w * X, 1.0 - (x * X + y * Y)]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def t3d_forward_def(pts, rot, trans, pose_src, T_means, T_stds, coord):
    """the operation's definition, torch float64, differentiable in rot and trans"""
    Rd = _quat_to_rot(rot)
    Rs, Ts = pose_src[:, :, :3], pose_src[:, :, 3]
    if coord == "NAIVE":
        return Rd @ (Rs @ pts + Ts[:, :, None]) + trans[:, :, None]
    R = Rs @ Rd if coord == "MODEL" else Rd @ Rs
    d = trans * T_stds + T_means
    z2 = Ts[:, 2] / torch.exp(d[:, 2])
    if coord == "CAMERA_NEW":
        x2, y2 = Ts[:, 2] * d[:, 0] + Ts[:, 0], Ts[:, 2] * d[:, 1] + Ts[:, 1]
    else:
        x2, y2 = z2 * (d[:, 0] + Ts[:, 0] / Ts[:, 2]), z2 * (d[:, 1] + Ts[:, 1] / Ts[:, 2])
    return R @ pts + torch.stack([x2, y2, z2], 1)[:, :, None]


def t3d_reference(inp, coord, setting):
    """-> out (B,3,N), d_rot (B,4), d_trans (B,3): float64 forward and autograd gradient of sum(out * out_grad) on the float32 inputs"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f64))  # noqa: E731
    m, s = ms(setting)
    rot, trans = T(inp["rot"]).requires_grad_(True), T(inp["trans"]).requires_grad_(True)
    out = t3d_forward_def(T(inp["pts"]), rot, trans, T(inp["pose_src"]), T(m), T(s), coord)
    d_rot, d_trans = torch.autograd.grad((out * T(inp["out_grad"])).sum(), (rot, trans))
    return out.detach().numpy(), d_rot.numpy(), d_trans.numpy()


@functools.lru_cache(maxsize=None)
def t3d_case_reference(B, N, coord, setting):
    """t3d_reference of t3d_inputs(B, N), computed once per process and read-only"""
    ref = t3d_reference(t3d_inputs(B, N), coord, setting)
    for a in ref:
        a.setflags(write=False)
    return ref


def grad_err(got, ref):
    """largest |got - ref| of a sample over that sample's largest |ref| entry, worst sample"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


# ---- the kernels' formulas in plain numpy float64, with one switch per planted fault
T3D_FAULTS = ("Rs_not_transposed", "pose_of_sample_0", "stds_one_in_backward", "no_xy_over_z", "tail_points_dropped")


def _restated_rot(q, thr):
    w, x, y, z = q
    Nq = w * w + x * x + y * y + z * z
    if not (-thr < Nq - 1.0 < thr):
        return np.eye(3)
    s = 2.0 / Nq
    X, Y, Z = x * s, y * s, z * s
    return np.array([[1.0 - (y * Y + z * Z), x * Y - w * Z, x * Z + w * Y], [x * Y + w * Z, 1.0 - (x * X + z * Z), y * Z - w * X],
                     [x * Z - w * Y, y * Z + w * X, 1.0 - (x * X + y * Y)]])


def t3d_restated(inp, coord, setting, fault=None):
    """-> out, d_rot, d_trans as transform3d_fwd_kernel / transform3d_bwd_kernel compute them (thresholds on |q|^2 included)"""
    assert fault is None or fault in T3D_FAULTS
    m, s = ms(setting)
    pts, rot, trans, pose, G = (np.asarray(inp[k], f64) for k in ("pts", "rot", "trans", "pose_src", "out_grad"))
    B, _, N = pts.shape
    out, d_rot, d_trans = np.zeros_like(pts), np.zeros((B, 4)), np.zeros((B, 3))
    sb = np.ones(3) if fault == "stds_one_in_backward" else s
    n_used = 256 * (N // 256) if fault == "tail_points_dropped" else N
    for b in range(B):
        ps = pose[0] if fault == "pose_of_sample_0" else pose[b]
        Rs, Ts = ps[:, :3], ps[:, 3]
        xz, yz = (0.0, 0.0) if fault == "no_xy_over_z" else (Ts[0] / Ts[2], Ts[1] / Ts[2])
        # ---- forward
        Rd = _restated_rot(rot[b], 1e-2)
        Rt = Rs @ Rd if coord == "MODEL" else Rd @ Rs
        t = trans[b] * s + m
        z2 = Ts[2] / np.exp(t[2])
        if coord == "NAIVE":
            Tt = Rd @ Ts + trans[b]
        elif coord == "CAMERA_NEW":
            Tt = np.array([Ts[2] * t[0] + Ts[0], Ts[2] * t[1] + Ts[1], z2])
        else:
            Tt = np.array([z2 * (t[0] + xz), z2 * (t[1] + yz), z2])
        out[b] = Rt @ pts[b] + Tt[:, None]
        # ---- backward: 12 sums over the points, then a few scalars
        g, p = G[b][:, :n_used], pts[b][:, :n_used]
        if coord == "NAIVE":
            p = Rs @ p + Ts[:, None]
        S, Dt = g.sum(1), g @ p.T
        if coord == "NAIVE":
            d_trans[b] = S
        elif coord == "CAMERA_NEW":
            d_trans[b] = [S[0] * (sb[0] * Ts[2]), S[1] * (sb[1] * Ts[2]), S[2] * (-sb[2] * z2)]
        else:
            share = -sb[2] * z2
            d_trans[b] = [S[0] * (sb[0] * z2), S[1] * (sb[1] * z2),
                          S[0] * (share * (t[0] + xz)) + S[1] * (share * (t[1] + yz)) + S[2] * (-sb[2] * z2)]
        RsT = Rs if fault == "Rs_not_transposed" else Rs.T
        D = Dt if coord == "NAIVE" else (RsT @ Dt if coord == "MODEL" else Dt @ RsT)
        w, x, y, z = rot[b]
        Nq = w * w + x * x + y * y + z * z
        if not (-1e-4 < Nq - 1.0 < 1e-4):
            continue
        Ns = np.sqrt(Nq)
        w_, x_, y_, z_ = rot[b] / Ns
        wd = 2.0 * (-z_ * D[0, 1] + y_ * D[0, 2] + z_ * D[1, 0] - x_ * D[1, 2] - y_ * D[2, 0] + x_ * D[2, 1])
        xd = 2.0 * (y_ * D[0, 1] + z_ * D[0, 2] + y_ * D[1, 0] - 2 * x_ * D[1, 1] - w_ * D[1, 2] + z_ * D[2, 0] + w_ * D[2, 1] - 2 * x_ * D[2, 2])
        yd = 2.0 * (-2 * y_ * D[0, 0] + x_ * D[0, 1] + w_ * D[0, 2] + x_ * D[1, 0] + z_ * D[1, 2] - w_ * D[2, 0] + z_ * D[2, 1] - 2 * y_ * D[2, 2])
        zd = 2.0 * (-2 * z_ * D[0, 0] - w_ * D[0, 1] + x_ * D[0, 2] + w_ * D[1, 0] - 2 * z_ * D[1, 1] + y_ * D[1, 2] + x_ * D[2, 0] + y_ * D[2, 1])
        share = Ns ** 3 * (w * wd + x * xd + y * yd + z * zd)
        d_rot[b] = [Ns * wd - w * share, Ns * xd - x * share, Ns * yd - y * share, Ns * zd - z * share]
    return out, d_rot, d_trans


# ================================================================================================ SE(3)
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0.2, -0.9, 0.4), (-0.7, 0.1, 0.7))
ANGLES = (0.0, 1e-7, 1e-5, 1e-3, 0.5, 2.0, 2.2, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.pi)
N_RANDOM = 64
N_ROWS = N_RANDOM + len(AXES) * len(ANGLES)          # 130: two full 64-thread blocks and a partial one


@functools.lru_cache(maxsize=None)
def se3_table():
    """src, tgt (130,3,4) float32; se3 (130,7) float32 = [raw quaternion, trans delta] for compose; angle (130,): the known angle
    between src and tgt of the built rows, nan on the random ones.  Built rows: tgt = src rotated by (axis, angle) in the model
    frame, T moved a little -- except at angle 0, where tgt IS src bit for bit (the rows that pin the exact zero translation)."""
    rng = np.random.default_rng(4711)
    src, tgt, se3, angle = [], [], [], []
    for _ in range(N_RANDOM):
        src.append(rand_pose(rng))
        tgt.append(rand_pose(rng))
        se3.append(np.concatenate([rng.normal(size=4) * rng.uniform(0.2, 3.0), rng.normal(size=3) * [0.05, 0.05, 0.2]]))
        angle.append(np.nan)
    for axis in AXES:
        for a in ANGLES:
            ps = rand_pose(rng).astype(f32).astype(f64)
            pt = ps.copy()
            if a != 0.0:
                pt[:, :3] = ps[:, :3] @ axis_angle(axis, a)
                pt[:, 3] += rng.uniform(-1.0, 1.0, size=3) * [0.02, 0.02, 0.05]
            u = np.asarray(axis, f64) / np.linalg.norm(axis)
            q = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * u]) * rng.uniform(0.2, 3.0)
            src.append(ps)
            tgt.append(pt)
            se3.append(np.concatenate([q, rng.normal(size=3) * [0.05, 0.05, 0.2]]))
            angle.append(a)
    return _frozen(dict(src=np.array(src).astype(f32), tgt=np.array(tgt).astype(f32), se3=np.array(se3).astype(f32), angle=np.array(angle)))


def quat_branch(M):
    """0..3: which of tr, M00, M11, M22 is chosen, as mat2quat_d selects"""
    M = np.asarray(M, f64)
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    if tr > M[0, 0] and tr > M[1, 1] and tr > M[2, 2]:
        return 0
    if M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
        return 1
    return 2 if M[1, 1] > M[2, 2] else 3


def shepperd(M, always_w=False):
    """mat2quat_d of csrc/twist_solve.h in numpy; always_w: the planted fault that never leaves the first branch"""
    M = np.asarray(M, f64)
    br = 0 if always_w else quat_branch(M)
    if br == 0:
        q = [1.0 + M[0, 0] + M[1, 1] + M[2, 2], M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]
    elif br == 1:
        q = [M[2, 1] - M[1, 2], 1.0 + M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[0, 2] + M[2, 0]]
    elif br == 2:
        q = [M[0, 2] - M[2, 0], M[0, 1] + M[1, 0], 1.0 - M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]]
    else:
        q = [M[1, 0] - M[0, 1], M[0, 2] + M[2, 0], M[1, 2] + M[2, 1], 1.0 - M[0, 0] - M[1, 1] + M[2, 2]]
    q = np.array(q)
    n = np.linalg.norm(q)
    return q / (-n if q[0] < 0 else n)


def _w(a):
    return np.asarray(a, f32).astype(f64)


@functools.lru_cache(maxsize=None)
def se3_delta_ref(coord, setting, table="se3"):
    """oracle.se3.calc_RT_delta per row on the widened float32 poses -> dict(R (n,3,3), q (n,4), e (n,3), t (n,3)) float64"""
    tab = se3_table() if table == "se3" else euler_table()
    m, s = ms(setting)
    R, q, e, t = [], [], [], []
    for ps, pt in zip(_w(tab["src"]), _w(tab["tgt"])):
        Rd, td = ose3.calc_RT_delta(ps, pt, m, s, coord, "MATRIX")
        Rd = np.asarray(Rd, f64)
        R.append(Rd)
        q.append(ose3.mat2quat(Rd))
        e.append(ose3.mat2euler(Rd))
        t.append(np.asarray(td, f64))
    return _frozen(dict(R=np.array(R), q=np.array(q), e=np.array(e), t=np.array(t)))


@functools.lru_cache(maxsize=None)
def se3_compose_ref(coord, setting, table="se3"):
    """oracle.se3.RT_transform per row on the widened float32 inputs -> (n,3,4) float64"""
    tab = se3_table() if table == "se3" else euler_table()
    m, s = ms(setting)
    rows = _w(tab["se3"])
    k = rows.shape[1] - 3
    out = np.array([np.asarray(ose3.RT_transform(ps, r[:k], r[k:], m, s, coord), f64) for ps, r in zip(_w(tab["src"]), rows)])
    out.setflags(write=False)
    return out


def quat_err(got, ref, free_sign_below=1e-6):
    """per row max |got - ref|; where |w_ref| < free_sign_below the better of the two global signs"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    e = np.abs(got - ref).max(1)
    free = np.abs(ref[:, 0]) < free_sign_below
    return np.where(free, np.minimum(e, np.abs(got + ref).max(1)), e)


# ---- Euler
N_EULER = 130
LOCK = ((0.3, 1, -0.7), (1.1, -1, 0.4), (0.0, 1, 0.0), (-2.9, -1, 2.5), (3.0, 1, 3.1), (-0.4, -1, -1.9), (1.57, 1, 0.01), (0.002, -1, -3.0))


@functools.lru_cache(maxsize=None)
def euler_table():
    """src, tgt (138,3,4), se3 (138,6) = [ai, aj, ak, trans delta], lock (138,) bool.
    Rows 0..129: random triples, every fifth with aj within 1e-3 of +-pi/2; tgt random on the first half and src turned by that
    triple (model frame) on the second, so the delta sees near-lock residuals too.
    Rows 130..137: src rotation = identity and tgt rotation = float32(euler2mat(ai, +-pi/2, ak)): the residual is then exact for
    every rot_coord and the lock branch is taken in float64."""
    rng = np.random.default_rng(1913)
    src, tgt, rows = [], [], []
    for i in range(N_EULER):
        e = rng.uniform(-np.pi, np.pi, size=3) * [1.0, 0.5, 1.0]
        if i % 5 == 0:
            e[1] = rng.choice([-1.0, 1.0]) * (np.pi / 2 + rng.choice([-1.0, 1.0]) * rng.uniform(1e-6, 1e-3))
        ps, pt = rand_pose(rng), rand_pose(rng)
        if i >= N_EULER // 2:
            pt[:, :3] = ps.astype(f32).astype(f64)[:, :3] @ ose3.euler2mat(*e)
        src.append(ps)
        tgt.append(pt)
        rows.append(np.concatenate([e, rng.normal(size=3) * [0.05, 0.05, 0.2]]))
    for ai, sgn, ak in LOCK:
        ps, pt = rand_pose(rng), rand_pose(rng)
        ps[:, :3] = np.eye(3)
        pt[:, :3] = ose3.euler2mat(ai, sgn * np.pi / 2, ak)
        src.append(ps)
        tgt.append(pt)
        rows.append(np.concatenate([[ai, sgn * np.pi / 2, ak], rng.normal(size=3) * [0.05, 0.05, 0.2]]))
    lock = np.arange(len(src)) >= N_EULER
    return _frozen(dict(src=np.array(src).astype(f32), tgt=np.array(tgt).astype(f32), se3=np.array(rows).astype(f32), lock=lock))


# ================================================================================================ pose_to_KT
K_LINEMOD = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
K_SKEW = np.array([[572.4114, 1.7, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def pose_to_KT_ref(src, tgt, K):
    """-> KT (n,3,4) float64 = K @ [calc_se3], and the per-entry bound 1e-6 * sum_k |K_ik| |M_kj|.  calc_se3 on the widened poses
    forms each product in float64 and rounds it to float32 once, like the kernel; the bound leaves room for three float32 roundings
    (2^-24 each: 1.8e-7 of that sum)."""
    K = _w(K)
    ref, bound = [], []
    for ps, pt in zip(_w(src), _w(tgt)):
        R, t = ose3.calc_se3(ps, pt)
        M = np.concatenate([np.asarray(R, f64), np.asarray(t, f64)[:, None]], axis=1)
        ref.append(K @ M)
        bound.append(1e-6 * (np.abs(K) @ np.abs(M)))
    return np.array(ref), np.array(bound)
