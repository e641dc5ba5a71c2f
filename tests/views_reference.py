"""numpy float64 restatement of the device rules for one object seen by several calibrated cameras (include/deepim_hip.h, "one object
from several calibrated cameras"; csrc/views.hip, gn_solve_views_kernel of csrc/twist_solve.h).

A batch of B = G V samples holds G groups with V views, sample b = g V + v.  cam_T_rig[b] = X_b = [R_b | t_b], p_cam = X_b p_rig; a
group has one pose T_g in the rig frame and X_b T_g in the camera of sample b.  X^-1 = [R^T | -R^T t].  Twists are ordered (omega, v).

The joint Gauss-Newton stages keep the stage's own accumulate step (icp_reference / sil_reference / photo_reference normal_equations,
evaluated at each view's state row) and replace the solve: joint_refine drives any of them through a callable."""
import numpy as np

import icp_reference as ir

STATUS_VIEWS_NO_CONSENSUS = 32768
MIN_POINTS = ir.MIN_POINTS
MAX_VIEWS = 16


# ------------------------------------------------------------------------------------------------------------------ rigid 3x4 algebra
def rt(T):
    T = np.asarray(T, np.float64)
    return T[:, :3], T[:, 3]


def mat(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def mul(A, B):
    (Ra, ta), (Rb, tb) = rt(A), rt(B)
    return mat(Ra @ Rb, Ra @ tb + ta)


def inverse(X):
    R, t = rt(X)
    return mat(R.T, -(R.T @ t))


# ------------------------------------------------------------------------------------------------------------------ rules 1 and 2
def views_from_rig(pose_rig, cam_T_rig, V):
    """rule 1 -> (B,3,4) float64, X_b T_g BEFORE the one rounding to float32"""
    B = len(cam_T_rig)
    return np.stack([mul(cam_T_rig[b], pose_rig[b // V]) for b in range(B)])


def consensus(score, status, fatal_mask, pose, cam_T_rig, V):
    """rule 2 -> choice (G,) int, pose_rig (G,3,4) float64, pose_views (B,3,4) float64 (the chosen row: pose[c] itself), bits (B,) int =
    what is OR-ed into status_out"""
    score, pose = np.asarray(score, np.float32), np.asarray(pose)
    B = len(pose)
    G = B // V
    status = np.zeros(B, np.int64) if status is None else np.asarray(status, np.int64)
    choice, pose_rig, pose_views, bits = np.zeros(G, np.int64), np.zeros((G, 3, 4)), np.zeros((B, 3, 4)), np.zeros(B, np.int64)
    for g in range(G):
        c, best = -1, None
        for v in range(V):
            b = g * V + v
            if not np.isfinite(score[b]) or (status[b] & fatal_mask) != 0:
                continue
            if c < 0 or score[b] > best:
                c, best = v, score[b]
        choice[g] = c
        if c < 0:
            bits[g * V:(g + 1) * V] = STATUS_VIEWS_NO_CONSENSUS
            c = 0
        bc = g * V + c
        pose_rig[g] = mul(inverse(cam_T_rig[bc]), pose[bc])
        for v in range(V):
            b = g * V + v
            pose_views[b] = pose[bc].astype(np.float64) if v == c else mul(cam_T_rig[b], pose_rig[g])
    return choice, pose_rig, pose_views, bits


# ------------------------------------------------------------------------------------------------------------------ rule 3: the joint solve
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint(X):
    """Ad = [[R, 0], [[t]x R, R]]: a rig-frame twist (omega, v) seen in the camera X = [R | t]"""
    R, t = rt(X)
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = R
    Ad[3:, :3] = skew(t) @ R
    return Ad


def pack_sums(A, g, N, rr):
    """a stage's normal_equations result -> the 29 sums (21 upper-triangle entries row-major, 6 of g, count, sum r^2)"""
    A = np.asarray(A, np.float64)
    return np.concatenate([[A[a, e] for a in range(6) for e in range(a, 6)], np.asarray(g, np.float64), [float(N), float(rr)]])


def fuse(sums, X):
    """sums (V,29) of the views in order, X (V,3,4) -> A (6,6), g (6,), N, rr of the group, summed in ascending v"""
    A, g, N, rr = np.zeros((6, 6)), np.zeros(6), 0.0, 0.0
    for S, Xv in zip(sums, X):
        Av, gv, Nv, rrv = ir.unpack_sums(S)
        Ad = adjoint(Xv)
        A = A + Ad.T @ (Av @ Ad)
        g = g + Ad.T @ gv
        N += Nv
        rr += rrv
    return A, g, N, rr


def group_stats(N, rr):
    return np.array([np.float32(N), np.float32(np.sqrt(rr / N)) if N > 0 else np.float32(0.0)], np.float32)


def views_step(R, t, sums, X):
    """one joint step at the rig correction D = (R, t) -> R', t', xi; (R, t, None) when skipped (the GROUP has fewer than MIN_POINTS
    points, or the fused system is not positive definite)"""
    A, g, N, _ = fuse(sums, X)
    xi = None
    if N >= MIN_POINTS:
        xi = ir.cholesky_solve(A + ir.DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
    if xi is None:
        return R, t, None
    dR = ir.rodrigues(xi[:3])
    return dR @ R, dR @ t + xi[3:], xi


def conjugate(X, R, t):
    """the state row of a view: X D X^-1 -> (R_s, t_s)"""
    return rt(mul(X, mul(mat(R, t), inverse(X))))


def joint_refine(view_sums, X, iters, pose_in, pose_rig_in):
    """one group.  view_sums(v, R_s, t_s) -> the 29 sums of view v at its state row (identity at iteration 0, as gn_load_pose).
    -> dict: pose (V,3,4) f32, pose_rig (3,4) f32, D = (R, t), states [(R_s, t_s)], stats (V,iters,2), stats_group (iters,2), failed
    (whether any step was skipped), stepped"""
    V = len(X)
    X = np.asarray(X, np.float64)
    R, t, stepped, failed = np.eye(3), np.zeros(3), False, False
    states = [(np.eye(3), np.zeros(3)) for _ in range(V)]
    stats, stats_group = np.zeros((V, iters, 2), np.float32), np.zeros((iters, 2), np.float32)
    for it in range(iters):
        sums = np.stack([view_sums(v, *states[v]) for v in range(V)])
        for v in range(V):
            stats[v, it] = group_stats(sums[v, 27], sums[v, 28])
        _, _, N, rr = fuse(sums, X)
        stats_group[it] = group_stats(N, rr)
        R, t, xi = views_step(R, t, sums, X)
        stepped, failed = stepped or xi is not None, failed or xi is None
        states = [conjugate(X[v], R, t) for v in range(V)]
    pose_in, pose_rig_in = np.asarray(pose_in, np.float32), np.asarray(pose_rig_in, np.float32)
    if not stepped:
        pose, pose_rig = pose_in.copy(), pose_rig_in.copy()
    else:
        pose = np.stack([mul(mat(*states[v]), pose_in[v]) for v in range(V)]).astype(np.float32)
        pose_rig = mul(mat(R, t), pose_rig_in).astype(np.float32)
    return dict(pose=pose, pose_rig=pose_rig, D=(R, t), states=states, stats=stats, stats_group=stats_group, failed=failed, stepped=stepped)


# ------------------------------------------------------------------------------------------------------------------ helpers for the tests
def random_rigid(rng, angle=1.0, shift=0.5):
    """a general rigid transform (3,4) float64"""
    return mat(ir.rodrigues(rng.uniform(-angle, angle, 3)), rng.uniform(-shift, shift, 3))


def ulp_close(got, want):
    """got (float32) within one float32 ulp of the float64 `want`, per entry"""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.dtype == np.float32
    return np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))
