"""numpy float64 restatement of the rig calibration rule (include/deepim_hip.h, "refining a rig's extrinsics with the object poses";
gn_rig_group_kernel and gn_rig_solve_kernel of csrc/twist_solve.h behind dim_icp_refine_rig), built on tests/views_reference.py.

A batch of B = G V samples, sample b = g V + v; X_v = cam_T_rig[v] is the nominal extrinsic of camera v, the same for every group.
Unknowns: a correction C_v per camera (X'_v = C_v X_v, C_0 = I for good: camera 0 is the gauge) and a rig-frame correction D_g per
object, all from the identity.  The state row of sample b, what its accumulate step linearises at, is S_b = X'_v D_g X_v^-1.  A left
perturbation exp(alpha_v) of C_v and exp(eta_g) of D_g moves sample b by the camera-frame twist alpha_v + Ad(X'_v) eta_g.

One iteration, from the 29 sums s_gv of every sample: W_gv = A_gv Ad_v, H_ee[g] = sum_v Ad_v^T W_gv, r_e[g] = -sum_v Ad_v^T g_gv,
H_aa[v] = sum_g A_gv, r_a[v] = -sum_g g_gv, coupling block (alpha_v, eta_g) = W_gv; the objects are eliminated (Schur complement),
the cameras solved by Cholesky, the objects back-substituted.  rig_step holds who takes part and what a skipped step does."""
import numpy as np

import icp_reference as ir
import views_reference as vr

STATUS_VIEWS_CALIB_HELD = 65536
FEW = ir.STATUS_ICP_FEW_POINTS
MIN_POINTS = ir.MIN_POINTS
IDENTITY = (np.eye(3), np.zeros(3))


def damped(A):
    return A + ir.DAMPING * np.trace(A) / 6.0 * np.eye(6)


def current_extrinsics(X, C, moved):
    """X'_v = C_v X_v; a camera that never moved keeps its nominal row exactly"""
    X = np.asarray(X, np.float64)
    return np.stack([vr.mul(vr.mat(*C[v]), X[v]) if moved[v] else X[v] for v in range(len(X))])


def participants(sums):
    """from the counts alone: sums (G,V,29) -> active (G,) bool, free (V,) bool (free[0] is always False)"""
    G, V = sums.shape[:2]
    active = np.zeros(G, bool)
    for g in range(G):
        N = 0.0
        for v in range(V):
            N += sums[g, v, 27]
        active[g] = N >= MIN_POINTS
    free = np.zeros(V, bool)
    for v in range(1, V):
        shared = 0.0
        for g in range(G):
            if active[g] and sums[g, 0, 27] >= MIN_POINTS:
                shared += sums[g, v, 27]
        free[v] = shared >= MIN_POINTS
    return active, free


def blocks(sums, Xc, active, free):
    """the blocks of the system at the current extrinsics Xc -> dict: fl (free views), gl (active groups), H_ee {g: damped (6,6)},
    r_e {g}, W {(g, v)}, H_aa {v: damped}, r_a {v}"""
    G, V = sums.shape[:2]
    fl, gl = [v for v in range(V) if free[v]], [g for g in range(G) if active[g]]
    Ad = [vr.adjoint(Xc[v]) for v in range(V)]
    H_ee, r_e, W = {}, {}, {}
    for g in gl:
        A, gs, _, _ = vr.fuse(sums[g], Xc)
        H_ee[g], r_e[g] = damped(A), -gs
        for v in fl:
            W[g, v] = ir.unpack_sums(sums[g, v])[0] @ Ad[v]
    H_aa, r_a = {}, {}
    for v in fl:
        A, gs = np.zeros((6, 6)), np.zeros(6)
        for g in gl:
            Av, gv, _, _ = ir.unpack_sums(sums[g, v])
            A, gs = A + Av, gs + gv
        H_aa[v], r_a[v] = damped(A), -gs
    return dict(fl=fl, gl=gl, H_ee=H_ee, r_e=r_e, W=W, H_aa=H_aa, r_a=r_a)


def dense_system(bk):
    """the full system over (alpha of the free views, eta of the active groups) -> H, r"""
    fl, gl = bk["fl"], bk["gl"]
    F, n = len(fl), 6 * (len(fl) + len(gl))
    H, r = np.zeros((n, n)), np.zeros(n)
    for i, v in enumerate(fl):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6], r[6 * i:6 * i + 6] = bk["H_aa"][v], bk["r_a"][v]
    for j, g in enumerate(gl):
        o = 6 * (F + j)
        H[o:o + 6, o:o + 6], r[o:o + 6] = bk["H_ee"][g], bk["r_e"][g]
        for i, v in enumerate(fl):
            H[6 * i:6 * i + 6, o:o + 6] = bk["W"][g, v]
            H[o:o + 6, 6 * i:6 * i + 6] = bk["W"][g, v].T
    return H, r


def dense_solve(bk):
    """-> alpha {v}, eta {g} by one Cholesky of the full system, or None"""
    H, r = dense_system(bk)
    x = ir.cholesky_solve(H, r)
    if x is None:
        return None
    F = len(bk["fl"])
    return ({v: x[6 * i:6 * i + 6] for i, v in enumerate(bk["fl"])}, {g: x[6 * (F + j):6 * (F + j) + 6] for j, g in enumerate(bk["gl"])})


def schur_solve(bk):
    """-> alpha {v}, eta {g} with the objects eliminated, or None when a pivot is not > 0.  Needs a free view."""
    fl, gl = bk["fl"], bk["gl"]
    F = len(fl)
    Y, z = {}, {}
    for g in gl:                                                          # H_ee^-1 W_gv^T, column by column, and H_ee^-1 r_e
        z[g] = ir.cholesky_solve(bk["H_ee"][g], bk["r_e"][g])
        if z[g] is None:
            return None
        for v in fl:
            Y[g, v] = np.stack([ir.cholesky_solve(bk["H_ee"][g], bk["W"][g, v][k]) for k in range(6)], axis=1)
    S, rs = np.zeros((6 * F, 6 * F)), np.zeros(6 * F)
    for i, v in enumerate(fl):
        t = np.zeros(6)
        for g in gl:
            t = t + bk["W"][g, v] @ z[g]
        rs[6 * i:6 * i + 6] = bk["r_a"][v] - t
        for j, w in enumerate(fl):
            T = np.zeros((6, 6))
            for g in gl:
                T = T + bk["W"][g, v] @ Y[g, w]
            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = (bk["H_aa"][v] if v == w else 0.0) - T
    x = ir.cholesky_solve(S, rs)
    if x is None:
        return None
    alpha = {v: x[6 * i:6 * i + 6] for i, v in enumerate(fl)}
    eta = {}
    for g in gl:
        rhs = bk["r_e"][g]
        for v in fl:
            rhs = rhs - bk["W"][g, v].T @ alpha[v]
        eta[g] = ir.cholesky_solve(bk["H_ee"][g], rhs)
    return alpha, eta


def apply_twist(T, xi):
    dR = ir.rodrigues(xi[:3])
    return dR @ T[0], dR @ T[1] + xi[3:]


def rig_step(sums, X, C, D, moved, solve=schur_solve):
    """one iteration.  sums (G,V,29), X (V,3,4) nominal, C [(R,t)] x V, D [(R,t)] x G, moved (V,) -> dict: C, D, moved (V,), stepped
    (G,) = the groups that stepped in THIS iteration, bits (G V,) to OR into the status, active, free, blocks"""
    sums = np.asarray(sums, np.float64)
    G, V = sums.shape[:2]
    active, free = participants(sums)
    bits = np.zeros(G * V, np.int64)
    for g in range(G):
        if not active[g]:
            bits[g * V:(g + 1) * V] |= FEW
    for v in range(1, V):
        if not free[v]:
            bits[v::V] |= STATUS_VIEWS_CALIB_HELD
    bk = blocks(sums, current_extrinsics(X, C, moved), active, free)
    C, D, moved, stepped = list(C), list(D), np.array(moved, bool), np.zeros(G, bool)
    if not bk["fl"]:                                                      # the joint step of every active group, each on its own
        for g in bk["gl"]:
            xi = ir.cholesky_solve(bk["H_ee"][g], bk["r_e"][g])
            if xi is None:
                bits[g * V:(g + 1) * V] |= FEW
                continue
            D[g], stepped[g] = apply_twist(D[g], xi), True
    else:
        sol = solve(bk)
        if sol is None:
            bits |= FEW
        else:
            for v in bk["fl"]:
                C[v], moved[v] = apply_twist(C[v], sol[0][v]), True
            for g in bk["gl"]:
                D[g], stepped[g] = apply_twist(D[g], sol[1][g]), True
    return dict(C=C, D=D, moved=moved, stepped=stepped, bits=bits, active=active, free=free, blocks=bk)


def state_row(Xc_v, D_g, X_v):
    """S_b = X'_v D_g X_v^-1 -> (R, t)"""
    return vr.rt(vr.mul(Xc_v, vr.mul(vr.mat(*D_g), vr.inverse(X_v))))


def rig_refine(sample_sums, cam_T_rig, G, iters, pose_in, pose_rig_in, solve=schur_solve):
    """sample_sums(g, v, R_s, t_s) -> the 29 sums of sample g V + v at its state row.  cam_T_rig (V,3,4), float32 on the device (a float64 one is taken as it is).
    -> dict: pose (B,3,4) f32, pose_rig (G,3,4) f32, cam_T_rig (V,3,4) f32, C, D, states, stats (B,iters,2), stats_group (G,iters,2),
    stats_view (V,iters,2), status (B,), moved (V,), stepped (G,) = ever, steps = every rig_step's dict"""
    X32 = np.asarray(cam_T_rig, np.float32)
    V, X = len(X32), np.asarray(cam_T_rig, np.float64)
    B = G * V
    pose_in, pose_rig_in = np.asarray(pose_in, np.float32), np.asarray(pose_rig_in, np.float32)
    C, D, moved, stepped = [IDENTITY] * V, [IDENTITY] * G, np.zeros(V, bool), np.zeros(G, bool)
    states = [IDENTITY] * B
    stats, stats_group, stats_view = (np.zeros((B, iters, 2), np.float32), np.zeros((G, iters, 2), np.float32),
                                      np.zeros((V, iters, 2), np.float32))
    status, steps = np.zeros(B, np.int64), []
    for it in range(iters):
        sums = np.stack([np.stack([sample_sums(g, v, *states[g * V + v]) for v in range(V)]) for g in range(G)])
        for g in range(G):
            N = rr = 0.0
            for v in range(V):
                stats[g * V + v, it] = vr.group_stats(sums[g, v, 27], sums[g, v, 28])
                N, rr = N + sums[g, v, 27], rr + sums[g, v, 28]
            stats_group[g, it] = vr.group_stats(N, rr)
        for v in range(V):
            N = rr = 0.0
            for g in range(G):
                N, rr = N + sums[g, v, 27], rr + sums[g, v, 28]
            stats_view[v, it] = vr.group_stats(N, rr)
        step = rig_step(sums, X, C, D, moved, solve)
        C, D, moved = step["C"], step["D"], step["moved"]
        stepped, status = stepped | step["stepped"], status | step["bits"]
        Xc = current_extrinsics(X, C, moved)
        states = [state_row(Xc[b % V], D[b // V], X[b % V]) for b in range(B)]
        steps.append(step)
    pose = np.stack([vr.mul(vr.mat(*states[b]), pose_in[b]).astype(np.float32) if stepped[b // V] else pose_in[b] for b in range(B)])
    pose_rig = np.stack([vr.mul(vr.mat(*D[g]), pose_rig_in[g]).astype(np.float32) if stepped[g] else pose_rig_in[g] for g in range(G)])
    Xc = current_extrinsics(X, C, moved)
    cam = np.stack([Xc[v].astype(np.float32) if moved[v] else X32[v] for v in range(V)])
    return dict(pose=pose, pose_rig=pose_rig, cam_T_rig=cam, C=C, D=D, states=states, stats=stats, stats_group=stats_group,
                stats_view=stats_view, status=status, moved=moved, stepped=stepped, steps=steps)


# ------------------------------------------------------------------------------------------------------------------ a problem with fixed correspondences
class PlaneProblem(object):
    """point-to-plane with fixed correspondences: G objects of n points with unit normals, V cameras whose nominal extrinsics are off
    (camera 0 is exact), object poses off as well.  Sample b's source points are pose_in[b] m = X_v P_g m, its targets X*_v P*_g m
    with the normals turned along; r = n . (S_b s - q), J = (p x n, n).  The exact answer: X'_v = X*_v, D_g P_g = P*_g."""

    def __init__(self, G=3, V=3, n=200, seed=0, angle=np.deg2rad(0.5), shift=5e-3):
        rng = np.random.default_rng(seed)
        self.G, self.V = G, V
        self.m = rng.uniform(-0.1, 0.1, (G, n, 3))
        nrm = rng.normal(size=(G, n, 3))
        self.nrm = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
        self.X_true = np.stack([vr.random_rigid(rng) for _ in range(V)])
        self.P_true = np.stack([vr.random_rigid(rng, shift=0.2) + [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1.0]] for _ in range(G)])

        def off(T):
            w = rng.normal(size=3)
            return vr.mul(vr.mat(ir.rodrigues(angle * w / np.linalg.norm(w)), rng.normal(size=3) * shift / np.sqrt(3)), T)

        self.X = np.stack([self.X_true[0]] + [off(self.X_true[v]) for v in range(1, V)])
        self.P = np.stack([off(self.P_true[g]) for g in range(G)])
        self.pose_in = vr.views_from_rig(self.P, np.tile(self.X, (G, 1, 1)), V)   # all float64: the answer is reachable exactly

    def sums(self, g, v, R, t):
        def move(T, p):
            return p @ T[:, :3].T + T[:, 3]
        s = move(self.pose_in[g * self.V + v], self.m[g])
        target = vr.mul(self.X_true[v], self.P_true[g])
        q, n = move(target, self.m[g]), self.nrm[g] @ target[:, :3].T
        p = s @ R.T + t
        r = np.sum(n * (p - q), axis=1)
        J = np.concatenate([np.cross(p, n), n], axis=1)
        return vr.pack_sums(J.T @ J, J.T @ r, len(r), float(r @ r))
