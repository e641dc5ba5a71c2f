"""Reading a Gauss-Newton stage's sums back from its workspace, with no library change (tests/test_gpu_icp_terms.py,
tests/test_gpu_gn_terms.py).

Every stage's workspace starts with [state B x 16 doubles = R, t, updated, pad][partial B x 16 workgroups x 32 doubles, terms 0..28]
(GnWorkspace in csrc/twist_solve.h).  After a call with iters = n the partials hold the sums of iteration n - 1, taken at the
correction T_{n-1}, and the state holds T_n; replays are bit-identical, so runs with iters = 1, 2, 3 give T_k (the state of run k)
and the 29 sums at T_k (the partials of run k + 1).  The pad doubles may keep the workspace's fill and are not read."""
import numpy as np

N_TERMS = 29     # 21 upper-triangle entries of J J^T (row-major), 6 of J r, the count, r^2
BLOCKS, SLOT, STATE = 16, 32, 16


def split_workspace(ws, B):
    """the leading doubles of a stage's workspace (a host float64 array) -> state (B,16), partial (B,16,32)"""
    ws = np.asarray(ws, np.float64).reshape(-1)
    return ws[:STATE * B].reshape(B, STATE).copy(), ws[STATE * B:(STATE + BLOCKS * SLOT) * B].reshape(B, BLOCKS, SLOT).copy()


def block_order_sum(partial):
    """the 16 workgroup partials added in block order with plain float64 adds, as gn_solve_kernel does"""
    S = np.zeros(N_TERMS)
    for k in range(BLOCKS):
        S = S + partial[k, :N_TERMS]
    return S


def stats_of(S):
    """the stats row gn_solve_kernel writes from the sums: (float32(N), float32(sqrt(S28 / N)))"""
    N, rr = S[27], S[28]
    return np.array([np.float32(N), np.float32(np.sqrt(rr / N)) if N > 0 else np.float32(0.0)], np.float32)


def state_of(run, b=0):
    """-> R (3,3), t (3,), updated of pair b from a run's state rows"""
    st = run["state"][b]
    return st[:9].reshape(3, 3).copy(), st[9:12].copy(), st[12]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def step_in_kernel_order(S):
    """the step of gn_solve_kernel on the 29 sums S with the kernel's own operations in the kernel's own order (csrc/twist_solve.h:
    the damping, cholesky_solve6 with its running subtractions, twist_rodrigues), in Python floats, which round like the kernel's
    float64 without contraction; only sin and cos may differ from the device's by an ulp.
    -> dR (3,3), v (3,), xi (6,), or None when the kernel skips the step.  icp_reference.gn_step is the same algebra with numpy's
    dot products, whose other association moves xi by cond(A) eps: too much for undoing a step to the last bits."""
    from math import cos, sin, sqrt

    s = [float(x) for x in S[:N_TERMS]]
    if not s[27] >= 64.0:
        return None
    A = [0.0] * 36
    k = 0
    for a in range(6):
        for e in range(a, 6):
            A[6 * a + e] = A[6 * e + a] = s[k]
            k += 1
    damp = 1e-9 * (A[0] + A[7] + A[14] + A[21] + A[28] + A[35]) / 6.0
    rhs = [0.0] * 6
    for a in range(6):
        A[6 * a + a] += damp
        rhs[a] = -s[21 + a]
    L = [0.0] * 36
    for j in range(6):
        d = A[6 * j + j]
        for k in range(j):
            d -= L[6 * j + k] * L[6 * j + k]
        if not d > 0.0:
            return None
        L[6 * j + j] = sqrt(d)
        for i in range(j + 1, 6):
            v = A[6 * i + j]
            for k in range(j):
                v -= L[6 * i + k] * L[6 * j + k]
            L[6 * i + j] = v / L[6 * j + j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = rhs[i]
        for k in range(i):
            v -= L[6 * i + k] * y[k]
        y[i] = v / L[6 * i + i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[6 * k + i] * x[k]
        x[i] = v / L[6 * i + i]
    w = x[:3]
    th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Wx = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    a, bq = 1.0, 0.0
    if th >= 1e-12:
        a = sin(th) / th
        bq = (1.0 - cos(th)) / (th * th)
    Rw = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            w2 = 0.0
            for k in range(3):
                w2 += Wx[3 * i + k] * Wx[3 * k + j]
            Rw[i, j] = (1.0 if i == j else 0.0) + a * Wx[3 * i + j] + bq * w2
    return Rw, np.array(x[3:]), np.array(x)


def undo_step_exactly(dR, v, R2, t2):
    """T_1 with T_2 = [dR | v] T_1, solved in rational arithmetic on the doubles and rounded once: R_1 = dR^-1 R_2,
    t_1 = dR^-1 (t_2 - v) (the inverse, not the transpose: dR is a rotation only to rounding)"""
    from fractions import Fraction

    M = [[Fraction(float(dR[i, j])) for j in range(3)] for i in range(3)]
    cof = [[M[(j + 1) % 3][(i + 1) % 3] * M[(j + 2) % 3][(i + 2) % 3] - M[(j + 1) % 3][(i + 2) % 3] * M[(j + 2) % 3][(i + 1) % 3]
            for j in range(3)] for i in range(3)]          # the adjugate
    det = sum(M[0][j] * cof[j][0] for j in range(3))
    rhs = [[Fraction(float(R2[i, j])) for j in range(3)] + [Fraction(float(t2[i])) - Fraction(float(v[i]))] for i in range(3)]
    T1 = np.array([[float(sum(cof[i][k] * rhs[k][j] for k in range(3)) / det) for j in range(4)] for i in range(3)])
    return T1[:, :3].copy(), T1[:, 3].copy()
