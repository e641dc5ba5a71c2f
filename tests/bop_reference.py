"""An independent float64 restatement of the BOP symmetry rule and of the two symmetry-aware pose errors, for the tests only (the
product does not import it): plain loops over the symmetries, every product and sum spelled out -- no matrix product, so no BLAS
kernel decides the order of a sum.

    symmetry set   the identity and the discrete symmetries (outer) times the n = ceil(pi / step) rotations by 2 pi i / n of every
                   continuous symmetry (inner); a product applies the discrete transformation first
    mssd           min over S of max over x of |(R_e x + t_e) - (R_g (S_R x + S_t) + t_g)|
    mspd           the same on the projections K (R p + t) divided by their third row
"""
import math

import numpy as np


def _axis_rotation(axis, angle):
    ax, ay, az = (float(v) for v in axis)
    n = math.sqrt(ax * ax + ay * ay + az * az)
    ax, ay, az = ax / n, ay / n, az / n
    c, s = math.cos(angle), math.sin(angle)
    C = 1.0 - c
    return np.array([[c + ax * ax * C, ax * ay * C - az * s, ax * az * C + ay * s],
                     [ay * ax * C + az * s, c + ay * ay * C, ay * az * C - ax * s],
                     [az * ax * C - ay * s, az * ay * C + ax * s, c + az * az * C]], dtype=np.float64)


def _compose(A, B):
    """4x4 product A . B by loops"""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = sum(A[i, k] * B[k, j] for k in range(4))
    return out


def symmetry_set(model_info, step):
    disc = [np.eye(4)]
    for s in model_info.get("symmetries_discrete", []):
        disc.append(np.array([float(v) for v in s], dtype=np.float64).reshape(4, 4))
    cont = []
    for s in model_info.get("symmetries_continuous", []):
        n = int(math.ceil(math.pi / step))
        off = np.array([float(v) for v in s["offset"]])
        for i in range(n):
            M = np.eye(4)
            if i > 0:
                R = _axis_rotation(s["axis"], 2.0 * math.pi * i / n)
                M[:3, :3] = R
                for r in range(3):   # x -> R (x - off) + off
                    M[r, 3] = off[r] - (R[r, 0] * off[0] + R[r, 1] * off[1] + R[r, 2] * off[2])
            cont.append(M)
    if not cont:
        cont = [np.eye(4)]
    return np.stack([_compose(c, d)[:3] for d in disc for c in cont])


def _move(P, x, y, z):
    """[R | t] applied to the columns x, y, z: ((R0 x + R1 y) + R2 z) + t per row"""
    return tuple(((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))


def _project(K, x, y, z):
    a = (K[0, 0] * x + K[0, 1] * y) + K[0, 2] * z
    b = (K[1, 0] * x + K[1, 1] * y) + K[1, 2] * z
    c = (K[2, 0] * x + K[2, 1] * y) + K[2, 2] * z
    return a / c, b / c


def per_symmetry(pose_est, pose_gt, K, pts, syms):
    """-> (S,2): per symmetry the largest 3-D distance and the largest pixel distance over the points"""
    pose_est, pose_gt, K = (np.asarray(a, dtype=np.float64) for a in (pose_est, pose_gt, K))
    pts = np.asarray(pts, dtype=np.float64)
    x, y, z = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
    ex, ey, ez = _move(pose_est, x, y, z)
    ue, ve = _project(K, ex, ey, ez)
    out = np.zeros((len(syms), 2))
    for k, S in enumerate(np.asarray(syms, dtype=np.float64)):
        sx, sy, sz = _move(S, x, y, z)
        gx, gy, gz = _move(pose_gt, sx, sy, sz)
        ug, vg = _project(K, gx, gy, gz)
        dx, dy, dz, du, dv = ex - gx, ey - gy, ez - gz, ue - ug, ve - vg
        out[k, 0] = np.max(np.sqrt((dx * dx + dy * dy) + dz * dz))
        out[k, 1] = np.max(np.sqrt(du * du + dv * dv))
    return out


def mssd_mspd(pose_est, pose_gt, K, pts, syms):
    """-> ((mssd, mspd), (argmin of each: the first index that attains it), the (S,2) table)"""
    table = per_symmetry(pose_est, pose_gt, K, pts, syms)
    best = (int(np.argmin(table[:, 0])), int(np.argmin(table[:, 1])))
    return (float(table[best[0], 0]), float(table[best[1], 1])), best, table


def margin(table):
    """per error: (second smallest - smallest) / smallest over the symmetries (inf for a set of one)"""
    out = []
    for k in range(2):
        v = np.sort(table[:, k])
        out.append(float("inf") if len(v) < 2 else float((v[1] - v[0]) / v[0]))
    return out
