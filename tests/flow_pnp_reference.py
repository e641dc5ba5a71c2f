"""numpy float64 restatement of the device pose-from-flow stage (csrc/flow_pnp.hip, dim_flow_pnp): the reference's flow2se3
(lib/pair_matching/flow2se3.py:13-56) with cv2.solvePnPRansac replaced by a deterministic robust Gauss-Newton of fixed length.

Per pair: every pixel of the rendered depth (inside the render's bbox, depth > 0, finite flow, valid >= 0.5 at the SOURCE pixel) is
back-projected with the pair's K to p and paired with the target pixel (u, v) = (x, y) + flow.  T = [R | t] starts at the identity;
every iteration takes m = R p + t, the pixel residual r = (fx m_x/m_z + cx - u, fy m_y/m_z + cy - v), a weight (1 in the first
`warm` iterations, then Huber under a hard gate) and the Jacobian in the left twist xi = (omega, v) with dm = omega x m + v, solves
the damped 6x6 normal equations by Cholesky and sets T <- [Rodrigues(omega) | v] . T.  pose_out = T . pose_src.
"""
import numpy as np

from icp_reference import cholesky_solve, rodrigues
from oracle.se3 import mat2quat

MIN_POINTS = 64                 # fewer weighted points: no update, DIM_STATUS_FLOW_PNP_FEW_POINTS
STATUS_FLOW_PNP_FEW_POINTS = 128
DAMPING = 1e-9                  # A + DAMPING tr(A) / 6 I


def correspondences(depth_rendered, flow, K, standard_rep=False, valid=None, bbox=None):
    """-> p (N,3) back-projected source pixels, uv (N,2) their target pixels; flow (2,H,W) in (dy,dx) unless standard_rep"""
    H, W = depth_rendered.shape
    K = np.asarray(K, np.float64).reshape(9)
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    none = np.zeros((0, 3)), np.zeros((0, 2))
    if not (fx > 0 and fy > 0 and np.all(np.isfinite([fx, fy, cx, cy]))):
        return none
    x0, x1, y0, y1 = (0, W - 1, 0, H - 1) if bbox is None else (max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0),
                                                                 min(int(bbox[3]), H - 1))
    if x1 < x0 or y1 < y0:
        return none
    d = np.asarray(depth_rendered, np.float64)
    f = np.asarray(flow, np.float64)
    fu, fv = (f[0], f[1]) if standard_rep else (f[1], f[0])
    ok = np.zeros((H, W), bool)
    ok[y0:y1 + 1, x0:x1 + 1] = True
    ok &= (d > 0) & np.isfinite(fu) & np.isfinite(fv)
    if valid is not None:
        ok &= np.asarray(valid, np.float64) >= 0.5        # at the source pixel, as flow2se3 indexes mask_image
    ys, xs = np.nonzero(ok)
    u, v = xs + fu[ys, xs], ys + fv[ys, xs]
    keep = (u >= -0.5) & (u <= W - 0.5) & (v >= -0.5) & (v <= H - 0.5)
    xs, ys, u, v = xs[keep], ys[keep], u[keep], v[keep]
    z = d[ys, xs]
    return np.stack([z * (xs - cx) / fx, z * (ys - cy) / fy, z], axis=1), np.stack([u, v], axis=1)


def normal_equations(m, uv, K, gated, huber_px, max_px):
    """one linearisation for the moved points m (N,3) -> A (6,6), g (6,), points with w > 0, sum of e^2 over them"""
    K = np.asarray(K, np.float64).reshape(9)
    fx, fy, cx, cy = K[0], K[4], K[2], K[5]
    front = m[:, 2] > 0
    m, uv = m[front], uv[front]
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    r = np.stack([fx * mx / mz + cx - uv[:, 0], fy * my / mz + cy - uv[:, 1]], axis=1)
    e = np.sqrt(np.sum(r * r, axis=1))
    w = np.ones(len(e))
    if gated:
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(e > max_px, 0.0, np.where(e <= huber_px, 1.0, huber_px / e))
    ax, bx, ay, by = fx / mz, -fx * mx / (mz * mz), fy / mz, -fy * my / (mz * mz)
    zero = np.zeros(len(e))
    Jx = np.stack([bx * my, ax * mz - bx * mx, -ax * my, ax, zero, bx], axis=1)
    Jy = np.stack([by * my - ay * mz, -by * mx, ay * mx, zero, ay, by], axis=1)
    A = (Jx * w[:, None]).T @ Jx + (Jy * w[:, None]).T @ Jy
    g = Jx.T @ (w * r[:, 0]) + Jy.T @ (w * r[:, 1])
    used = w > 0
    return A, g, int(np.sum(used)), float(np.sum(e[used] ** 2))


def flow_pnp_pair(depth_rendered, flow, pose_src, K, iters, warm=2, huber_px=2.0, max_px=8.0, standard_rep=False, valid=None, bbox=None):
    """-> pose_out (3,4) float32, se3_q (7,) float32 = [quat, t] of T, stats (iters,2) = (points with w > 0, rms e) before each
    update, status bits"""
    pose_src = np.asarray(pose_src, np.float32)
    p, uv = correspondences(depth_rendered, flow, K, standard_rep, valid, bbox)
    R, t = np.eye(3), np.zeros(3)
    stats = np.zeros((iters, 2))
    status, updated = 0, False
    for k in range(iters):
        A, g, N, ee = normal_equations(p @ R.T + t, uv, K, k >= warm, huber_px, max_px)
        stats[k] = (N, np.sqrt(ee / N) if N > 0 else 0.0)
        xi = None
        if N >= MIN_POINTS:
            xi = cholesky_solve(A + DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
        if xi is None:
            status |= STATUS_FLOW_PNP_FEW_POINTS
            continue
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        updated = True
    if not updated:
        return pose_src.copy(), np.array([1, 0, 0, 0, 0, 0, 0], np.float32), stats, status
    T0 = pose_src.astype(np.float64)
    out = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + t)[:, None]], axis=1)
    return out.astype(np.float32), np.concatenate([mat2quat(R), t]).astype(np.float32), stats, status


def flow_pnp(depth_rendered, flow, pose_src, K, iters, warm=2, huber_px=2.0, max_px=8.0, standard_rep=False, valid=None, bbox=None):
    """batched: depth_rendered (B,H,W) or (B,1,H,W), flow (B,2,H,W), pose_src (B,3,4), K (3,3) for all or (B,3,3) / (B,9) per pair,
    valid like the depth or None, bbox (B,4) or None -> pose_out (B,3,4), se3_q (B,7), stats (B,iters,2), status (B,) int32"""
    B = pose_src.shape[0]
    dr = np.asarray(depth_rendered).reshape(B, *np.asarray(depth_rendered).shape[-2:])
    va = None if valid is None else np.asarray(valid).reshape(dr.shape)
    Ks = np.asarray(K, np.float64)
    Ks = np.tile(Ks.reshape(1, 9), (B, 1)) if Ks.size == 9 else Ks.reshape(B, 9)
    rows = [flow_pnp_pair(dr[b], flow[b], pose_src[b], Ks[b], iters, warm, huber_px, max_px, standard_rep, None if va is None else va[b],
                          None if bbox is None else bbox[b]) for b in range(B)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            np.asarray([r[3] for r in rows], np.int32))


def transform_error(R, t, R_true, t_true):
    """-> (rotation angle of R R_true^T in radians, from its sine and cosine; |t - t_true|)"""
    M = np.asarray(R, np.float64) @ np.asarray(R_true, np.float64).T
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.arctan2(s, (np.trace(M) - 1.0) / 2.0)), float(np.linalg.norm(np.asarray(t, np.float64) - np.asarray(t_true, np.float64)))
