"""numpy float64 restatement of the device ICP stage (csrc/icp.hip, dim_icp_refine): projective point-to-plane ICP, model to frame.

Per pair: the source points are the depth rendered at the input pose T0 back-projected with the pair's K, the target is the observed
depth.  Every iteration moves the source points by the current correction T_delta (identity at the start), projects each one into the
observed frame (integer pixel, floor(v + 0.5)), takes the observed point there and the normal of its four neighbours, and linearises
r = n . (p - q) in the twist xi = (omega, v):  J = (p x n, n).  The 6x6 normal equations are solved by Cholesky and
T_delta <- [Rodrigues(omega) | v] . T_delta.  pose_out = T_delta . T0.
"""
import numpy as np

MIN_POINTS = 64            # fewer inliers: no update, DIM_STATUS_ICP_FEW_POINTS
STATUS_ICP_FEW_POINTS = 32
DAMPING = 1e-9             # A + DAMPING tr(A) / 6 I


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1.0 - np.cos(th)) / (th * th) * (Wx @ Wx)


def cholesky_solve(A, b):
    """-> x with A x = b, or None when A is not positive definite (a pivot <= 0)"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > 0.0:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def _camera(K):
    K = np.asarray(K, np.float64).reshape(9)
    return K[0], K[4], K[2], K[5]


def source_points(depth_rendered, K, bbox=None):
    """(N,3) back-projected pixels of depth_rendered > 0 inside bbox {min_x, max_x, min_y, max_y} (inclusive; None = whole frame)"""
    H, W = depth_rendered.shape
    fx, fy, cx, cy = _camera(K)
    x0, x1, y0, y1 = (0, W - 1, 0, H - 1) if bbox is None else (max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0),
                                                                 min(int(bbox[3]), H - 1))
    if x1 < x0 or y1 < y0:
        return np.zeros((0, 3))
    d = np.asarray(depth_rendered, np.float64)[y0:y1 + 1, x0:x1 + 1]
    ys, xs = np.nonzero(d > 0)
    z = d[ys, xs]
    xs = xs + x0
    ys = ys + y0
    return np.stack([z * (xs - cx) / fx, z * (ys - cy) / fy, z], axis=1)


def _backproject(D, u, v, fx, fy, cx, cy):
    z = D[v, u]
    return np.stack([z * (u - cx) / fx, z * (v - cy) / fy, z], axis=1), z


def normal_equations(p, depth_observed, K, max_dist, mask_observed=None):
    """one data association + linearisation for source points p (N,3) already moved by T_delta.
    -> A (6,6), g (6,), n_inliers, sum r^2"""
    H, W = depth_observed.shape
    fx, fy, cx, cy = _camera(K)
    D = np.asarray(depth_observed, np.float64)
    p = p[p[:, 2] > 0]
    u = np.floor(fx * p[:, 0] / p[:, 2] + cx + 0.5)
    v = np.floor(fy * p[:, 1] / p[:, 2] + cy + 0.5)
    ok = (u >= 1) & (u <= W - 2) & (v >= 1) & (v <= H - 2)
    p, u, v = p[ok], u[ok].astype(np.int64), v[ok].astype(np.int64)
    ok = D[v, u] > 0
    if mask_observed is not None:
        ok &= np.asarray(mask_observed, np.float64)[v, u] >= 0.5
    p, u, v = p[ok], u[ok], v[ok]
    q, zq = _backproject(D, u, v, fx, fy, cx, cy)
    nb = []
    ok = np.ones(len(p), bool)
    for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        qn, zn = _backproject(D, u + du, v + dv, fx, fy, cx, cy)
        ok &= (zn > 0) & (np.abs(zn - zq) < max_dist)
        nb.append(qn)
    n = np.cross(nb[0] - nb[1], nb[2] - nb[3])
    nn = np.sum(n * n, axis=1)
    ok &= nn > 1e-20
    p, q, n, nn = p[ok], q[ok], n[ok], nn[ok]
    n = n / np.sqrt(nn)[:, None]
    n = np.where((np.sum(n * q, axis=1) > 0)[:, None], -n, n)
    e = p - q
    ok = np.sum(e * e, axis=1) <= max_dist * max_dist
    p, n, e = p[ok], n[ok], e[ok]
    r = np.sum(n * e, axis=1)
    J = np.concatenate([np.cross(p, n), n], axis=1)
    return J.T @ J, J.T @ r, int(len(r)), float(np.sum(r * r))


def icp_refine_pair(depth_rendered, depth_observed, pose_in, K, iters, max_dist, mask_observed=None, bbox=None):
    """-> pose_out (3,4) float32, stats (iters,2) = (inliers, rms residual) before each update, status bits"""
    pose_in = np.asarray(pose_in, np.float32)
    p0 = source_points(depth_rendered, K, bbox)
    R, t = np.eye(3), np.zeros(3)
    stats = np.zeros((iters, 2))
    status, updated = 0, False
    for k in range(iters):
        A, g, N, rr = normal_equations(p0 @ R.T + t, depth_observed, K, max_dist, mask_observed)
        stats[k] = (N, np.sqrt(rr / N) if N > 0 else 0.0)
        xi = None
        if N >= MIN_POINTS:
            xi = cholesky_solve(A + DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
        if xi is None:
            status |= STATUS_ICP_FEW_POINTS
            continue
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        updated = True
    if not updated:
        return pose_in.copy(), stats, status
    T0 = pose_in.astype(np.float64)
    out = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + t)[:, None]], axis=1)
    return out.astype(np.float32), stats, status


def icp_refine(depth_rendered, depth_observed, pose_in, K, iters, max_dist, mask_observed=None, bbox=None):
    """batched: depth_* (B,H,W) or (B,1,H,W), pose_in (B,3,4), K (3,3) for all or (B,3,3) / (B,9) per pair, bbox (B,4) or None"""
    B = pose_in.shape[0]
    dr = np.asarray(depth_rendered).reshape(B, *np.asarray(depth_rendered).shape[-2:])
    do = np.asarray(depth_observed).reshape(dr.shape)
    mo = None if mask_observed is None else np.asarray(mask_observed).reshape(dr.shape)
    Ks = np.asarray(K, np.float64)
    Ks = np.tile(Ks.reshape(1, 9), (B, 1)) if Ks.size == 9 else Ks.reshape(B, 9)
    poses, stats, status = [], [], []
    for b in range(B):
        p, s, st = icp_refine_pair(dr[b], do[b], pose_in[b], Ks[b], iters, max_dist, None if mo is None else mo[b],
                                   None if bbox is None else bbox[b])
        poses.append(p)
        stats.append(s)
        status.append(st)
    return np.stack(poses), np.stack(stats), np.asarray(status, np.int32)


def add_error(pose, pose_gt, pts):
    """ADD: mean distance of the model points under the two poses"""
    pose, pose_gt = np.asarray(pose, np.float64), np.asarray(pose_gt, np.float64)
    a = pts @ pose[:, :3].T + pose[:, 3]
    b = pts @ pose_gt[:, :3].T + pose_gt[:, 3]
    return float(np.mean(np.linalg.norm(a - b, axis=1)))
