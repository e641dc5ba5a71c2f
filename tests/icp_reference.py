"""numpy float64 restatement of the device ICP stage (csrc/icp.hip, dim_icp_refine): projective point-to-plane ICP, model to frame.

Per pair: the source points are the depth rendered at the input pose T0 back-projected with the pair's K, the target is the observed
depth.  Every iteration moves the source points by the current correction T_delta (identity at the start), projects each one into the
observed frame (integer pixel, floor(v + 0.5)), takes the observed point there and the normal of its four neighbours, and linearises
r = n . (p - q) in the twist xi = (omega, v):  J = (p x n, n).  The 6x6 normal equations are solved by Cholesky and
T_delta <- [Rodrigues(omega) | v] . T_delta.  pose_out = T_delta . T0.

point_terms is the per-point form of one linearisation; with dtype=np.float32 (and source_points, move_points, lane_sums in the same
dtype) it is the float32 model of icp_accumulate_kernel, operation by operation, for tests/test_gpu_icp_terms.py.
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


def _camera(K, dtype=np.float64):
    K = np.asarray(K, np.float64).reshape(9).astype(dtype)
    return K[0], K[4], K[2], K[5]


def camera_ok(K):
    """cam_ok of twist_solve.h, on the float32 the kernel sees: fx > 0, fy > 0 and fx, fy, cx, cy finite; else the pair has no points"""
    with np.errstate(over="ignore"):
        fx, fy, cx, cy = _camera(K, np.float32)
    return bool(fx > 0 and fy > 0 and np.all(np.isfinite([fx, fy, cx, cy])))


def clamp_bbox(bbox, H, W):
    """clamp_bbox of twist_solve.h -> x0, x1, y0, y1 (empty when x1 < x0 or y1 < y0)"""
    if bbox is None:
        return 0, W - 1, 0, H - 1
    return max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0), min(int(bbox[3]), H - 1)


def source_points(depth_rendered, K, bbox=None, dtype=np.float64, with_index=False):
    """(N,3) back-projected pixels of depth_rendered > 0 inside bbox {min_x, max_x, min_y, max_y} (inclusive; None = whole frame), none
    when the camera is not camera_ok.  with_index: also the linear index of each point inside the clamped box (row-major, the order
    in which the kernel's lanes take them)."""
    H, W = depth_rendered.shape
    x0, x1, y0, y1 = clamp_bbox(bbox, H, W)
    if x1 < x0 or y1 < y0 or not camera_ok(K):
        return (np.zeros((0, 3), dtype), np.zeros((0,), np.int64)) if with_index else np.zeros((0, 3), dtype)
    fx, fy, cx, cy = _camera(K, dtype)
    d = np.asarray(depth_rendered, dtype)[y0:y1 + 1, x0:x1 + 1]
    ys, xs = np.nonzero(d > 0)
    z = d[ys, xs]
    index = ys * (x1 - x0 + 1) + xs
    xs = (xs + x0).astype(dtype)
    ys = (ys + y0).astype(dtype)
    pts = np.stack([z * (xs - cx) / fx, z * (ys - cy) / fy, z], axis=1)
    return (pts, index) if with_index else pts


def move_points(s, R, t, dtype=np.float64):
    """R s + t in the kernel's order, ((R0 sx + R1 sy) + R2 sz) + t0, with R, t cast to float32 first as the kernel reads them"""
    R = np.asarray(R, np.float64).astype(np.float32).astype(dtype)
    t = np.asarray(t, np.float64).astype(np.float32).astype(dtype)
    s = np.asarray(s, dtype)
    return np.stack([R[i, 0] * s[:, 0] + R[i, 1] * s[:, 1] + R[i, 2] * s[:, 2] + t[i] for i in range(3)], axis=1).reshape(-1, 3)


N_TERMS = 29     # 21 upper-triangle entries of J J^T (row-major), 6 of J r, the count, r^2
LANES = 4096     # 16 workgroups of 256 lanes per pair
# planted defects of the float32 model (tests/test_icp_terms_host.py shows that the bar of tests/test_gpu_icp_terms.py catches each;
# the seventh, another pair's mask plane, is planted by the caller)
DEFECTS = ("swap_fxfy_q", "no_flip", "rot_sign", "ax_fu", "border_u", "rr_before_gate")


def _keep(ok, *arrays):
    return [a[ok] for a in arrays]


def point_terms(p, depth_observed, K, max_dist, mask_observed=None, dtype=np.float64, index=None, defect=None, margins=None):
    """one data association + linearisation for source points p (N,3) already moved by T_delta, in the expression order of
    icp_accumulate_kernel, every operation rounded to dtype.
    -> terms (n, 29): what each surviving point adds to the 29 sums; index (n,): its entry of `index` (default: its row in p).
    defect: one of DEFECTS (with rr_before_gate the points that fail the distance gate come back too, r^2 their only term).
    margins: a dict that receives how far the gate decisions were from flipping (the smallest over the points that reached each gate)."""
    assert defect is None or defect in DEFECTS, defect
    H, W = depth_observed.shape
    fx, fy, cx, cy = _camera(K, dtype)
    D = np.asarray(depth_observed, dtype).reshape(-1)
    M = None if mask_observed is None else np.asarray(mask_observed, np.float64).reshape(-1)
    p = np.asarray(p, dtype).reshape(-1, 3)
    idx = np.arange(len(p)) if index is None else np.asarray(index)
    half, one, md = dtype(0.5), dtype(1.0), dtype(max_dist)
    m = {} if margins is None else margins
    p, idx = _keep(p[:, 2] > 0, p, idx)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    ur, vr = fx * px / pz + cx + half, fy * py / pz + cy + half
    uf, vf = np.floor(ur), np.floor(vr)
    fr = np.concatenate([ur - uf, vr - vf])
    m["round_px"] = float(np.min(np.minimum(fr, 1.0 - fr), initial=np.inf))
    ok = (uf >= 1) & (uf <= (W - 1 if defect == "border_u" else W - 2)) & (vf >= 1) & (vf <= H - 2)
    px, py, pz, uf, vf, idx = _keep(ok, px, py, pz, uf, vf, idx)
    o = vf.astype(np.int64) * W + uf.astype(np.int64)
    zq = D[o]
    ok = zq > 0
    if M is not None:
        m["mask"] = float(np.min(np.abs(M[o][ok] - 0.5), initial=np.inf))
        ok &= M[o] >= 0.5
    px, py, pz, uf, vf, idx, o, zq = _keep(ok, px, py, pz, uf, vf, idx, o, zq)
    zr, zl, zd, zu = D[o + 1], D[o - 1], D[o + W], D[o - W]
    ok = np.ones(len(o), bool)
    jump = [np.inf]
    for zn in (zr, zl, zd, zu):
        ok &= (zn > 0) & (np.abs(zn - zq) < md)
        jump.append(np.min(np.abs(np.abs(zn - zq)[zn > 0] - md), initial=np.inf))
    m["jump"] = float(min(jump) / md)
    px, py, pz, uf, vf, idx, zq, zr, zl, zd, zu = _keep(ok, px, py, pz, uf, vf, idx, zq, zr, zl, zd, zu)
    qfx, qfy = (fy, fx) if defect == "swap_fxfy_q" else (fx, fy)
    qx, qy, qz = zq * (uf - cx) / qfx, zq * (vf - cy) / qfy, zq
    # central differences (q(u+1) - q(u-1)) x (q(v+1) - q(v-1))
    ax = zr * ((uf if defect == "ax_fu" else uf + one) - cx) / fx - zl * (uf - one - cx) / fx
    ay = zr * (vf - cy) / fy - zl * (vf - cy) / fy
    az = zr - zl
    bx = zd * (uf - cx) / fx - zu * (uf - cx) / fx
    by = zd * (vf + one - cy) / fy - zu * (vf - one - cy) / fy
    bz = zd - zu
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    nn = nx * nx + ny * ny + nz * nz
    m["nn"] = float(np.min(nn, initial=np.inf))
    ok = nn > dtype(1e-20)
    px, py, pz, idx, qx, qy, qz, nx, ny, nz, nn = _keep(ok, px, py, pz, idx, qx, qy, qz, nx, ny, nz, nn)
    nl = np.sqrt(nn)
    nx, ny, nz = nx / nl, ny / nl, nz / nl
    dot = nx * qx + ny * qy + nz * qz
    m["flip"] = float(np.min(np.abs(dot), initial=np.inf))
    if defect != "no_flip":
        flip = dot > 0
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
    ex, ey, ez = px - qx, py - qy, pz - qz
    ee = ex * ex + ey * ey + ez * ez
    m["dist"] = float(np.min(np.abs(np.sqrt(ee.astype(np.float64)) - float(md)), initial=np.inf) / float(md))
    inl = ee <= md * md
    r = nx * ex + ny * ey + nz * ez
    J = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
    if defect == "rot_sign":
        J[:3] = [-J[0], -J[1], -J[2]]
    cols = [J[a] * J[e] for a in range(6) for e in range(a, 6)] + [J[a] * r for a in range(6)] + [np.ones_like(r), r * r]
    terms = np.stack(cols, axis=1)
    assert terms.dtype == dtype and terms.shape == (len(r), N_TERMS)
    if defect == "rr_before_gate":
        terms[~inl, :28] = 0
        return terms, idx
    return terms[inl], idx[inl]


def lane_sums(terms, index, dtype=np.float64):
    """the 29 sums as the kernel takes them -> partial (16, 29) float64, one row per workgroup: lane index % 4096 adds its points in
    dtype in the order of their index (the grid-stride loop), then float64 across the 256 lanes of a workgroup"""
    acc = np.zeros((LANES, N_TERMS), dtype)
    index = np.asarray(index, np.int64)
    terms = np.asarray(terms, dtype)
    assert np.all(np.diff(index) > 0)
    for k in range(int(index.max(initial=-1)) // LANES + 1):
        sel = (index // LANES) == k
        lanes = index[sel] % LANES
        acc[lanes] = acc[lanes] + terms[sel]
    return acc.astype(np.float64).reshape(16, LANES // 16, N_TERMS).sum(axis=1)


def unpack_sums(S):
    """29 sums -> A (6,6), g (6,), count, sum r^2"""
    S = np.asarray(S, np.float64)
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for e in range(a, 6):
            A[a, e] = A[e, a] = S[k]
            k += 1
    return A, S[21:27].copy(), float(S[27]), float(S[28])


def normal_equations(p, depth_observed, K, max_dist, mask_observed=None):
    """one data association + linearisation for source points p (N,3) already moved by T_delta.
    -> A (6,6), g (6,), n_inliers, sum r^2"""
    terms, _ = point_terms(p, depth_observed, K, max_dist, mask_observed)
    A, g, N, rr = unpack_sums(terms.sum(axis=0))
    return A, g, int(N), rr


def gn_step(R, t, S):
    """gn_solve_kernel on the 29 sums S at the correction (R, t): -> R', t', xi; (R, t, None) when the step is skipped (fewer than
    MIN_POINTS points or a system that is not positive definite)"""
    A, g, N, _ = unpack_sums(S)
    xi = None
    if N >= MIN_POINTS:
        xi = cholesky_solve(A + DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
    if xi is None:
        return R, t, None
    dR = rodrigues(xi[:3])
    return dR @ R, dR @ t + xi[3:], xi


def icp_refine_pair(depth_rendered, depth_observed, pose_in, K, iters, max_dist, mask_observed=None, bbox=None):
    """-> pose_out (3,4) float32, stats (iters,2) = (inliers, rms residual) before each update, status bits"""
    pose_in = np.asarray(pose_in, np.float32)
    p0 = source_points(depth_rendered, K, bbox)
    R, t = np.eye(3), np.zeros(3)
    stats = np.zeros((iters, 2))
    status, updated = 0, False
    for k in range(iters):
        terms, _ = point_terms(p0 @ R.T + t, depth_observed, K, max_dist, mask_observed)
        S = terms.sum(axis=0)
        N, rr = S[27], S[28]
        stats[k] = (N, np.sqrt(rr / N) if N > 0 else 0.0)
        R, t, xi = gn_step(R, t, S)
        if xi is None:
            status |= STATUS_ICP_FEW_POINTS
            continue
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
