"""Float64 numpy restatement of several hypotheses per pair (csrc/hyp.hip, include/deepim_hip.h): the axis table, the expansion of a
pair's pose into N starting poses, the two scores of a rendered pose and the choice per pair.  Written from the definitions, not
from the kernels: the ZNCC uses centred sums, "constant plane" means every value of S is equal."""
import numpy as np

MIN_PIXELS = 64
STATUS_HYP_NO_SCORE = 64


def fibonacci_axes(M):
    """(M,3): z = 1 - (2k+1)/M, r = sqrt(1-z^2), phi = k pi (3 - sqrt 5), axis = (r cos phi, r sin phi, z)"""
    k = np.arange(M, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / M
    r = np.sqrt(np.clip(1.0 - z * z, 0.0, None))
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def rodrigues(axis, angle_rad):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle_rad) * Kx + (1.0 - np.cos(angle_rad)) * Kx @ Kx


def rotation_table(N, rot_deg):
    """(N,3,3): identity, then the rotation by rot_deg about each of the N-1 Fibonacci axes"""
    R = [np.eye(3)]
    if N > 1:
        R += [rodrigues(a, np.radians(rot_deg)) for a in fibonacci_axes(N - 1)]
    return np.stack(R)


def expand(table, poses):
    """table (N,3,3), poses (P,3,4) -> (P*N,3,4): [R_h R_p | t_p], sample p*N+h"""
    table, poses = np.asarray(table, np.float64), np.asarray(poses, np.float64)
    N, P = table.shape[0], poses.shape[0]
    out = np.zeros((P * N, 3, 4))
    for p in range(P):
        for h in range(N):
            out[p * N + h, :, :3] = table[h] @ poses[p, :, :3]
            out[p * N + h, :, 3] = poses[p, :, 3]
    return out


def _support(depth_rendered, bbox):
    """bool (H,W): pixels inside bbox {min_x,max_x,min_y,max_y} (inclusive, None = whole frame) with rendered depth > 0"""
    H, W = depth_rendered.shape
    S = np.zeros((H, W), dtype=bool)
    x0, x1, y0, y1 = (0, W - 1, 0, H - 1) if bbox is None else (max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0),
                                                                min(int(bbox[3]), H - 1))
    if x1 >= x0 and y1 >= y0:
        S[y0:y1 + 1, x0:x1 + 1] = True
    with np.errstate(invalid="ignore"):
        return S & (np.asarray(depth_rendered) > 0)


def score_one(mode, image_observed, image_rendered, depth_rendered, bbox=None, depth_observed=None, tau=0.02):
    """one sample: image_* (3,H,W), depth_* (H,W) -> score (float, -inf when undefined)"""
    S = _support(depth_rendered, bbox)
    if mode == "rgb":
        a = np.asarray(image_observed, np.float64).sum(0)[S]
        r = np.asarray(image_rendered, np.float64).sum(0)[S]
        if a.size < MIN_PIXELS or not (np.all(np.isfinite(a)) and np.all(np.isfinite(r))):
            return -np.inf
        if np.all(a == a[0]) or np.all(r == r[0]):
            return -np.inf
        da, dr = a - a.mean(), r - r.mean()
        return float(np.clip(np.sum(da * dr) / np.sqrt(np.sum(da * da) * np.sum(dr * dr)), -1.0, 1.0))
    if mode == "depth":
        Dr = np.asarray(depth_rendered, np.float64)[S]
        Do = np.asarray(depth_observed, np.float64)[S]
        with np.errstate(invalid="ignore"):
            ok = Do > 0
            n = int(ok.sum())
            if n < MIN_PIXELS:
                return -np.inf
            return float(np.sum(np.abs(Dr[ok] - Do[ok]) < tau) / n)
    raise ValueError(mode)


def scores(mode, image_observed, image_rendered, depth_rendered, bbox=None, depth_observed=None, tau=0.02):
    """batched: image_* (B,3,H,W), depth_* (B,1,H,W), bbox (B,4) or None -> (B,) float64"""
    B = depth_rendered.shape[0]
    return np.array([score_one(mode, None if image_observed is None else image_observed[b], None if image_rendered is None else image_rendered[b],
                               depth_rendered[b, 0], None if bbox is None else bbox[b],
                               None if depth_observed is None else depth_observed[b, 0], tau) for b in range(B)])


def select(score, N):
    """score (P*N,) -> choice (P,) int, none_finite (P,) bool: the largest finite score, ties to the smaller h, none finite: 0"""
    s = np.asarray(score, np.float64).reshape(-1, N)
    choice = np.zeros(s.shape[0], dtype=int)
    none = np.zeros(s.shape[0], dtype=bool)
    for p in range(s.shape[0]):
        best = None
        for h in range(N):
            if np.isfinite(s[p, h]) and (best is None or s[p, h] > s[p, best]):
                best = h
        none[p] = best is None
        choice[p] = 0 if best is None else best
    return choice, none


def gather(choice, N, poses_iter, status_iter=None, pose_icp=None):
    """the chosen rows: poses_iter (T,P*N,3,4) -> (T,P,3,4), status_iter (T,P*N) -> (T,P), pose_icp (P*N,3,4) -> (P,3,4)"""
    idx = np.arange(len(choice)) * N + np.asarray(choice)
    return (poses_iter[:, idx], None if status_iter is None else status_iter[:, idx], None if pose_icp is None else pose_icp[idx])
