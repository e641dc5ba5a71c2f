"""numpy restatement of the photometric pose polish (csrc/photo.hip, dim_photo_refine): a dense direct image alignment between the
render at the loop's last pose and the observed image.  The planes (gray, pyramids, validity) are float32 and meant to be bit for bit
what the device builds; everything after them is float64.

Per pair: gray planes g = (c0 + c1) + c2 of the two mean-subtracted images; 2x2-mean pyramids of the observed gray, the rendered gray,
the rendered depth and a template-valid flag (level 0: depth > 0 inside the box; level l: all four children valid); one gain and bias
from the level-0 valid pixels, t = a Ir + b; then, from the coarsest level down, `iters` Gauss-Newton iterations per level on
r = I_obs(project(T_delta p0)) - t with a Huber weight under a hard gate, in the left twist xi = (omega, v).  pose_out = T_delta pose_in.
"""
import numpy as np

from icp_reference import DAMPING, add_error, cholesky_solve, rodrigues  # noqa: F401  (add_error: for the tests)

MIN_POINTS = 64                  # fewer weighted points (or level-0 template pixels): no update, DIM_STATUS_PHOTO_FEW_POINTS
STATUS_PHOTO_FEW_POINTS = 1024
MAX_LEVELS = 5
f32 = np.float32


def gray(image):
    """(3,H,W) float32 -> (H,W) float32, (c0 + c1) + c2"""
    im = np.asarray(image, f32)
    return ((im[0] + im[1]) + im[2]).astype(f32)


def level_sizes(H, W, levels):
    out = [(int(H), int(W))]
    for _ in range(1, levels):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def half(plane):
    """the 2x2 mean ((a + b) + (c + d)) * 0.25 in float32, a, b on the upper row; a leftover row or column is dropped"""
    p = np.asarray(plane, f32)
    h, w = p.shape[0] // 2, p.shape[1] // 2
    a, b = p[0:2 * h:2, 0:2 * w:2], p[0:2 * h:2, 1:2 * w:2]
    c, d = p[1:2 * h:2, 0:2 * w:2], p[1:2 * h:2, 1:2 * w:2]
    return (((a + b) + (c + d)) * f32(0.25)).astype(f32)


def half_valid(flag):
    p = np.asarray(flag, bool)
    h, w = p.shape[0] // 2, p.shape[1] // 2
    return p[0:2 * h:2, 0:2 * w:2] & p[0:2 * h:2, 1:2 * w:2] & p[1:2 * h:2, 0:2 * w:2] & p[1:2 * h:2, 1:2 * w:2]


def pyramid(plane, levels, step=half):
    out = [plane]
    for _ in range(1, levels):
        out.append(step(out[-1]))
    return out


def clamp_bbox(bbox, H, W):
    """{min_x, max_x, min_y, max_y} clamped to the frame; None = the frame"""
    if bbox is None:
        return 0, W - 1, 0, H - 1
    return max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0), min(int(bbox[3]), H - 1)


def template_valid(depth, bbox=None):
    """level 0 of the template-valid flag: depth > 0 inside the clamped box"""
    d = np.asarray(depth, f32)
    H, W = d.shape
    x0, x1, y0, y1 = clamp_bbox(bbox, H, W)
    inside = np.zeros((H, W), bool)
    if x1 >= x0 and y1 >= y0:
        inside[y0:y1 + 1, x0:x1 + 1] = True
    return (d > 0) & inside


def planes(image_observed, image_rendered, depth_rendered, bbox, levels):
    """-> dict of per-level lists: obs, ren (float32 gray), depth (float32), valid (bool)"""
    d = np.asarray(depth_rendered, f32).reshape(np.asarray(depth_rendered).shape[-2:])
    return {"obs": pyramid(gray(image_observed), levels), "ren": pyramid(gray(image_rendered), levels), "depth": pyramid(d, levels),
            "valid": pyramid(template_valid(d, bbox), levels, half_valid)}


def gain_sums(pl):
    """float64 (n, sum Ir, sum Ir^2, sum Io, sum Io^2) over the level-0 valid pixels"""
    v = pl["valid"][0]
    ir, io = pl["ren"][0][v].astype(np.float64), pl["obs"][0][v].astype(np.float64)
    return np.array([float(v.sum()), ir.sum(), (ir * ir).sum(), io.sum(), (io * io).sum()])


def gain_bias(sums, gain=True):
    """-> (a, b, ok): t = a Ir + b.  Not ok (the pair takes no step): n < MIN_POINTS or a variance that is not a finite number > 0"""
    n, sr, srr, so, soo = (float(x) for x in sums)
    if not n >= MIN_POINTS:
        return 1.0, 0.0, False
    mr, mo = sr / n, so / n
    vr, vo = srr / n - mr * mr, soo / n - mo * mo
    if not (vr > 0.0 and vo > 0.0 and np.isfinite(vr) and np.isfinite(vo)):
        return 1.0, 0.0, False
    if not gain:
        return 1.0, 0.0, True
    a = float(np.sqrt(vo / vr))
    return a, mo - a * mr, True


def _camera(K):
    K = np.asarray(K, f32).reshape(9).astype(np.float64)
    return K[0], K[4], K[2], K[5]


def camera_ok(K):
    fx, fy, cx, cy = _camera(K)
    return bool(fx > 0 and fy > 0 and np.all(np.isfinite([fx, fy, cx, cy])))


def normal_equations(pl, lvl, K, R, t, a, b, huber, gate):
    """one linearisation at pyramid level lvl with the correction (R, t) -> A (6,6), g (6,), points with w > 0, sum of w r^2"""
    fx, fy, cx, cy = _camera(K)
    s = float(2 ** lvl)
    o = (s - 1.0) / 2.0
    Io = pl["obs"][lvl].astype(np.float64)
    Hl, Wl = Io.shape
    Y, X = np.nonzero(pl["valid"][lvl])
    d = pl["depth"][lvl][Y, X].astype(np.float64)
    tv = a * pl["ren"][lvl][Y, X].astype(np.float64) + b
    xc, yc = X * s + o, Y * s + o
    p0 = np.stack([d * (xc - cx) / fx, d * (yc - cy) / fy, d], axis=1)
    p = p0 @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    keep = p[:, 2] > 0
    p, tv = p[keep], tv[keep]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    U = ((fx * px / pz + cx) - o) / s
    V = ((fy * py / pz + cy) - o) / s
    x0f, y0f = np.floor(U), np.floor(V)
    keep = (x0f >= 0) & (x0f < Wl - 1) & (y0f >= 0) & (y0f < Hl - 1)
    p, tv, U, V, x0f, y0f = p[keep], tv[keep], U[keep], V[keep], x0f[keep], y0f[keep]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    ax, ay = U - x0f, V - y0f
    i00, i01, i10, i11 = Io[y0, x0], Io[y0, x0 + 1], Io[y0 + 1, x0], Io[y0 + 1, x0 + 1]
    val = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11)
    gx = ((1.0 - ay) * (i01 - i00) + ay * (i11 - i10)) / s
    gy = ((1.0 - ax) * (i10 - i00) + ax * (i11 - i01)) / s
    r = val - tv
    e = np.abs(r)
    keep = e <= gate            # a NaN residual is dropped too
    w = np.where(e <= huber, 1.0, huber / np.where(e > 0, e, 1.0))[keep]
    p, r, gx, gy = p[keep], r[keep], gx[keep], gy[keep]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    gp = np.stack([gx * (fx / pz), gy * (fy / pz), -(gx * fx * px + gy * fy * py) / (pz * pz)], axis=1)
    J = np.concatenate([np.cross(p, gp), gp], axis=1)
    Jw = J * w[:, None]
    return Jw.T @ J, Jw.T @ r, int(len(r)), float(np.sum(w * r * r))


def photo_refine_pair(image_observed, image_rendered, depth_rendered, pose_in, K, levels, iters, huber, gate, gain=True, bbox=None):
    """-> pose_out (3,4) float32, stats (levels*iters, 2) = (points with w > 0, sqrt(sum w r^2 / points)) before each update, status,
    and the planes and gain sums the device is compared against"""
    pose_in = np.asarray(pose_in, f32)
    pl = planes(image_observed, image_rendered, depth_rendered, bbox, levels)
    sums = gain_sums(pl)
    a, b, ok = gain_bias(sums, gain)
    ok = ok and camera_ok(K)
    R, t = np.eye(3), np.zeros(3)
    stats = np.zeros((levels * iters, 2))
    status, updated, k = 0, False, 0
    for lvl in range(levels - 1, -1, -1):
        for _ in range(iters):
            A, g, N, wrr = normal_equations(pl, lvl, K, R, t, a, b, huber, gate) if ok else (np.zeros((6, 6)), np.zeros(6), 0, 0.0)
            stats[k] = (N, np.sqrt(wrr / N) if N > 0 else 0.0)
            k += 1
            xi = None
            if N >= MIN_POINTS:
                xi = cholesky_solve(A + DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
            if xi is None:
                status |= STATUS_PHOTO_FEW_POINTS
                continue
            dR = rodrigues(xi[:3])
            R, t = dR @ R, dR @ t + xi[3:]
            updated = True
    extra = {"planes": pl, "sums": sums, "gain": (a, b, ok)}
    if not updated:
        return pose_in.copy(), stats, status, extra
    T0 = pose_in.astype(np.float64)
    out = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + t)[:, None]], axis=1)
    return out.astype(f32), stats, status, extra


def photo_refine(image_observed, image_rendered, depth_rendered, pose_in, K, levels, iters, huber, gate, gain=True, bbox=None,
                 with_extra=False):
    """batched: images (B,3,H,W), depth (B,1,H,W) or (B,H,W), pose_in (B,3,4), K (3,3) for all or (B,3,3) / (B,9) per pair, bbox (B,4)
    or None -> pose_out (B,3,4) float32, stats (B, levels*iters, 2), status (B,) int32 [, per-pair extras]"""
    B = pose_in.shape[0]
    Ks = np.asarray(K, f32)
    Ks = np.tile(Ks.reshape(1, 9), (B, 1)) if Ks.size == 9 else Ks.reshape(B, 9)
    res = [photo_refine_pair(image_observed[b], image_rendered[b], depth_rendered[b], pose_in[b], Ks[b], levels, iters, huber, gate, gain,
                             None if bbox is None else bbox[b]) for b in range(B)]
    out = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.asarray([r[2] for r in res], np.int32))
    return out + ([r[3] for r in res],) if with_extra else out
