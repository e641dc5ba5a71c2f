"""numpy restatement of the silhouette pose polish (csrc/sil.hip), written from the text of include/deepim_hip.h: dim_sil_edge_field in
integers (a brute-force lexicographic argmin over all edge pixels) and dim_sil_refine in float64.

Field: a pixel is foreground when m >= 0.5 (a NaN is background); an edge pixel is a foreground pixel with a background 4-neighbour
inside the frame; field[y, x] = (ey << 16) | ex of the edge pixel that minimises (dx^2 + dy^2, ex, ey) among those with
dx^2 + dy^2 <= radius^2, else -1.
Refine: the contour pixels of the rendered depth (depth > 0, inside the clipped box, a 4-neighbour inside the frame without depth)
are back-projected, moved by T = [R | t] (from the identity), projected and rounded to a pixel; the field there names the edge pixel
they are pulled to: r = (u - ex, v - ey), Huber weight under a hard gate, Jacobian in the left twist, damped normal equations,
Cholesky, T <- [Rodrigues(omega) | v] T.  pose_out = T pose_in.
"""
import numpy as np

from icp_reference import DAMPING, add_error, cholesky_solve, rodrigues  # noqa: F401  (add_error: for the tests)

MIN_POINTS = 64                  # fewer weighted points: no update, DIM_STATUS_SIL_FEW_POINTS
STATUS_SIL_FEW_POINTS = 2048
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the field
def boundary(fg):
    """fg (H,W) bool -> the foreground pixels with a background 4-neighbour inside the frame"""
    bg = ~fg
    near = np.zeros_like(fg)
    near[:, 1:] |= bg[:, :-1]
    near[:, :-1] |= bg[:, 1:]
    near[1:, :] |= bg[:-1, :]
    near[:-1, :] |= bg[1:, :]
    return fg & near


def edge_pixels(mask):
    """mask (H,W) float -> (H,W) bool"""
    with np.errstate(invalid="ignore"):
        return boundary(np.asarray(mask, f32) >= f32(0.5))


def edge_field_pair(mask, radius, chunk_rows=16):
    """(H,W) mask -> (H,W) int32.  Every pixel against every edge pixel; pixels farther than `radius` rows or columns from the box
    of all edge pixels cannot have one within the radius and are left at -1 without the comparison."""
    edge = edge_pixels(mask)
    H, W = edge.shape
    out = np.full((H, W), -1, np.int32)
    ey, ex = (a.astype(np.int64) for a in np.nonzero(edge))
    if len(ex) == 0:
        return out
    r = int(radius)
    y_lo, y_hi = max(int(ey.min()) - r, 0), min(int(ey.max()) + r, H - 1)
    x_lo, x_hi = max(int(ex.min()) - r, 0), min(int(ex.max()) + r, W - 1)
    xs = np.arange(x_lo, x_hi + 1, dtype=np.int64)
    for y0 in range(y_lo, y_hi + 1, chunk_rows):
        ys = np.arange(y0, min(y0 + chunk_rows, y_hi + 1), dtype=np.int64)
        sel = np.abs(ey[None, :] - ys[:, None]).min(axis=0) <= r     # the edge pixels that can matter to these rows
        if not sel.any():
            continue
        cy, cx = ey[sel], ex[sel]
        d2 = (cy[None, None, :] - ys[:, None, None]) ** 2 + (cx[None, None, :] - xs[None, :, None]) ** 2
        key = (d2 << 32) | (cx << 16)[None, None, :] | cy[None, None, :]          # (d^2, ex, ey), lexicographic
        k = key.argmin(axis=2)
        best = np.take_along_axis(d2, k[..., None], axis=2)[..., 0]
        val = ((cy[k] << 16) | cx[k]).astype(np.int32)
        out[ys[0]:ys[-1] + 1, x_lo:x_hi + 1] = np.where(best <= r * r, val, -1)
    return out


def edge_field(mask, radius):
    """(B,1,H,W) or (B,H,W) -> (B,H,W) int32"""
    m = np.asarray(mask)
    m = m.reshape(m.shape[0], *m.shape[-2:])
    return np.stack([edge_field_pair(p, radius) for p in m])


# ------------------------------------------------------------------------------------------------------------------ the refinement
def _camera(K):
    K = np.asarray(K, f32).reshape(9).astype(np.float64)
    return K[0], K[4], K[2], K[5]


def camera_ok(K):
    fx, fy, cx, cy = _camera(K)
    return bool(fx > 0 and fy > 0 and np.all(np.isfinite([fx, fy, cx, cy])))


def clamp_bbox(bbox, H, W):
    """{min_x, max_x, min_y, max_y} clamped to the frame; None = the frame"""
    if bbox is None:
        return 0, W - 1, 0, H - 1
    return max(int(bbox[0]), 0), min(int(bbox[1]), W - 1), max(int(bbox[2]), 0), min(int(bbox[3]), H - 1)


def contour_points(depth, K, bbox=None):
    """-> p0 (N,3) float64, the back-projected contour pixels of the rendered depth (H,W), and their pixels (N,2) = (x, y)"""
    d = np.asarray(depth, f32)
    H, W = d.shape
    none = np.zeros((0, 3)), np.zeros((0, 2), np.int64)
    if not camera_ok(K):
        return none
    x0, x1, y0, y1 = clamp_bbox(bbox, H, W)
    if x1 < x0 or y1 < y0:
        return none
    with np.errstate(invalid="ignore"):
        on = boundary(d > 0)
    inside = np.zeros((H, W), bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    ys, xs = np.nonzero(on & inside)
    fx, fy, cx, cy = _camera(K)
    z = d[ys, xs].astype(np.float64)
    return np.stack([z * (xs - cx) / fx, z * (ys - cy) / fy, z], axis=1), np.stack([xs, ys], axis=1)


def normal_equations(m, field, K, huber_px, max_px):
    """one linearisation for the moved points m (N,3) against field (H,W) -> A (6,6), g (6,), points with w > 0, sum of e^2 over
    them, and the margins of the three decisions: the least distance of u + 0.5 / v + 0.5 from an integer, of e from huber_px and of
    e from max_px over the points that reach the decision (inf when none does)"""
    fx, fy, cx, cy = _camera(K)
    H, W = field.shape
    m = m[m[:, 2] > 0]
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    u, v = fx * mx / mz + cx, fy * my / mz + cy
    margin = {"round": np.inf, "huber": np.inf, "gate": np.inf}
    if len(u):
        margin["round"] = float(min(np.abs(u + 0.5 - np.round(u + 0.5)).min(), np.abs(v + 0.5 - np.round(v + 0.5)).min()))
    xi, yi = np.floor(u + 0.5), np.floor(v + 0.5)
    keep = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
    m, u, v, xi, yi = m[keep], u[keep], v[keep], xi[keep].astype(np.int64), yi[keep].astype(np.int64)
    f = field[yi, xi].astype(np.int64)
    keep = f >= 0
    m, u, v, f = m[keep], u[keep], v[keep], f[keep]
    r = np.stack([u - (f & 0xFFFF), v - (f >> 16)], axis=1)
    e = np.sqrt(np.sum(r * r, axis=1))
    if len(e):
        margin["huber"], margin["gate"] = float(np.abs(e - huber_px).min()), float(np.abs(e - max_px).min())
    keep = e <= max_px
    m, r, e = m[keep], r[keep], e[keep]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(e <= huber_px, 1.0, huber_px / e)
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    ax, bx, ay, by = fx / mz, -fx * mx / (mz * mz), fy / mz, -fy * my / (mz * mz)
    zero = np.zeros(len(e))
    Jx = np.stack([bx * my, ax * mz - bx * mx, -ax * my, ax, zero, bx], axis=1)
    Jy = np.stack([by * my - ay * mz, -by * mx, ay * mx, zero, ay, by], axis=1)
    A = (Jx * w[:, None]).T @ Jx + (Jy * w[:, None]).T @ Jy
    g = Jx.T @ (w * r[:, 0]) + Jy.T @ (w * r[:, 1])
    return A, g, int(len(e)), float(np.sum(e * e)), margin


def sil_refine_pair(depth_rendered, field, pose_in, K, iters, huber_px, max_px, bbox=None):
    """-> pose_out (3,4) float32, stats (iters,2) = (points with w > 0, rms e in pixels) before each update, status bits, and
    extra = {"points": contour points, "margin": the least margin of each decision over all iterations}"""
    pose_in = np.asarray(pose_in, f32)
    d = np.asarray(depth_rendered, f32)
    d = d.reshape(d.shape[-2:])
    field = np.asarray(field, np.int32)
    p0, _ = contour_points(d, K, bbox)
    R, t = np.eye(3), np.zeros(3)
    stats = np.zeros((iters, 2))
    status, updated = 0, False
    worst = {"round": np.inf, "huber": np.inf, "gate": np.inf}
    for k in range(iters):
        A, g, N, ee, margin = normal_equations(p0 @ R.T + t, field, K, huber_px, max_px)
        worst = {key: min(worst[key], margin[key]) for key in worst}
        stats[k] = (N, np.sqrt(ee / N) if N > 0 else 0.0)
        xi = None
        if N >= MIN_POINTS:
            xi = cholesky_solve(A + DAMPING * np.trace(A) / 6.0 * np.eye(6), -g)
        if xi is None:
            status |= STATUS_SIL_FEW_POINTS
            continue
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        updated = True
    extra = {"points": len(p0), "margin": worst}
    if not updated:
        return pose_in.copy(), stats, status, extra
    T0 = pose_in.astype(np.float64)
    out = np.concatenate([R @ T0[:, :3], (R @ T0[:, 3] + t)[:, None]], axis=1)
    return out.astype(f32), stats, status, extra


def sil_refine(depth_rendered, field, pose_in, K, iters, huber_px, max_px, bbox=None, with_extra=False):
    """batched: depth (B,1,H,W) or (B,H,W), field (B,H,W), pose_in (B,3,4), K (3,3) for all or (B,3,3) / (B,9) per pair, bbox (B,4) or
    None -> pose_out (B,3,4) float32, stats (B,iters,2), status (B,) int32 [, per-pair extras]"""
    B = pose_in.shape[0]
    Ks = np.asarray(K, f32)
    Ks = np.tile(Ks.reshape(1, 9), (B, 1)) if Ks.size == 9 else Ks.reshape(B, 9)
    res = [sil_refine_pair(depth_rendered[b], field[b], pose_in[b], Ks[b], iters, huber_px, max_px, None if bbox is None else bbox[b])
           for b in range(B)]
    out = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.asarray([r[2] for r in res], np.int32))
    return out + ([r[3] for r in res],) if with_extra else out
