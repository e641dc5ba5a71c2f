"""An independent float64 statement of the cost each Gauss-Newton pose stage minimises (depth ICP, flow PnP, photometric polish,
silhouette polish), differentiated by torch autograd on the CPU -- no hand-derived Jacobian anywhere in this file.

The restatements (tests/icp_reference.py, flow_pnp_reference.py, photo_reference.py, sil_reference.py) write J with the formulas of the
kernels, so "device == restatement" cannot see a derivation that slipped in both.  Here every stage is only a function
residuals(xi) -> r at the current correction (R, t), with the pose moved by the LEFT twist xi = (omega, v):
    p' = exp([xi]^) (R p0 + t),   exp = torch.matrix_exp of the 4x4 twist,
and J = d r / d xi at xi = 0 comes from torch.autograd.functional.jacobian.  What a stage's linearisation treats as constant is
frozen at xi = 0, in numpy, before autograd sees anything: the point set (in front of the camera, inside the frame, the gates), the
IRLS weights w, and
    ICP         the associated point q and the unit normal n (flipped towards the camera):   r = n . (p' - q)
    flow PnP    the target pixel uv:                                                          r = project(p') - uv
    silhouette  the edge pixel (ex, ey) the field names at the rounded projection:            r = project(p') - (ex, ey)
    photo       the bilinear cell (floor U, floor V) and the template value a Ir + b:         r = bilinear(I_obs, U(p'), V(p')) - t
                with U = ((fx px/pz + cx) - (s - 1)/2) / s at level lvl, s = 2^lvl.
w is Huber on |r| (photo) or on ||r||_2 (PnP, silhouette) under a hard gate; PnP's warm iterations are ungated with w = 1; ICP has
w = 1.  Only the input preparation of the restatements is reused (source_points, move_points, correspondences, contour_points,
planes, gain_bias, the edge field), here and by the callers: that is not what is checked here.

Every stage function returns a dict:
    terms      (29,) the sums in the order of csrc/twist_solve.h: 21 upper-triangle entries of A = sum w J^T J (row-major), 6 of
               g = sum w J^T r, the count (points with w > 0), and term 28 as the stage defines it: the unweighted sum of r^2 over
               the counted points for ICP, PnP and the silhouette, sum w r^2 for photo
    abs_terms  (29,) the same sums over the absolute values of the per-point contributions, taken per residual row (see
               _linearise): the unit of the tests' bars
    A, g, count, s28   terms unpacked
    grad_cost  the autograd gradient at xi = 0 of the robust cost itself over the frozen set, sum rho(e) with rho(e) = e^2/2 for
               e <= h and h (e - h/2) above (sum r^2/2 for ICP and the warm PnP iterations): equal to g exactly when the weight on g
               is the IRLS weight of that cost
    margins    name -> the least distance of any point from flipping a decision (inf when no point reaches it), in the units of the
               decision: pixels, grey levels, metres
    w, r       the weights and residuals of the counted points
    frozen     the per-point constants, for the planted defects of tests/test_gn_calculus_host.py
"""
import numpy as np
import torch

import flow_pnp_reference as fr
import icp_reference as ir
import sil_reference as sr

F64 = torch.float64
N_TERMS = 29
EPS64 = float(np.finfo(np.float64).eps)
BAR = 64.0 * EPS64           # x abs_terms: a per-point term is about ten rounded operations, the sums add a few eps per level
_UPPER = [(a, e) for a in range(6) for e in range(a, 6)]


def _generators():
    G = torch.zeros((6, 4, 4), dtype=F64)
    G[0, 2, 1], G[0, 1, 2] = 1.0, -1.0        # [omega]x: omega x p
    G[1, 0, 2], G[1, 2, 0] = 1.0, -1.0
    G[2, 1, 0], G[2, 0, 1] = 1.0, -1.0
    for k in range(3):
        G[3 + k, k, 3] = 1.0
    return G


_GEN = _generators()


def move(xi, m0):
    """exp([xi]^) applied to the points m0 (N,3)"""
    T = torch.matrix_exp(torch.einsum("k,kij->ij", xi, _GEN))
    return m0 @ T[:3, :3].T + T[:3, 3]


def unpack(terms):
    """29 sums -> A (6,6), g (6,), count, term 28"""
    terms = np.asarray(terms, np.float64)
    A = np.zeros((6, 6))
    for k, (a, e) in enumerate(_UPPER):
        A[a, e] = A[e, a] = terms[k]
    return A, terms[21:27].copy(), int(terms[27]), float(terms[28])


def pack(A, g, count, s28):
    """the inverse of unpack, for the results of the restatements"""
    A = np.asarray(A, np.float64)
    return np.array([A[a, e] for a, e in _UPPER] + list(np.asarray(g, np.float64)) + [float(count), float(s28)])


def _camera(K):
    K = np.asarray(K, np.float32).reshape(9).astype(np.float64)     # the float32 the kernels read
    return K[0], K[4], K[2], K[5]


def _least(x):
    return float(np.min(x, initial=np.inf))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _project(p, cam):
    fx, fy, cx, cy = cam
    return fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy


def _huber_weights(e, huber, gate, margins):
    """e (N,) >= 0 -> keep (N,) bool (e <= gate), w of the kept points"""
    margins["huber"], margins["gate"] = _least(np.abs(e - huber)), _least(np.abs(e - gate))
    keep = e <= gate
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(e <= huber, 1.0, huber / e)
    return keep, w[keep]


def _linearise(residuals, w, huber, weighted_28, margins, frozen):
    """residuals: xi (6,) -> (N,) or (N,2) over the frozen set; w (N,) numpy; huber None: the cost is sum r^2 / 2"""
    xi0 = torch.zeros(6, dtype=F64)
    w = _t(w)
    n = int(w.shape[0])
    if n == 0:
        zero = np.zeros(N_TERMS)
        return dict(terms=zero, abs_terms=zero.copy(), A=np.zeros((6, 6)), g=np.zeros(6), count=0, s28=0.0, grad_cost=np.zeros(6),
                    margins=margins, w=np.zeros(0), r=np.zeros(0), frozen=frozen)
    r = residuals(xi0).detach()
    J = torch.autograd.functional.jacobian(residuals, xi0, vectorize=True, strategy="forward-mode")
    rows, J = r.reshape(n, -1), J.reshape(n, -1, 6)               # one or two residual rows per point
    JJ = torch.einsum("nra,nre->nae", J, J)
    Jr = torch.einsum("nra,nr->na", J, rows)
    e2 = (rows * rows).sum(dim=1)
    contrib = torch.cat([torch.stack([w * JJ[:, a, e] for a, e in _UPPER], dim=1), w[:, None] * Jr, torch.ones((n, 1), dtype=F64),
                         ((w * e2) if weighted_28 else e2)[:, None]], dim=1)
    # the unit of the bars: every product that is rounded, in absolute value.  A pixel residual has two rows, and a point's own
    # contribution J_x[a] J_x[e] + J_y[a] J_y[e] can cancel inside the point: A[2][5] is mx my (fx^2 - fy^2) / mz^3, a few per cent of
    # either product when fx is about fy, so the rounding of the two products is dozens of eps of their sum (measured on the PnP
    # frames: 430 eps of the per-point sums, 7 x the bar, between two float64 evaluations of the same formula).  Hence the absolute
    # values are taken per residual row, |w J_x[a] J_x[e]| + |w J_y[a] J_y[e]|, which for the one-row stages is the per-point value.
    Ja, ra = J.abs(), rows.abs()
    JJa, Jra = torch.einsum("nra,nre->nae", Ja, Ja), torch.einsum("nra,nr->na", Ja, ra)
    contrib_abs = torch.cat([torch.stack([w * JJa[:, a, e] for a, e in _UPPER], dim=1), w[:, None] * Jra, contrib[:, 27:]], dim=1)
    terms, abs_terms = contrib.sum(dim=0).numpy(), contrib_abs.sum(dim=0).numpy()
    # the robust cost itself, its branch frozen like the weight
    xi = xi0.clone().requires_grad_(True)
    rx = residuals(xi).reshape(n, -1)
    ex2 = (rx * rx).sum(dim=1)
    if huber is None:
        cost = 0.5 * ex2.sum()
    else:
        quad = w >= 1.0
        e = torch.sqrt(torch.where(quad, torch.ones_like(ex2), ex2))
        cost = torch.where(quad, 0.5 * ex2, huber * (e - 0.5 * huber)).sum()
    grad_cost, = torch.autograd.grad(cost, xi)
    A, g, count, s28 = unpack(terms)
    return dict(terms=terms, abs_terms=abs_terms, A=A, g=g, count=count, s28=s28, grad_cost=grad_cost.numpy(), margins=margins,
                w=w.numpy(), r=r.numpy(), frozen=frozen)


# ------------------------------------------------------------------------------------------------------------------ depth ICP
def icp(depth_rendered, depth_observed, K, R, t, max_dist, mask_observed=None, bbox=None):
    """point-to-plane ICP at the correction (R, t), which the kernel reads as float32 (icp_reference.move_points)"""
    cam = fx, fy, cx, cy = _camera(K)
    H, W = depth_observed.shape
    D = np.asarray(depth_observed, np.float64)
    m = ir.move_points(ir.source_points(depth_rendered, K, bbox), R, t)
    mg = {"pz": _least(np.abs(m[:, 2]))}
    m = m[m[:, 2] > 0]
    u, v = _project(m, cam)
    fr_ = np.concatenate([u + 0.5 - np.floor(u + 0.5), v + 0.5 - np.floor(v + 0.5)])
    mg["round"] = _least(np.minimum(fr_, 1.0 - fr_))
    ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
    ok = (ui >= 1) & (ui <= W - 2) & (vi >= 1) & (vi <= H - 2)
    m, ui, vi = m[ok], ui[ok].astype(np.int64), vi[ok].astype(np.int64)
    ok = D[vi, ui] > 0
    if mask_observed is not None:
        M = np.asarray(mask_observed, np.float64)[vi, ui]
        mg["mask"] = _least(np.abs(M[ok] - 0.5))
        ok &= M >= 0.5
    m, ui, vi = m[ok], ui[ok], vi[ok]

    def back(x, y):
        z = D[y, x]
        return np.stack([z * (x - cx) / fx, z * (y - cy) / fy, z], axis=1), z

    q, zq = back(ui, vi)
    nb, ok, jump = [], np.ones(len(m), bool), [np.inf]
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        qn, zn = back(ui + dx, vi + dy)
        ok &= (zn > 0) & (np.abs(zn - zq) < max_dist)
        jump.append(_least(np.abs(np.abs(zn - zq)[zn > 0] - max_dist)))
        nb.append(qn)
    mg["jump"] = min(jump)
    n = np.cross(nb[0] - nb[1], nb[2] - nb[3])
    nn = np.sum(n * n, axis=1)
    mg["normal"] = _least(np.sqrt(nn[ok]) - 1e-10)          # |a x b| against the root of 1e-20
    ok &= nn > 1e-20
    m, q, n, nn = m[ok], q[ok], n[ok], nn[ok]
    n = n / np.sqrt(nn)[:, None]
    dot = np.sum(n * q, axis=1)
    mg["flip"] = _least(np.abs(dot))
    n = np.where((dot > 0)[:, None], -n, n)
    dist = np.sqrt(np.sum((m - q) ** 2, axis=1))
    mg["dist"] = _least(np.abs(dist - max_dist))
    ok = np.sum((m - q) ** 2, axis=1) <= max_dist * max_dist
    m, q, n = m[ok], q[ok], n[ok]
    mt, qt, nt = _t(m), _t(q), _t(n)

    def residuals(xi):
        return (nt * (move(xi, mt) - qt)).sum(dim=1)

    return _linearise(residuals, np.ones(len(m)), None, False, mg, dict(m=m, q=q, n=n))


# ------------------------------------------------------------------------------------------------------------------ reprojection
def _pixel_stage(m, target, cam, gated, huber, gate, mg, frozen):
    """m (N,3) in front of the camera, target (N,2) the frozen pixel each one is pulled to"""
    u, v = _project(m, cam)
    e = np.hypot(u - target[:, 0], v - target[:, 1])
    if gated:
        keep, w = _huber_weights(e, huber, gate, mg)
        m, target = m[keep], target[keep]
    else:
        w = np.ones(len(m))
    mt, tt = _t(m), _t(target)

    def residuals(xi):
        p = move(xi, mt)
        pu, pv = _project(p, cam)
        return torch.stack([pu - tt[:, 0], pv - tt[:, 1]], dim=1)

    frozen.update(m=m, target=target, cam=cam)
    return _linearise(residuals, w, huber if gated else None, False, mg, frozen)


def flow_pnp(depth_rendered, flow, K, R, t, gated, huber_px, max_px, standard_rep=False, valid=None, bbox=None):
    """pose from flow at the correction (R, t); gated False: a warm iteration, every point in front of the camera with w = 1"""
    cam = _camera(K)
    p0, uv = fr.correspondences(depth_rendered, flow, np.asarray(K, np.float32), standard_rep, valid, bbox)
    m = p0 @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    mg = {"pz": _least(np.abs(m[:, 2]))}
    front = m[:, 2] > 0
    return _pixel_stage(m[front], uv[front], cam, gated, huber_px, max_px, mg, {})


def sil(depth_rendered, field, K, R, t, huber_px, max_px, bbox=None):
    """silhouette polish at the correction (R, t) against the nearest-edge field (H,W) int32"""
    cam = _camera(K)
    d = np.asarray(depth_rendered, np.float32)
    d = d.reshape(d.shape[-2:])
    H, W = d.shape
    p0, _ = sr.contour_points(d, K, bbox)
    m = p0 @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    mg = {"pz": _least(np.abs(m[:, 2]))}
    m = m[m[:, 2] > 0]
    u, v = _project(m, cam)
    fr_ = np.concatenate([u + 0.5 - np.floor(u + 0.5), v + 0.5 - np.floor(v + 0.5)])
    mg["round"] = _least(np.minimum(fr_, 1.0 - fr_))
    ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
    ok = (ui >= 0) & (ui <= W - 1) & (vi >= 0) & (vi <= H - 1)
    m, ui, vi = m[ok], ui[ok].astype(np.int64), vi[ok].astype(np.int64)
    f = np.asarray(field, np.int64)[vi, ui]
    m, f = m[f >= 0], f[f >= 0]
    edge = np.stack([f & 0xFFFF, f >> 16], axis=1).astype(np.float64)
    return _pixel_stage(m, edge, cam, True, huber_px, max_px, mg, {})


# ------------------------------------------------------------------------------------------------------------------ photo
def photo(pl, lvl, K, R, t, a, b, huber, gate):
    """photometric polish at pyramid level lvl of the planes pl (photo_reference.planes) with the template t = a Ir + b"""
    cam = fx, fy, cx, cy = _camera(K)
    s = float(2 ** lvl)
    o = (s - 1.0) / 2.0
    Io = pl["obs"][lvl].astype(np.float64)
    Hl, Wl = Io.shape
    Y, X = np.nonzero(pl["valid"][lvl])
    d = pl["depth"][lvl][Y, X].astype(np.float64)
    tv = a * pl["ren"][lvl][Y, X].astype(np.float64) + b
    p0 = np.stack([d * ((X * s + o) - cx) / fx, d * ((Y * s + o) - cy) / fy, d], axis=1)       # the pixel's centre at level 0
    m = p0 @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    mg = {"pz": _least(np.abs(m[:, 2]))}
    m, tv = m[m[:, 2] > 0], tv[m[:, 2] > 0]

    def level_pixel(p):
        u, v = _project(p, cam)
        return (u - o) / s, (v - o) / s

    U, V = level_pixel(m)
    xf, yf = np.floor(U), np.floor(V)
    fr_ = np.concatenate([U - xf, V - yf])
    mg["cell"] = _least(np.minimum(fr_, 1.0 - fr_))
    ok = (xf >= 0) & (xf < Wl - 1) & (yf >= 0) & (yf < Hl - 1)
    m, tv, xf, yf = m[ok], tv[ok], xf[ok], yf[ok]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    cell = [Io[y0, x0], Io[y0, x0 + 1], Io[y0 + 1, x0], Io[y0 + 1, x0 + 1]]

    def sample(p, xf, yf, cell, tv):
        U, V = level_pixel(p)
        ax, ay = U - xf, V - yf
        return (1.0 - ay) * ((1.0 - ax) * cell[0] + ax * cell[1]) + ay * ((1.0 - ax) * cell[2] + ax * cell[3]) - tv

    r0 = sample(m, xf, yf, cell, tv)
    keep, w = _huber_weights(np.abs(r0), huber, gate, mg)
    m, tv, xf, yf, cell = m[keep], tv[keep], xf[keep], yf[keep], [c[keep] for c in cell]
    mt, tt, xt, yt, ct = _t(m), _t(tv), _t(xf), _t(yf), [_t(c) for c in cell]

    def residuals(xi):
        return sample(move(xi, mt), xt, yt, ct, tt)

    frozen = dict(m=m, cam=cam, s=s, xf=xf, yf=yf, cell=cell, tv=tv, level_pixel=level_pixel,
                  at_identity=bool(np.array_equal(R, np.eye(3)) and not np.any(t)))
    return _linearise(residuals, w, huber, True, mg, frozen)
