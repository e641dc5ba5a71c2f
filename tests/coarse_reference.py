"""Float64 numpy restatement of the coarse stage (csrc/coarse.hip, deepim/core/coarse.py), written from the stage's contract in
include/deepim_hip.h, not from the kernels: the viewpoint grid, the box fit, the top-k, and the seeded cases the tests share.

Samples are pair-major: sample b = p * M + m.  The box fit only uses elementwise products, sums, two divisions and min / max, in the
order the header states, so the device result equals it bit for bit (min / max do not depend on the order of the points)."""
import numpy as np

STATUS_BAD_CLASS = 4
STATUS_HYP_NO_SCORE = 64
STATUS_COARSE_BAD_BOX = 512

LINEMOD_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ the grid
def rotation_grid(n_views, n_inplane):
    """(M,3,3), m = v * n_inplane + j: R = Rz(2 pi j / n_inplane) R_view(v); rows of R_view: x_c = normalise(up x z_c), y_c = z_c x x_c,
    z_c = -d with d the v-th direction of the Fibonacci sphere and up = (0,0,1), or (0,1,0) when |d_z| > 0.999"""
    out = []
    golden = np.pi * (3.0 - np.sqrt(5.0))
    for v in range(n_views):
        z = 1.0 - (2.0 * v + 1.0) / n_views
        r = np.sqrt(max(0.0, 1.0 - z * z))
        d = np.array([r * np.cos(v * golden), r * np.sin(v * golden), z])
        up = np.array([0.0, 1.0, 0.0]) if abs(d[2]) > 0.999 else np.array([0.0, 0.0, 1.0])
        zc = -d
        xc = np.cross(up, zc)
        xc = xc / np.sqrt(np.sum(xc * xc))
        yc = np.cross(zc, xc)
        view = np.array([xc, yc, zc])
        for j in range(n_inplane):
            a = 2.0 * np.pi * j / n_inplane
            c, s = np.cos(a), np.sin(a)
            out.append(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).dot(view))
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------------ the box fit
def project(pts, R, t, K):
    """(u, v, c) of every point under [R | t]: ((R0 x + R1 y) + R2 z) + t, then K row by row and two divisions"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    X = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
    Y = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
    Z = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
    a = (K[0, 0] * X + K[0, 1] * Y) + K[0, 2] * Z
    b = (K[1, 0] * X + K[1, 1] * Y) + K[1, 2] * Z
    c = (K[2, 0] * X + K[2, 1] * Y) + K[2, 2] * Z
    with np.errstate(all="ignore"):
        return a / c, b / c, c


def exact_box(pts, R, t, K):
    """{x0, x1, y0, y1}: the extents of the projected points, the box a perfect detector would give"""
    u, v, _ = project(pts, R, t, K)
    return np.array([u.min(), u.max(), v.min(), v.max()])


def int_box(box):
    """the exact box rounded outward to whole pixels: the extents of the inclusive int box that covers it"""
    x0, x1, y0, y1 = box
    return np.array([np.floor(x0 + 0.5) - 0.5, np.ceil(x1 - 0.5) + 0.5, np.floor(y0 + 0.5) - 0.5, np.ceil(y1 - 0.5) + 0.5])


def box_valid(box):
    x0, x1, y0, y1 = [float(v) for v in box]
    return bool(np.all(np.isfinite([x0, x1, y0, y1])) and x1 > x0 and y1 > y0)


def box_fit(pts, R, box, K, iters, z_init):
    """-> (t (3,), ok).  ok False: the fallback (0, 0, z_init) -- a bad box, no points, a point behind the camera or a non-finite s"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    fall = np.array([0.0, 0.0, float(z_init)])
    x0, x1, y0, y1 = [float(v) for v in box]
    if not box_valid(box) or len(pts) == 0:
        return fall, False
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    bw, bh, cu, cv = x1 - x0, y1 - y0, 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    with np.errstate(all="ignore"):
        tx, ty, tz = (cu - cx) * z_init / fx, (cv - cy) * z_init / fy, float(z_init)
        for _ in range(iters):
            u, v, c = project(pts, R, (tx, ty, tz), K)
            if not np.all(c > 0.0):
                return fall, False
            umin, umax, vmin, vmax = u.min(), u.max(), v.min(), v.max()
            s = 0.5 * ((umax - umin) / bw + (vmax - vmin) / bh)
            if not np.isfinite(s):
                return fall, False
            tzn = tz * s
            tx = tx * s + (cu - 0.5 * (umin + umax)) * tzn / fx
            ty = ty * s + (cv - 0.5 * (vmin + vmax)) * tzn / fy
            tz = tzn
    return np.array([tx, ty, tz]), True


def pose_from_box(points, table_off, class_index, rot_table, boxes, K, iters, z_init, K_per_sample=None):
    """the entry: rot_table (M,9) float32 and boxes (P,4) float32 as the device reads them -> (pose (P*M,3,4) float64, status (P*M,)
    int32); the float32 output is pose.astype(float32)"""
    P, M = len(class_index), len(rot_table)
    n_classes = len(table_off) - 1
    rot = np.asarray(rot_table, dtype=np.float32).astype(np.float64).reshape(M, 3, 3)
    boxes = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    pose = np.zeros((P * M, 3, 4))
    status = np.zeros((P * M,), np.int32)
    for p in range(P):
        Kp = np.asarray(K if K_per_sample is None else K_per_sample[p], dtype=np.float64).reshape(3, 3)
        c = int(class_index[p])
        bad_class = c < 0 or c >= n_classes
        pts = np.zeros((0, 3)) if bad_class else points[table_off[c]:table_off[c + 1]]
        for m in range(M):
            if bad_class:   # the fallback row; the box is still judged
                t, ok = np.array([0.0, 0.0, float(z_init)]), box_valid(boxes[p])
                status[p * M + m] |= STATUS_BAD_CLASS
            else:
                t, ok = box_fit(pts, rot[m], boxes[p], Kp, iters, z_init)
            if not ok:
                status[p * M + m] |= STATUS_COARSE_BAD_BOX
            pose[p * M + m, :, :3] = rot[m]
            pose[p * M + m, :, 3] = t
    return pose, status


# ------------------------------------------------------------------------------------------------------------------ the top-k
def topk(score, M, k, status_in=None, reject_mask=0):
    """-> (idx (P,k), filler (P,k) bool).  Per pair the k largest finite scores, descending, ties to the smaller m; a candidate whose
    status has a bit of reject_mask is skipped.  Fewer than k: the other slots repeat slot 0 and are fillers; none: all candidate 0"""
    score = np.asarray(score, dtype=np.float64).reshape(-1, M)
    P = score.shape[0]
    st = np.zeros((P, M), np.int64) if status_in is None else np.asarray(status_in).reshape(P, M)
    idx = np.zeros((P, k), np.int32)
    filler = np.zeros((P, k), bool)
    for p in range(P):
        cand = [m for m in range(M) if np.isfinite(score[p, m]) and not (int(st[p, m]) & reject_mask)]
        cand.sort(key=lambda m: (-score[p, m], m))
        for j in range(k):
            if j < len(cand):
                idx[p, j] = cand[j]
            else:
                idx[p, j] = cand[0] if cand else 0
                filler[p, j] = True
    return idx, filler


def topk_outputs(score, M, k, poses, status_in=None, reject_mask=0):
    """everything dim_hyp_topk writes: (idx (P,k), score_out (P,k), poses_out (P,k,3,4), status_out (P,k))"""
    idx, filler = topk(score, M, k, status_in, reject_mask)
    P = idx.shape[0]
    flat = np.arange(P)[:, None] * M + idx
    st = np.zeros((P * M,), np.int32) if status_in is None else np.asarray(status_in, dtype=np.int32).reshape(-1)
    return idx, np.asarray(score).reshape(-1)[flat], np.asarray(poses).reshape(P * M, 3, 4)[flat], st[flat] | (filler * STATUS_HYP_NO_SCORE).astype(np.int32)


TOPK_M, TOPK_K = 37, 4


def topk_cases():
    """score (3*37,) float32 and status (3*37,) int32 with reject mask 512 | 4: ties, -inf, NaN, +inf, -0 / +0, rejected candidates,
    a pair with fewer than k candidates and a pair with none"""
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(12)
    s = np.full((3, TOPK_M), -inf, np.float32)
    st = rng.integers(0, 4, size=(3, TOPK_M)).astype(np.int32) * 8   # bits outside the mask travel with the candidate
    # pair 0: plenty, with ties (the smaller m first), a rejected maximum, an infinity and the two zeros
    s[0] = rng.uniform(-0.5, 0.5, TOPK_M).astype(np.float32)
    s[0, [30, 7, 19]] = 0.75
    s[0, 3] = 0.9
    st[0, 3] |= 512
    s[0, 5], s[0, 6], s[0, 8] = inf, nan, -inf
    s[0, [11, 2]] = [0.0, -0.0]
    s[0, 20] = 0.6
    # pair 1: two candidates only (one more is rejected, the rest not finite)
    s[1, 36], s[1, 0], s[1, 17] = -0.25, -0.75, 0.5
    st[1, 17] |= 4
    s[1, 9] = nan
    # pair 2: none
    s[2, 4] = nan
    s[2, 5] = 0.3
    st[2, 5] |= 512 | 4
    return s.reshape(-1), st.reshape(-1), 512 | 4


# ------------------------------------------------------------------------------------------------------------------ shared cases
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


CONVERGENCE_SEED, CONVERGENCE_CASES = 20240, 1000


def convergence_cases(seed=CONVERGENCE_SEED, n=CONVERGENCE_CASES):
    """n seeded (points, R, t) under LINEMOD's K: anisotropic clouds of 200 points about 0.2 m across, a random rotation, t_z in
    [0.4, 1.5] m and the centre projected at least 120 px inside the 640 x 480 frame"""
    rng = np.random.default_rng(seed)
    K = LINEMOD_K
    for _ in range(n):
        pts = rng.normal(size=(200, 3)) * rng.uniform(0.4, 1.0, size=3)
        pts *= 0.2 / (pts.max(0) - pts.min(0)).max()
        R = random_rotation(rng)
        tz = rng.uniform(0.4, 1.5)
        u, v = rng.uniform(120, 520), rng.uniform(120, 360)
        yield pts, R, np.array([(u - K[0, 2]) * tz / K[0, 0], (v - K[1, 2]) * tz / K[1, 1], tz])


def convergence_errors(box_of, iters=(1, 8, 24)):
    """(n, len(iters)): |t - t*| / t*_z of the fit against box_of(exact box) after each number of iterations, z_init 1"""
    out = []
    for pts, R, t in convergence_cases():
        box = box_of(exact_box(pts, R, t, LINEMOD_K))
        row = []
        for it in iters:
            got, ok = box_fit(pts, R, box, LINEMOD_K, it, 1.0)
            assert ok
            row.append(np.linalg.norm(got - t) / t[2])
        out.append(row)
    return np.array(out)


# the pipeline scene of tests/test_gpu_coarse.py, checked on the CPU by tests/test_coarse_host.py: a quarter-size LINEMOD frame
PIPE_H, PIPE_W = 240, 320
PIPE_K = np.array([[286.2057, 0, 162.63055], [0, 286.785215, 121.024495], [0, 0, 1]], dtype=np.float32)   # LINEMOD's K / 2
PIPE_VIEWS, PIPE_INPLANE = 12, 4
PIPE_TRUE_M = (17, 38)                                                                                   # m_p of the two pairs
PIPE_T = np.array([[0.03, -0.02, 0.55], [-0.05, 0.03, 0.65]], dtype=np.float32)                          # t_p
PIPE_MODEL_SEED = 77


def pipeline_scene():
    """-> (models: two lib.utils.synthetic meshes, class_index (2,), pose_true (2,3,4) float32 = [R_grid[m_p] | t_p])"""
    from lib.utils import synthetic as syn

    models = syn.make_models(seed=PIPE_MODEL_SEED, n_models=2, subdiv=3)
    grid = rotation_grid(PIPE_VIEWS, PIPE_INPLANE).astype(np.float32)
    pose = np.zeros((2, 3, 4), np.float32)
    for p, m in enumerate(PIPE_TRUE_M):
        pose[p, :, :3] = grid[m]
        pose[p, :, 3] = PIPE_T[p]
    return models, np.array([0, 1], np.int32), pose


def pipeline_cpu(mode="rgb", iters=8, z_init=1.0):
    """the pipeline scene through the CPU rasteriser of oracle/ and the restatements: observed frames = the render at the true poses,
    boxes = the extents of their drawn pixels, candidates = the grid fitted to the boxes on the mesh vertices, scored by
    tests/hyp_reference.py.  -> (score (2, M) float64, boxes (2,4) float32, pose (2*M,3,4) float64)"""
    import hyp_reference as hr
    from lib.utils import synthetic as syn
    from oracle import native

    models, cls, pose_true = pipeline_scene()
    K, H, W = PIPE_K, PIPE_H, PIPE_W
    obs, dobs, boxes = [], [], []
    for p in range(2):
        v, t, f, tex = models[cls[p]]
        bgr, d = native.render(v, t, f, tex, pose_true[p][:, :3], pose_true[p][:, 3], K, H=H, W=W)
        ys, xs = np.nonzero(d > 0)
        boxes.append([xs.min() - 0.5, xs.max() + 0.5, ys.min() - 0.5, ys.max() + 0.5])
        obs.append(syn.bgr_to_blob(bgr)[0])
        dobs.append(np.where(d > 0, d, 1.5))   # in front of a wall
    boxes = np.array(boxes, np.float32)
    pts = np.concatenate([np.asarray(m[0], np.float64) for m in models])
    off = np.concatenate([[0], np.cumsum([len(m[0]) for m in models])])
    grid = rotation_grid(PIPE_VIEWS, PIPE_INPLANE).astype(np.float32).reshape(-1, 9)
    pose, status = pose_from_box(pts, off, cls, grid, boxes, K, iters, z_init)
    assert not status.any()
    M = len(grid)
    score = np.zeros((2, M))
    for p in range(2):
        v, t, f, tex = models[cls[p]]
        for m in range(M):
            q = pose[p * M + m].astype(np.float32)
            bgr, d = native.render(v, t, f, tex, q[:, :3], q[:, 3], K, H=H, W=W)
            score[p, m] = hr.score_one(mode, obs[p], syn.bgr_to_blob(bgr)[0], d, depth_observed=dobs[p], tau=0.02)
    return score, boxes, pose
