"""Analytic depth scenes for the term-by-term ICP tests (tests/test_icp_terms_host.py fixes them on the CPU, tests/test_gpu_icp_terms.py
runs them on the device): no render, no randomness in the depth.

The observed depth is a gently curved, tilted surface with a small ripple, z about 1 m, sampled at the pixel centres; the rendered
depth is the same surface read about a pixel away and a few millimetres deeper or nearer, so the first Gauss-Newton steps rotate
and shift the source points onto other pixels.  A patch of the rendered depth lies 1.5 max_dist too deep (points the
distance gate removes).  fx != fy and the principal point is off-centre.  Every scene comes in two variants: `plain` (whole frame, no
mask, the host K) and `cut` (its own irregular mask_observed, a bbox that leaves drawn pixels outside, K per pair)."""
import numpy as np

import icp_reference as ir

MAX_DIST = float(np.float32(0.02))   # the float the kernel receives
ITERS = 3                            # corrections T_0 (identity), T_1, T_2 at which the terms are compared

#         name   H    W   fx     shift (px)    dz      amp    mask seed
# The shifts and depths were searched on the CPU so that every gate decision of three iterations keeps the margins that
# tests/test_icp_terms_host.py asserts: a shift of about a pixel moves every point onto a neighbour pixel and, being nearly uniform
# over the frame, keeps all of them away from the rounding boundary.
BASES = [("f12", 12, 16, 20.0, (-1.30, 0.80), 0.0015, 0.039, 1),
         ("f24a", 24, 32, 40.0, (0.85, -1.20), 0.0030, 0.065, 2),
         ("f24b", 24, 32, 40.0, (0.85, -1.20), 0.0015, 0.045, 3),
         ("f24c", 24, 32, 40.0, (1.20, -1.20), -0.0020, 0.0715, 4),
         ("f37", 37, 50, 60.0, (1.20, -1.20), -0.0020, 0.078, 5),
         ("f72", 72, 80, 100.0, (0.85, -1.20), 0.0015, 0.104, 6),
         ("f96", 96, 128, 140.0, (1.20, -1.20), 0.0015, 0.104, 7)]
BATCH = ("f24a", "f24b", "f24c")     # one frame size: the batch of three with their own mask planes


def camera(H, W, fx):
    return np.array([[fx, 0.0, 0.5 * W - 0.7], [0.0, 1.08 * fx, 0.5 * H + 0.4], [0.0, 0.0, 1.0]], np.float32)


def surface(H, W, amp, sx=0.0, sy=0.0, dz=0.0):
    """float32 depth of the surface at pixel centres displaced by (sx, sy) pixels, dz deeper"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b = (x + sx - 0.5 * W) / (0.5 * W), (y + sy - 0.5 * H) / (0.5 * H)
    z = 1.0 + 0.020 * a - 0.015 * b + amp * (0.5 * a * a + 0.35 * b * b + 0.2 * a * b) \
        + 0.15 * amp * np.sin(3.1 * a + 0.5) * np.cos(2.7 * b - 0.3)
    return (z + dz).astype(np.float32)


def irregular_mask(H, W, seed):
    """1 outside an off-centre ellipse, inside it a fixed irregular pattern of 0 / 0.3 / 0.8 / 1: never within 0.01 of 0.5"""
    y, x = np.mgrid[0:H, 0:W]
    inside = ((x - 0.62 * W) / (0.22 * W)) ** 2 + ((y - 0.4 * H) / (0.3 * H)) ** 2 < 1.0
    pat = (x * 7 + y * 13 + seed * 5) % 11
    m = np.ones((H, W), np.float32)
    m[inside & (pat < 4)] = 0.0
    m[inside & (pat == 4)] = 0.3
    m[inside & (pat == 5)] = 0.8
    return m


def general_pose(seed):
    rng = np.random.default_rng(100 + seed)
    R = ir.rodrigues(rng.uniform(-0.8, 0.8, 3))
    return np.concatenate([R, rng.uniform(-0.3, 0.3, (3, 1)) + [[0.0], [0.0], [1.0]]], axis=1).astype(np.float32)


class Scene(object):
    def __init__(self, name, K, dr, do, mask=None, bbox=None, per_pair_K=False, pose_in=None):
        self.name, self.K, self.dr, self.do, self.mask, self.bbox, self.per_pair_K = name, K, dr, do, mask, bbox, per_pair_K
        self.H, self.W = dr.shape
        self.pose_in = general_pose(0) if pose_in is None else pose_in

    def partial(self, R, t, dtype, defect=None, margins=None, mask="own"):
        """-> partial (16, 29) float64 as the kernel sums them in dtype, terms (n, 29) of the surviving points"""
        s, idx = ir.source_points(self.dr, self.K, self.bbox, dtype, with_index=True)
        terms, idx = ir.point_terms(ir.move_points(s, R, t, dtype), self.do, self.K, MAX_DIST, self.mask if isinstance(mask, str) else mask,
                                    dtype, index=idx, defect=defect, margins=margins)
        return ir.lane_sums(terms, idx, dtype), terms

    def truth(self, R, t, margins=None):
        """float64 arithmetic on the same float32 inputs -> sums (29,), unit (29,) = sum of |contribution|"""
        _, terms = self.partial(R, t, np.float64, margins=margins)
        return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def term_error(S, truth, unit):
    """error of each of the 29 sums in units of sum |contribution| (0 where a term has no contribution at all)"""
    return np.abs(np.asarray(S, np.float64) - truth) / np.where(unit > 0, unit, 1.0)


def base(name):
    return next(b for b in BASES if b[0] == name)


def make(name, variant, params=None):
    _, H, W, fx, (sx, sy), dz, amp, seed = base(name) if params is None else params
    K = camera(H, W, fx)
    do = surface(H, W, amp)
    dr = surface(H, W, amp, sx, sy, dz)
    # a patch 1.5 max_dist too deep: the distance gate removes it, with a wide margin
    dr[H // 5:H // 5 + max(H // 6, 2), W // 6:W // 6 + max(W // 5, 2)] += np.float32(1.5 * MAX_DIST)
    pose = general_pose(seed)
    if variant == "plain":
        return Scene(name + "-plain", K, dr, do, pose_in=pose)
    assert variant == "cut"
    # the drawn area reaches the frame's edge; the box leaves a band of it outside on every side (and is not a multiple of anything)
    bbox = np.array([2, W - 4, 1, H - 3], np.int32)
    return Scene(name + "-cut", K, dr, do, mask=irregular_mask(H, W, seed), bbox=bbox, per_pair_K=True, pose_in=pose)


def all_scenes():
    return [make(b[0], v) for b in BASES for v in ("plain", "cut")]


# ---------------------------------------------------------------------------------------------------------------- hand-built gates
GH, GW = 8, 10            # the gate frame: 6 x 8 = 48 interior pixels, so no variant ever updates; only iteration 0 is read
GP = (4, 3)               # the pixel (x, y) the variants act on, interior, not next to the border


def gate_base(name="base", single=None):
    """observed: the surface; rendered: the same 1 mm deeper, drawn everywhere (48 inliers: the interior) or, with single = (x, y),
    at that pixel alone"""
    K = camera(GH, GW, 14.0)
    do = surface(GH, GW, 0.02)
    dr = do + np.float32(0.001)
    if single is not None:
        one = np.zeros_like(dr)
        one[single[1], single[0]] = dr[single[1], single[0]]
        dr = one
    return Scene("gate-" + name, K, dr, do, pose_in=general_pose(11))


def gate_variants():
    """-> [(scene, expected inliers at the identity)]; tests/test_icp_terms_host.py checks the expectation against the restatement"""
    x, y = GP
    out = [(gate_base(), 48)]
    for what, val in (("zero", 0.0), ("negative", -1.0), ("nan", np.nan)):            # rendered depth at one source pixel
        s = gate_base("rendered-" + what)
        s.dr[y, x] = val
        out.append((s, 47))
    for c in (0, 1, GW - 2, GW - 1):                                                    # one source pixel on a border column / row
        out.append((gate_base("col{}".format(c), single=(c, y)), int(1 <= c <= GW - 2)))
    for r in (0, 1, GH - 2, GH - 1):
        out.append((gate_base("row{}".format(r), single=(x, r)), int(1 <= r <= GH - 2)))
    s = gate_base("observed-zero")                                                      # the target and its four neighbours lose it
    s.do[y, x] = 0.0
    out.append((s, 43))
    for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1)):                   # one source pixel; (1, 1) is not read
        s = gate_base("single-zero{:+d}{:+d}".format(dx, dy), single=GP)
        s.do[y + dy, x + dx] = 0.0
        out.append((s, int((dx, dy) == (1, 1))))
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):                                   # neighbour jumps
        for f in (1.5, 0.5):
            s = gate_base("jump{}{:+d}{:+d}".format(f, dx, dy), single=GP)
            s.do[y + dy, x + dx] += np.float32(f * MAX_DIST)
            out.append((s, int(f < 1)))
    for f, n in ((1.5, 47), (0.5, 48), (-1.5, 47)):                                     # the distance gate
        s = gate_base("offset{}".format(f))
        s.dr[y, x] += np.float32(f * MAX_DIST)
        out.append((s, n))
    for val, n in ((0.0, 47), (0.49, 47), (0.5, 48), (1.0, 48), (np.nan, 47)):          # mask_observed at the target
        s = gate_base("mask{}".format(val))
        s.mask = np.ones((GH, GW), np.float32)
        s.mask[y, x] = val
        out.append((s, n))
    return out


def tiny_frame():
    """3 x 3: only the centre pixel can count"""
    K = camera(3, 3, 5.0)
    do = surface(3, 3, 0.01)
    return Scene("3x3", K, do + np.float32(0.001), do, pose_in=general_pose(12))


BOXES = {"min-below-0": (-5, 20, -3, 15), "max-beyond": (10, 100, 5, 99), "one-row": (0, 31, 7, 7), "one-column": (13, 13, 0, 23),
         "inverted": (20, 10, 3, 15), "inside-the-drawn-area": (8, 20, 6, 18)}


def box_scene(name):
    s = make("f24a", "plain")
    s.name, s.bbox = "box-" + name, np.array(BOXES[name], np.int32)
    return s


def threshold_pair():
    """10 x 10, every interior pixel an inlier: -> (scene with 64 inliers, the same with one masked pixel: 63)"""
    out = []
    for n in (64, 63):
        K = camera(10, 10, 16.0)
        do = surface(10, 10, 0.025)
        s = Scene("threshold-{}".format(n), K, do + np.float32(0.001), do, mask=np.ones((10, 10), np.float32), pose_in=general_pose(13))
        if n == 63:
            s.mask[5, 4] = 0.0
        out.append(s)
    return out


def update_then_skip():
    """f37 with every third pixel drawn and mask_observed = exactly those pixels: the identity hits them all, the first update moves
    every point onto a neighbour pixel, which the mask removes"""
    s = make("f37", "plain")
    y, x = np.mgrid[0:s.H, 0:s.W]
    grid = (x % 3 == 1) & (y % 3 == 1)
    s.name, s.dr, s.mask = "update-then-skip", np.where(grid, s.dr, np.float32(0.0)), grid.astype(np.float32)
    return s


def zero_residual():
    s = make("f24a", "plain")
    s.name, s.dr = "zero-residual", s.do.copy()
    return s


def model_chain(scene, iters=ITERS):
    """the float32 model iterated: -> [(R_k, t_k)] for k = 0 .. iters - 1, the corrections at which iteration k takes its sums"""
    R, t = np.eye(3), np.zeros(3)
    chain = []
    for _ in range(iters):
        chain.append((R, t))
        part, _ = scene.partial(R, t, np.float32)
        R, t, _ = ir.gn_step(R, t, part.sum(axis=0))
    return chain
