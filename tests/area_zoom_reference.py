"""Plain numpy restatement of the area-filtered zoom (csrc/zoom.hip dim_zoom_planes_area / dim_zoom_net_input_area / dim_zoom_area_taps,
DESIGN.md section 6d): where the zoom window shrinks the source, every network pixel is the mean of n_y x n_x bilinear samples taken at
sub-pixel offsets of the network grid.  It extends tests/source_size_reference.py (same inputs, same float32 discipline: ONE rounding
per operation) and is pinned by tests/test_area_zoom_host.py to oracle.zoom.bilinear_sampler on shifted grids.

    step_x = |wx| * f32((Ws - 1) / (Wn - 1))                  source pixels per network pixel (the quotient in double, rounded once)
    n_x    = min(max(floor(step_x + 0.5), 1), max_taps)       per axis; fmax before fmin: a NaN step gives 1, an infinite one max_taps
    o_k    = f32((k + 0.5) / n - 0.5), k < n                  (in double, rounded once; exactly 0 for n = 1)
    x_t    = -1 + (f32(j) + o_kx) * f32(2 / (Wn - 1))         then source_size_reference's arithmetic unchanged
    value  = (s_00 + s_01 + ... ) / f32(n_x n_y)              ky outer, kx inner; the first sample starts the sum; then `- add`, rounding

`mutant=NAME` evaluates a plausible wrong kernel instead (MUTANTS lists them).
"""
from fractions import Fraction

import numpy as np

import source_size_reference as S
from source_size_reference import SIZE_PAIRS, ZOOM_MEANS, mx_round, round_boundary_distance_ulps  # noqa: F401

f32 = np.float32

MUTANTS = ("offsets_not_centred",     # o_k = k / n
           "one_n",                   # the x axis's count for both axes
           "ceil",                    # n = ceil(step) instead of round-half-up
           "step_network",            # the step from the network-to-network ratio: |w| * 1
           "mean_of_rounded",         # the mask lanes: the mean of the ROUNDED samples
           "divide_by_sum")           # the sum divided by n_x + n_y

MAX_TAPS = 4
# tests/pixel_kernels_reference.py ZOOM_FACTORS (zoom in; the exact identity; a window larger than the frame; far outside; 1e30) and four
# rows of this module: 1.45 (three source pixels per network pixel at ratio 2.1-2.2), unequal axes, 2.7 (past max_taps = 4 at ratio 2),
# a mirrored window (wx < 0: the step is |wx|)
ZOOM_FACTORS = np.concatenate([S.ZOOM_FACTORS, np.array([[1.45, 1.45, 0.05, -0.1], [0.9, 1.15, -0.2, 0.1], [2.7, 2.7, 0, 0],
                                                         [-1.25, 1.25, 0.1, 0]], f32)]).astype(f32)
ZOOM_B = len(ZOOM_FACTORS)
STRIPE_PAIRS = (((24, 32), (12, 16)), ((48, 64), (12, 16)))     # full-frame window: steps 2.07 / 2.09 and 4.2 / 4.27


def zoom_inputs(H, W):
    """source_size_reference.zoom_inputs for ZOOM_B = 9 pairs: its 5 and the first 4 of a second draw"""
    a, b = S.zoom_inputs(H, W), S.zoom_inputs(H, W, seed=1)
    return {k: np.concatenate([a[k], b[k]])[:ZOOM_B].copy() for k in a}


def ratio(s, n):
    return f32((s - 1) / (n - 1))


def steps(zf, Hs, Ws, Hn, Wn, mutant=None):
    """(B,2) float32 (step_x, step_y)"""
    zf = np.asarray(zf, f32).reshape(-1, 4)
    rx, ry = (f32(1), f32(1)) if mutant == "step_network" else (ratio(Ws, Wn), ratio(Hs, Hn))
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.stack([np.abs(zf[:, 0]) * rx, np.abs(zf[:, 1]) * ry], axis=1)
    assert out.dtype == f32
    return out


def taps(zf, Hs, Ws, Hn, Wn, max_taps=MAX_TAPS, mutant=None):
    """(B,2) int32 (n_x, n_y), as dim_zoom_area_taps writes them"""
    assert mutant is None or mutant in MUTANTS, mutant
    st = steps(zf, Hs, Ws, Hn, Wn, mutant)
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.ceil(st) if mutant == "ceil" else np.floor(st + f32(0.5))
        n = np.fmin(np.fmax(n, f32(1)), f32(max_taps))          # fmax / fmin return the other operand for a NaN, as fmaxf / fminf do
    n = n.astype(np.int32)
    if mutant == "one_n":
        n[:, 1] = n[:, 0]
    return n


def offsets(n, mutant=None):
    return np.array([(k / n) if mutant == "offsets_not_centred" else ((k + 0.5) / n - 0.5) for k in range(n)], dtype=np.float64).astype(f32)


def _bilinear(x, zf4, Hn, Wn, oy, ox, add, pre):
    """x (C,Hs,Ws) of one pair -> (C,Hn,Wn): sample(pre(x) + add) at the network grid shifted by (oy, ox) pixels, BEFORE `- add`;
    source_size_reference.zoom_sample_src's arithmetic with x_t = -1 + (f32(j) + o) * f32(2 / (Wn - 1))"""
    C, Hs, Ws = x.shape
    one = f32(1)
    wx, wy, tx, ty = zf4
    xt = f32(-1) + (np.arange(Wn, dtype=f32) + f32(ox)) * f32(2.0 / (Wn - 1))
    yt = f32(-1) + (np.arange(Hn, dtype=f32) + f32(oy)) * f32(2.0 / (Hn - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        xr = (((wx * xt + tx) + one) * f32(Ws - 1)) / f32(2)
        yr = (((wy * yt + ty) + one) * f32(Hs - 1)) / f32(2)
    x0f, y0f = np.floor(xr), np.floor(yr)
    wx0 = (one - (xr - x0f))[None, :]
    wy0 = (one - (yr - y0f))[:, None]
    x0 = np.clip(x0f, -2, Ws + 1).astype(np.int64)
    y0 = np.clip(y0f, -2, Hs + 1).astype(np.int64)
    out = np.empty((C, Hn, Wn), f32)
    for c in range(C):
        p = x[c]
        if pre == 1:
            p = np.where(p > f32(0.2), one, f32(0))
        p = (p + add[c]).astype(f32)

        def corner(yy, xx):
            vy, vx = (yy >= 0) & (yy <= Hs - 1), (xx >= 0) & (xx <= Ws - 1)
            v = p[np.clip(yy, 0, Hs - 1)[:, None], np.clip(xx, 0, Ws - 1)[None, :]]
            return np.where(vy[:, None] & vx[None, :], v, f32(0))
        tl, tr, bl, br = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
        wx1, wy1 = one - wx0, one - wy0
        r = (tl * wy0) * wx0
        r = r + (tr * wy0) * wx1
        r = r + (bl * wy1) * wx0
        r = r + (br * wy1) * wx1
        out[c] = r
    assert out.dtype == f32
    return out


def zoom_sample_area(x, zf, Hn, Wn, max_taps=MAX_TAPS, add=None, pre=0, mutant=None, round_each=False, n_xy=None):
    """x (B,C,Hs,Ws) f32 -> (B,C,Hn,Wn): mean(sample(pre(x) + add)) - add, un-rounded.  n_xy: (B,2) counts to use instead of taps();
    round_each: every sample rounded (mx_round) before it is summed (the mask lanes' mutant)"""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x, f32)
    B, C, Hs, Ws = x.shape
    zf = np.asarray(zf, f32).reshape(B, 4)
    add = np.zeros(C, f32) if add is None else np.asarray(add, f32)
    n_xy = taps(zf, Hs, Ws, Hn, Wn, max_taps, mutant) if n_xy is None else np.asarray(n_xy)
    out = np.empty((B, C, Hn, Wn), f32)
    for b in range(B):
        nx, ny = int(n_xy[b, 0]), int(n_xy[b, 1])
        ox, oy = offsets(nx, mutant), offsets(ny, mutant)
        acc = None
        for ky in range(ny):
            for kx in range(nx):
                r = _bilinear(x[b], zf[b], Hn, Wn, oy[ky], ox[kx], add, pre)
                if round_each:
                    r = mx_round(r)
                acc = r if acc is None else acc + r            # the first sample starts the sum: a -0 survives n = 1
        count = f32(nx + ny) if mutant == "divide_by_sum" else f32(nx * ny)
        out[b] = (acc / count) - add.reshape(C, 1, 1)
    assert out.dtype == f32
    return out


def zoom_planes_area(x, zf, Hn, Wn, max_taps=MAX_TAPS, pre=0, post=0, add3=None, mutant=None):
    """(value as dim_zoom_planes_area writes it, the value before rounding or None)"""
    add = None if (add3 is None or x.shape[1] > 3) else add3
    v = zoom_sample_area(x, zf, Hn, Wn, max_taps, add, pre, mutant)
    if post == 1:
        return mx_round(v), v
    if post == 2:
        before = v - f32(0.45)
        return mx_round(before), before
    return v, None


def net_input_area(io, ir, eo, er, zf, means, mode, Hn, Wn, max_taps=MAX_TAPS, mutant=None):
    """dim_zoom_net_input_area: source_size_reference.net_input_src's lanes with every sample replaced by the mean of its sub-samples;
    the mask lanes are round(mean(sample(mask))), the depth lanes of mode 2 mean(sample(depth)) / 255"""
    B = io.shape[0]
    X = np.zeros((B, Hn, Wn, 8), f32)
    c255 = f32(255)
    s = lambda x, add=None, pre=0, **kw: zoom_sample_area(x, zf, Hn, Wn, max_taps, add, pre, mutant, **kw)  # noqa: E731
    zio, zir = s(io, means), s(ir, means)
    pre_o = pre_r = zmo = zmr = None
    if mode != 3:
        X[..., 0:3] = (zio / c255).transpose(0, 2, 3, 1)
        X[..., 3:6] = (zir / c255).transpose(0, 2, 3, 1)
    if mode in (0, 3):
        each = mutant == "mean_of_rounded"
        pre_o, pre_r = s(eo, round_each=each), s(er, pre=1, round_each=each)
        zmo, zmr = mx_round(pre_o), mx_round(pre_r)
        lo = 6 if mode == 0 else 0
        X[..., lo], X[..., lo + 1] = zmo[:, 0], zmr[:, 0]
    elif mode == 2:
        X[..., 6], X[..., 7] = s(eo)[:, 0] / c255, s(er)[:, 0] / c255
    return {"X": X, "nchw": (zio, zir, zmo, zmr), "pre_round": (pre_o, pre_r)}


def stripe_source(Hs, Ws):
    """(1,1,Hs,Ws): vertical stripes of period 2 pixels, 0 / 255 -- finer than a network pixel at either STRIPE_PAIRS ratio"""
    return np.tile((np.arange(Ws) % 2).astype(f32) * f32(255), (Hs, 1))[None, None].copy()


def stripe_stats(out):
    """(peak-to-peak, mean) over the interior rows and columns [2:-2] of a (1,1,Hn,Wn) output"""
    inner = np.asarray(out, np.float64)[0, 0, 2:-2, 2:-2]
    return float(inner.max() - inner.min()), float(inner.mean())


def check_stripes(area, bilinear, what):
    """the behaviour asserted of an area-filtered stripe output next to the bilinear one (host restatement and device alike): the
    interior peak-to-peak at most 1/4 of the bilinear output's -- a condition, not a measurement -- and the interior mean within 1 of 127.5"""
    (pa, ma), (pb, mb) = stripe_stats(area), stripe_stats(bilinear)
    print("{}: peak-to-peak area {:.3f} bilinear {:.3f} (ratio {:.3f}); interior mean area {:.3f}".format(what, pa, pb, pa / pb, ma))
    assert pb > 100, what                     # the bilinear output does alias
    assert pa <= 0.25 * pb, what
    assert abs(ma - 127.5) <= 1.0, what


FULL_FRAME = np.array([[1, 1, 0, 0]], f32)

# The tap rule at its boundaries, for sizes whose ratio is exact in float32: 17 -> 9 gives 16 / 8 = 2, so step = 2 |w| exactly.
# |w| = 0.75: step + 0.5 = 2 exactly -> 2; one ulp below: 1.49999988 + 0.5 = 1.99999988 (representable) -> 1; one ulp above: 1.50000012 +
# 0.5 lies halfway between 2 and 2.00000024 and rounds to even, 2 -> 2.  |w| = 1.25: 3; one ulp below 2.99999976 -> 2; above -> 3.
# NaN -> 1 (fmax first); inf and 1e30 -> max_taps; a negative w counts as |w|; 0 -> 1.
BOUNDARY_SIZES = ((17, 17), (9, 9))
BOUNDARY_MAX_TAPS = 5


def boundary_cases():
    """(zf (B,4), expected (B,2) int32): wx walks through the cases, wy = the mirrored value of the same case"""
    w, want = [], []
    for centre, n in ((0.75, 2), (1.25, 3)):
        c = f32(centre)
        w += [np.nextafter(c, f32(0)), c, np.nextafter(c, f32(9))]
        want += [n - 1, n, n]
    w += [f32(np.nan), f32(np.inf), f32(1e30), f32(0), f32(-1.25), f32(-1e30), f32(3.9)]
    want += [1, BOUNDARY_MAX_TAPS, BOUNDARY_MAX_TAPS, 1, 3, BOUNDARY_MAX_TAPS, BOUNDARY_MAX_TAPS]
    w = np.array(w, f32)
    zf = np.stack([w, -w, np.zeros_like(w), np.zeros_like(w)], axis=1).astype(f32)
    return zf, np.stack([want, want], axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- conditions on the inputs
def _step_is_exact(w, s, n, step):
    """the float32 step equals |w| (s - 1) / (n - 1) in exact arithmetic: no rounding took place, so no last bit decides the count"""
    return np.isfinite(step) and Fraction(float(abs(w))) * Fraction(s - 1, n - 1) == Fraction(float(step))


def half_integer_distance(step):
    s = float(step)
    return abs(s - np.floor(s) - 0.5)


def _check_inputs():
    """no step of any case lies within 1e-3 of a half-integer, so that no tap count depends on the last bit of the step.  (A step that
    is EXACT in float32 -- |w| = 1 on the 21 -> 9 rows axis: 20 / 8 = 2.5 -- involves no rounding at all; its count is the rule's own
    round-half-up of an exact number and equally independent of any last bit.  The boundary itself is tested on its own in
    tests/test_area_zoom_host.py.)  And the size pairs together reach (1,1), (2,2), (3,3), a mixed pair and the max_taps clamp."""
    seen = set()
    for (Hs, Ws), (Hn, Wn) in SIZE_PAIRS + STRIPE_PAIRS:
        table = ZOOM_FACTORS if ((Hs, Ws), (Hn, Wn)) in SIZE_PAIRS else FULL_FRAME
        st = steps(table, Hs, Ws, Hn, Wn)
        for b in range(len(table)):
            for axis, (s, n) in enumerate(((Ws, Wn), (Hs, Hn))):
                step = st[b, axis]
                assert half_integer_distance(step) > 1e-3 or _step_is_exact(table[b, axis], s, n, step), ((Hs, Ws), (Hn, Wn), b, axis, step)
        if table is ZOOM_FACTORS:
            raw = np.floor(st.astype(np.float64) + 0.5)
            seen |= {tuple(int(v) for v in t) for t in taps(table, Hs, Ws, Hn, Wn, MAX_TAPS)}
            if (raw[np.isfinite(raw)] > MAX_TAPS).any():
                seen.add("clamp")
    for want in ((1, 1), (2, 2), (3, 3), (1, 3), "clamp"):
        assert want in seen, (want, seen)


_check_inputs()


# ------------------------------------------------------------------------------------------- refinement-loop scenes and the oracle loop
# (the helpers of tests/test_gpu_source_size_refine.py, with the source size an argument, a scene whose object fills the frame, and
# the sampler of the oracle's forward a choice; oracle and torch are imported where they are used: the host tests need neither)
NET = (480, 640)
LOOP_T = 2
LOOP_BLOBS = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")


def source_K(Hs):
    """the LINEMOD camera scaled to an image Hs rows high"""
    from lib.utils import synthetic as syn

    K = np.array(syn.LINEMOD_K, np.float64) * (Hs / float(NET[0]))
    K[2, 2] = 1.0
    return K.astype(f32)


def make_loop_scene(Hs, Ws, B=2, fill=None, seed=2333, subdiv=3, shift=0.0):
    """tests/scene.py make_scene in the frame of a source camera, rendered by the CPU oracle at Hs x Ws.  fill: None = the draws of
    lib.utils.synthetic.sample_pairs (small objects: every window magnifies), else the fraction of the frame height the object's
    diameter spans, the object near the frame centre (fill 0.6 at 960x1280: a window of 0.8-0.9 of the frame, two source pixels per
    network pixel and more); shift: the object's centre below the frame centre, as a fraction of the frame height (fill 2.2 and shift
    0.1 at 480x640: an object larger than the frame, a window of 1.6 frames)"""
    from lib.utils import synthetic as syn
    from oracle import native

    K = source_K(Hs)
    models = syn.make_models(seed=seed, n_models=1, subdiv=subdiv)
    if fill is None:
        cls, gt, init = syn.sample_pairs(seed + 1, B, n_classes=1, frame=(K, Ws, Hs))
    else:
        rng = np.random.default_rng(seed + 1)
        cls = np.zeros(B, np.int32)
        pts = models[0][0].astype(np.float64)
        diam = float(np.linalg.norm(pts.max(0) - pts.min(0)))
        gt = []
        for b in range(B):
            z = float(K[1, 1]) * diam / (fill * Hs) * (1.0 + 0.1 * b)
            u, v = Ws / 2.0 + rng.uniform(-0.03, 0.03) * Ws, Hs / 2.0 + (shift + rng.uniform(-0.03, 0.03)) * Hs
            t = np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z])
            gt.append(np.concatenate([syn.random_rotation(rng), t.reshape(3, 1)], axis=1).astype(f32))
        gt = np.stack(gt)
        init = np.stack([syn.perturb_pose(rng, gt[b], xy_std=0.005, z_std=0.02) for b in range(B)])
    rng = np.random.default_rng(seed + 2)
    io, ir, mo, mr = [], [], [], []
    for b in range(B):
        v, t, f, tex = models[cls[b]]
        bgr_gt, d_gt = native.render(v, t, f, tex, gt[b][:, :3], gt[b][:, 3], K, H=Hs, W=Ws)
        obs = syn.compose_observed(bgr_gt, d_gt, rng)
        bgr_r, d_r = native.render(v, t, f, tex, init[b][:, :3], init[b][:, 3], K, H=Hs, W=Ws)
        io.append(syn.bgr_to_blob(obs))
        ir.append(syn.bgr_to_blob(bgr_r.astype(np.uint8)))
        m_r = (d_r > 0.2).astype(f32)
        mr.append(m_r[None, None])
        mo.append(syn.box_from_mask(m_r)[None, None])
    blobs = {"image_observed": np.concatenate(io).astype(f32), "image_rendered": np.concatenate(ir).astype(f32),
             "mask_observed": np.concatenate(mo).astype(f32), "mask_rendered": np.concatenate(mr).astype(f32),
             "src_pose": init.astype(f32), "class_index": cls}
    return {"models": models, "K": K, "blobs": blobs, "pose_gt": gt, "size": (Hs, Ws)}


def oracle_window(batch, K, size):
    """the zoom window of one forward: oracle.zoom.zoom_factor_from_valid at the source size"""
    from oracle import zoom as ozoom

    mo, mr = np.asarray(batch["mask_observed"], f32), np.asarray(batch["mask_rendered"], f32)
    mr_bin = np.where(mr > 0.2, f32(1), f32(0)).astype(f32)
    zf, _ = ozoom.zoom_factor_from_valid(np.sum(mo, axis=1) > 0.3, np.sum(mr_bin, axis=1) > 0.3, batch["src_pose"], K, *size)
    return zf


def oracle_forward(params, batch, K, pixel_means, size, sampler="area", max_taps=MAX_TAPS):
    """one forward from source-size blobs: the window at the source size, the blobs sampled into 480x640 -- sampler "area": this
    module's restatement (pinned to oracle.zoom.bilinear_sampler on shifted grids by tests/test_area_zoom_host.py), "bilinear": the
    oracle's own sampler on its own grid -- then the unchanged Concat, encoder, heads and inverse ZoomTrans"""
    import torch

    from oracle import flownet as oflow, zoom as ozoom

    Hn, Wn = NET
    zf = oracle_window(batch, K, size)
    io, ir = np.asarray(batch["image_observed"], f32), np.asarray(batch["image_rendered"], f32)
    mo, mr = np.asarray(batch["mask_observed"], f32), np.asarray(batch["mask_rendered"], f32)
    if sampler == "area":
        means = np.asarray(pixel_means, f32).reshape(3)[::-1]
        zio, zir = zoom_sample_area(io, zf, Hn, Wn, max_taps, add=means), zoom_sample_area(ir, zf, Hn, Wn, max_taps, add=means)
        zmo, zmr = mx_round(zoom_sample_area(mo, zf, Hn, Wn, max_taps)), mx_round(zoom_sample_area(mr, zf, Hn, Wn, max_taps, pre=1))
    else:
        assert sampler == "bilinear", sampler
        grid = ozoom._grid_from_factor(zf, Hn, Wn)
        pm = np.asarray(pixel_means, f32).reshape(3)[::-1].reshape(1, 3, 1, 1)
        mr_bin = np.where(mr > 0.2, f32(1), f32(0)).astype(f32)
        zio = (ozoom.bilinear_sampler(io + pm, grid) - pm).astype(f32)
        zir = (ozoom.bilinear_sampler(ir + pm, grid) - pm).astype(f32)
        zmo, zmr = ozoom.mx_round(ozoom.bilinear_sampler(mo, grid)), ozoom.mx_round(ozoom.bilinear_sampler(mr_bin, grid))
    data = oflow.network_input(zio, zir, zmo.astype(f32), zmr.astype(f32))
    assert data.shape[2:] == (Hn, Wn)
    with torch.no_grad():
        fc7 = oflow.encoder(params, torch.from_numpy(np.ascontiguousarray(data, dtype=f32)))
        rot = torch.nn.functional.linear(fc7, oflow._t(params, "rot_weight", torch.float32), oflow._t(params, "rot_bias", torch.float32))
        tz = torch.nn.functional.linear(fc7, oflow._t(params, "trans_weight", torch.float32), oflow._t(params, "trans_bias", torch.float32))
    trans = ozoom.zoom_trans(zf, tz.numpy(), b_inv_zoom=True)
    return np.concatenate([rot.numpy(), trans], axis=1).astype(f32)[0], zf


def oracle_loop(params, mesh, blobs_b, K, pixel_means, size, forced_poses=None, sampler="area", max_taps=MAX_TAPS, test_iter=LOOP_T):
    """oracle.refine.refine_pair's loop on source-size blobs (one pair, UPDATE_MASK 'box_rendered'): -> (poses, se3s, windows)"""
    from oracle import native, se3 as ose3
    from oracle.refine import image_transform, update_mask_observed_box_rendered

    Hs, Ws = size
    verts, uvs, faces, tex = mesh
    z3, o3 = np.zeros(3), np.ones(3)
    batch = {k: np.array(v, dtype=f32) for k, v in blobs_b.items()}
    pose_rendered = np.array(batch["src_pose"][0], dtype=np.float64)
    poses, se3s, windows = [], [], []
    for it in range(test_iter):
        se3, zf = oracle_forward(params, batch, K, pixel_means, size, sampler, max_taps)
        se3s.append(se3), windows.append(zf)
        pose_new = ose3.RT_transform(pose_rendered, se3[:-3], se3[-3:], z3, o3, "CAMERA")
        poses.append(pose_new)
        if forced_poses is not None:
            pose_new = np.array(forced_poses[it], dtype=np.float64)
        if it < test_iter - 1:
            bgr, depth = native.render(verts, uvs, faces, tex, pose_new[:3, :3], pose_new[:, 3], K, H=Hs, W=Ws)
            mask_r = np.zeros(depth.shape)
            mask_r[depth > 0.2] = 1
            batch["image_rendered"] = image_transform(bgr.astype("uint8").astype(np.float64), pixel_means).astype(f32)
            batch["mask_rendered"] = mask_r[None, None].astype(f32)
            batch["mask_observed"] = update_mask_observed_box_rendered(mask_r)[None, None].astype(f32)
            batch["src_pose"] = pose_new[None].astype(f32)
            pose_rendered = pose_new
    return poses, se3s, windows
