"""Plain numpy restatement of the two-size zoom (csrc/zoom.hip dim_zoom_planes_src / dim_zoom_net_input_src): planes of a SOURCE size
(Hs, Ws) sampled into the NETWORK size (Hn, Wn), the zoom window given in the source's normalised coordinates.  It extends
tests/pixel_kernels_reference.py (same inputs, same float32 discipline: ONE rounding per operation, in oracle/zoom.py's order) and is
pinned by tests/test_source_size_host.py to oracle.zoom.bilinear_sampler(x, oracle.zoom._grid_from_factor(zf, Hn, Wn)).

    x_t = -1 + j * f32(2 / (Wn - 1)), j < Wn;   x_s = wx * x_t + tx;   x_r = (x_s + 1) * (Ws - 1) / 2
    corners valid inside [0, Ws - 1] x [0, Hs - 1], read at offset y * Ws + x of the source plane

`mutant=NAME` evaluates a plausible wrong kernel instead (MUTANTS lists them per operation).
"""
import numpy as np

from pixel_kernels_reference import ZOOM_B, ZOOM_FACTORS, ZOOM_MEANS, mx_round, round_boundary_distance_ulps, zoom_inputs  # noqa: F401

f32 = np.float32

MUTANTS = {
    "sample": ("grid_from_source",      # the target grid's step from the source size: 2 / (Ws - 1)
               "xreal_network",         # x_real scaled by the network size: (x_s + 1) (Wn - 1) / 2
               "valid_network",         # corner validity (and the clamp) against the network size
               "stride_network",        # row stride of the plane that is read from the network width
               "sizes_swapped"),        # Hs and Ws exchanged in x_real and the validity test
    "window": ("window_network",),      # tx, ty of the window rule as fractions of the network size
}

# (Hs, Ws) -> (Hn, Wn): ratio 1.5; ratio 2; a source smaller than the network; unequal ratios with a 128-wide block; a network row
# across two 256-thread blocks
SIZE_PAIRS = (((9, 12), (6, 8)), ((12, 16), (6, 8)), ((6, 8), (12, 16)), ((21, 77), (9, 128)), ((13, 300), (6, 260)))
SAME_SIZE = (16, 36)


def _check(op, mutant):
    assert mutant is None or mutant in MUTANTS[op], (op, mutant)


def zoom_sample_src(x, zf, Hn, Wn, add=None, pre=0, mutant=None):
    """x (B,C,Hs,Ws) f32 -> (B,C,Hn,Wn): sample(pre(x) + add) - add, un-rounded"""
    _check("sample", mutant)
    x = np.asarray(x, f32)
    B, C, Hs, Ws = x.shape
    zf = np.asarray(zf, f32).reshape(B, 4)
    add = np.zeros(C, f32) if add is None else np.asarray(add, f32)
    one = f32(1)
    gw, gh = (Ws - 1, Hs - 1) if mutant == "grid_from_source" else (Wn - 1, Hn - 1)
    xt = f32(-1) + np.arange(Wn, dtype=f32) * f32(2.0 / gw)
    yt = f32(-1) + np.arange(Hn, dtype=f32) * f32(2.0 / gh)
    rw, rh = {"xreal_network": (Wn, Hn), "sizes_swapped": (Hs, Ws)}.get(mutant, (Ws, Hs))        # x_real's scale
    vw, vh = {"valid_network": (Wn, Hn), "sizes_swapped": (Hs, Ws)}.get(mutant, (Ws, Hs))        # validity and clamp
    stride = Wn if mutant == "stride_network" else Ws
    out = np.empty((B, C, Hn, Wn), f32)
    for b in range(B):
        wx, wy, tx, ty = zf[b]
        with np.errstate(over="ignore", invalid="ignore"):
            xr = (((wx * xt + tx) + one) * f32(rw - 1)) / f32(2)
            yr = (((wy * yt + ty) + one) * f32(rh - 1)) / f32(2)
        x0f, y0f = np.floor(xr), np.floor(yr)
        wx0 = (one - (xr - x0f))[None, :]
        wy0 = (one - (yr - y0f))[:, None]
        x0 = np.clip(x0f, -2, vw + 1).astype(np.int64)
        y0 = np.clip(y0f, -2, vh + 1).astype(np.int64)
        for c in range(C):
            p = x[b, c]
            if pre == 1:
                p = np.where(p > f32(0.2), one, f32(0))
            flat = (p + add[c]).ravel()

            def corner(yy, xx):
                vy, vx = (yy >= 0) & (yy <= vh - 1), (xx >= 0) & (xx <= vw - 1)
                off = np.clip(yy, 0, vh - 1)[:, None] * stride + np.clip(xx, 0, vw - 1)[None, :]
                v = flat[np.clip(off, 0, flat.size - 1)]      # (a wrong kernel would read out of bounds; the restatement stays inside)
                return np.where(vy[:, None] & vx[None, :], v, f32(0))
            tl, tr, bl, br = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
            wx1, wy1 = one - wx0, one - wy0
            r = (tl * wy0) * wx0
            r = r + (tr * wy0) * wx1
            r = r + (bl * wy1) * wx0
            r = r + (br * wy1) * wx1
            out[b, c] = r - add[c]
    assert out.dtype == f32
    return out


def zoom_planes_src(x, zf, Hn, Wn, pre=0, post=0, add3=None, mutant=None):
    """(value as dim_zoom_planes_src writes it, the value before rounding or None)"""
    add = None if (add3 is None or x.shape[1] > 3) else add3
    v = zoom_sample_src(x, zf, Hn, Wn, add, pre, mutant)
    if post == 1:
        return mx_round(v), v
    if post == 2:
        before = v - f32(0.45)
        return mx_round(before), before
    return v, None


def net_input_src(io, ir, eo, er, zf, means, mode, Hn, Wn, mutant=None):
    """dim_zoom_net_input_src: X (B,Hn,Wn,8) NHWC + the four NCHW tensors of mode 0 + the pre-round values of the two mask lanes (the
    lanes of tests/pixel_kernels_reference.py net_input, mode by mode)"""
    B = io.shape[0]
    X = np.zeros((B, Hn, Wn, 8), f32)
    c255 = f32(255)
    s = lambda x, add=None, pre=0: zoom_sample_src(x, zf, Hn, Wn, add, pre, mutant)  # noqa: E731
    zio, zir = s(io, means), s(ir, means)
    pre_o = pre_r = zmo = zmr = None
    if mode != 3:
        X[..., 0:3] = (zio / c255).transpose(0, 2, 3, 1)
        X[..., 3:6] = (zir / c255).transpose(0, 2, 3, 1)
    if mode in (0, 3):
        pre_o, pre_r = s(eo), s(er, pre=1)
        zmo, zmr = mx_round(pre_o), mx_round(pre_r)
        lo = 6 if mode == 0 else 0
        X[..., lo], X[..., lo + 1] = zmo[:, 0], zmr[:, 0]
    elif mode == 2:
        X[..., 6], X[..., 7] = s(eo)[:, 0] / c255, s(er)[:, 0] / c255
    return {"X": X, "nchw": (zio, zir, zmo, zmr), "pre_round": (pre_o, pre_r)}


def window(bbox_obs, bbox_ren, src_pose, K, Hs, Ws, Hn=None, Wn=None, mutant=None):
    """the zoom window from the two SOURCE-size boxes {min_x, max_x, min_y, max_y} (both non-empty) and the source camera K:
    oracle.zoom.zoom_factor_from_valid's rule with H = Hs, W = Ws -- wx = wy = crop_h / Hs, tx = zcx / Ws * 2 - 1, ty = zcy / Hs * 2 - 1
    (float32 K t; the device kernel continues in float64, within 2e-6 of this)"""
    _check("window", mutant)
    tw, th = (Wn, Hn) if mutant == "window_network" else (Ws, Hs)
    K = np.asarray(K, f32).reshape(3, 3)
    zf = np.zeros((len(bbox_obs), 4), f32)
    for b, (bo, br) in enumerate(zip(bbox_obs, bbox_ren)):
        # numpy's own widths, as in the oracle: the box edges are int64 (differences with them are float64), the projected centre is a
        # float32 scalar (tx and ty, which mix it with Python numbers only, stay float32)
        rsx, rex, rsy, rey = (np.int64(v) for v in bo)
        dsx, dex, dsy, dey = (np.int64(v) for v in br)
        c = np.dot(K, np.asarray(src_pose[b], f32)[:, 3])
        zcx, zcy = c[0] / c[2], c[1] / c[2]
        left, right = max(zcx - dsx, zcx - rsx), max(dex - zcx, rex - zcx)
        up, down = max(zcy - dsy, zcy - rsy), max(rey - zcy, dey - zcy)
        crop_h = np.max([0.75 * right, 0.75 * left, up, down]) * 1.4 * 2
        wx = crop_h / Hs
        zf[b] = [wx, wx, zcx / tw * 2 - 1, zcy / th * 2 - 1]
    return zf


def window_case(Hs, Ws):
    """boxes, poses and a camera of the source size for `window`: two pairs whose projected centre lies off the frame centre"""
    K = np.array([[1.2 * Ws, 0, 0.5 * Ws - 0.7], [0, 1.2 * Ws, 0.5 * Hs + 0.4], [0, 0, 1]], f32)
    pose = np.tile(np.eye(3, 4, dtype=f32), (2, 1, 1))
    pose[:, :, 3] = [[0.05, -0.03, 0.8], [-0.1, 0.06, 1.1]]
    bo = np.array([[Ws // 3, Ws // 2, Hs // 4, Hs // 2], [Ws // 5, Ws // 3, Hs // 2, Hs - 2]], np.int32)
    br = np.array([[Ws // 3 + 1, Ws // 2 + 2, Hs // 4 + 1, Hs // 2 - 1], [Ws // 5 - 1, Ws // 3, Hs // 2 + 1, Hs - 3]], np.int32)
    return bo, br, pose, K
