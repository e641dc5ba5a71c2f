"""The Winograd layers of csrc/winograd.hip and csrc/wino_s2.hip restated in numpy, the number format a parameter (no GPU, no HIP):
written from the matrices and index rules in the headers of those two files.  Every family runs in the kernels' three stages

    input transform -> V (P, T, K)      weight transform -> U (P, K, Nout)      per-plane product M = V . U      output transform

with the product a callable (test_split_terms.six_product_dot / f32_pipe_dot: the two arithmetics of the plane GEMMs; default: a
float64 product rounded once to dt).  With dt = float64 each family IS the convolution (tests/test_wino_reference_host.py: 1e-11 of
max|ref| against torch's float64 conv2d / autograd); with dt = float32 it is the model whose worst element sets the bar of
tests/test_gpu_wino_layers.py.  Maps are NHWC, weights (Cout, Cin, k, k), as the library takes them.

Transforms are applied one axis at a time (rows, then columns: the kernels' order), each output a left-to-right sum of coefficient x
value in dt with the zero coefficients left out.  The kernels contract some of these into FMAs and group a few sums differently
(DIM_WINO4_AT's s1 / d1, DIM_WINO4_G4's ev_ / od_); the factor of the GPU bar covers that.

Defects for the negative controls, all off by default:
    mats        replaces BT / G / AT of the family (one coefficient scaled)
    v_hook      V (P, T, K) -> V, applied before the product (one plane rounded to bf16)
    border      "edge": pixels outside the map replicate the nearest edge pixel instead of being zero
    swap_phase  5x5 / stride-2 families: py and px exchanged in the phase-major channel order of one side of the product"""
import numpy as np

_ = np.array
# F(2x2, 3x3): points {0, 1, -1, inf}
F23 = dict(BT=_([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
           G=_([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
           AT=_([[1., 1, 1, 0], [0, 1, -1, -1]]))
# F(4x4, 3x3): points {0, 1, -1, 2, -1/2, inf}
F43 = dict(BT=_([[1., 1.5, -2, -1.5, 1, 0], [0, -1, -2.5, -.5, 1, 0], [0, 1, .5, -2.5, 1, 0], [0, -.5, -1, .5, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 1, 1.5, -2, -1.5, 1]]),
           G=_([[1., 0, 0], [-1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3], [1 / 15, 2 / 15, 4 / 15], [-16 / 15, 8 / 15, -4 / 15], [0, 0, 1]]),
           AT=_([[1., 1, 1, 1, 1, 0], [0, 1, -1, 2, -.5, 0], [0, 1, 1, 4, .25, 0], [0, 1, -1, 8, -.125, 1]]))
# F(3x3, 4x4), the weight gradient: BT = the forward's (its V), G = G4 on the 4x4 tile of dY, AT = A3^T
F34 = dict(BT=F43["BT"],
           G=_([[1., 0, 0, 0], [-1 / 3, -1 / 3, -1 / 3, -1 / 3], [1 / 3, -1 / 3, 1 / 3, -1 / 3], [1 / 15, 2 / 15, 4 / 15, 8 / 15],
                [-16 / 15, 8 / 15, -4 / 15, 2 / 15], [0, 0, 0, 1]]),
           AT=_([[1., 1, 1, 1, 1, 0], [0, 1, -1, 2, -.5, 0], [0, 1, 1, 4, .25, 1]]))
# F(4, 2) of the odd phase of a 3x3 / stride-2 axis: points {0, 1, -1, 2, inf}
F42 = dict(BT=_([[2., -1, -2, 1, 0], [0, 2, 1, -1, 0], [0, -2, 3, -1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]]),
           G=_([[.5, 0], [.5, .5], [1 / 6, -1 / 6], [1 / 6, 1 / 3], [0, 1]]),
           AT=_([[1., 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 0], [0, 1, -1, 8, 1]]))
del _

FAMILIES = ("f2x2", "f4x4", "conv5x5s2", "dgrad5x5s2", "wgrad_s1", "wgrad_s2", "conv3x3s2")
INPUT_CLASSES = ("randn", "lrelu", "dc", "sparse")


# ------------------------------------------------------------------------------------------------------------------------ the stages
def apply(mat, d, axis, dt):
    """sum_j mat[i][j] d[j] along `axis`, in dt, left to right, zero coefficients left out"""
    d = np.moveaxis(np.asarray(d, dt), axis, 0)
    out = []
    for row in np.asarray(mat):
        acc = None
        for c, v in zip(row, d):
            if c != 0:
                acc = dt(c) * v if acc is None else acc + dt(c) * v
        out.append(np.zeros(d.shape[1:], dt) if acc is None else acc)
    return np.moveaxis(np.stack(out), 0, axis)


def transform2d(my, mx, d, dt):
    """my d mx^T on the axes (-3, -2) of d (..., ny, nx, C): rows first, as every kernel here"""
    return apply(mx, apply(my, d, -3, dt), -2, dt)


def idx(nt, n, step, off, S, p):
    """(nt, n) pixel index of point a of tile t along one axis: S (step t + off + a) + p"""
    return S * (step * np.arange(nt)[:, None] + off + np.arange(n)[None, :]) + p


def gather(x, rows, cols, border="zero"):
    """x (N, H, W, C) -> (N, th, tw, ny, nx, C) for rows (th, ny), cols (tw, nx); outside the map: zero, or the edge pixel"""
    H, W = x.shape[1:3]
    oky, okx = (rows >= 0) & (rows < H), (cols >= 0) & (cols < W)
    d = x[:, np.clip(rows, 0, H - 1)[:, None, :, None], np.clip(cols, 0, W - 1)[None, :, None, :], :]
    if border == "zero":
        d = np.where((oky[:, None, :, None] & okx[None, :, None, :])[None, ..., None], d, x.dtype.type(0))
    else:
        assert border == "edge", border
    return d


def planes(d):
    """(N, th, tw, ny, nx, C) -> (ny nx, T, C), T = N th tw"""
    ny, nx, C = d.shape[3:]
    return d.transpose(3, 4, 0, 1, 2, 5).reshape(ny * nx, -1, C)


def unplanes(M, ny, nx, N, th, tw):
    return M.reshape(ny, nx, N, th, tw, -1).transpose(2, 3, 4, 0, 1, 5)


def untile(Y):
    """(N, th, tw, m, m', C) -> (N, th m, tw m', C)"""
    N, th, tw, my, mx, C = Y.shape
    return Y.transpose(0, 1, 3, 2, 4, 5).reshape(N, th * my, tw * mx, C)


def weights(Gy, Gx, g, wdt, dt):
    """g (O, I, ry, rx) -> U (ny nx, I, O) = Gy g Gx^T per (o, i), in wdt (float64: the F(4x4) and stride-2 pack kernels; the F(2x2) pack
    kernel works in f32), rounded once to dt"""
    u = apply(Gx, apply(Gy, np.asarray(g, wdt), 2, wdt), 3, wdt).astype(dt)
    return u.transpose(2, 3, 1, 0).reshape(u.shape[2] * u.shape[3], g.shape[1], g.shape[0])


def exact_dot(dt):
    """the default product: float64, rounded once to dt"""
    return lambda V, U: np.matmul(np.asarray(V, np.float64), np.asarray(U, np.float64)).astype(dt)


def padded(dot, mult=16):
    """dot for a contraction length that is no multiple of the model's k-step: zeros appended (they add nothing to any sum)"""
    def f(V, U):
        K = V.shape[-1]
        pad = -K % mult
        if pad:
            V = np.concatenate([V, np.zeros(V.shape[:-1] + (pad,), V.dtype)], axis=-1)
            U = np.concatenate([U, np.zeros(U.shape[:-2] + (pad, U.shape[-1]), U.dtype)], axis=-2)
        return dot(V, U)
    return f


def _products(dot, V, U, v_hook, dt):
    """M per product callable: dot may be one callable (or None) or a tuple of them -- the transforms then run once for all"""
    if v_hook is not None:
        V = np.asarray(v_hook(V), dt)
    dots = dot if isinstance(dot, (tuple, list)) else (dot,)
    return [np.asarray((d or exact_dot(dt))(V, U), dt) for d in dots]


def _result(outs, dot):
    return tuple(outs) if isinstance(dot, (tuple, list)) else outs[0]


def finish(y, b, slope, dt):
    if b is not None:
        y = y + np.asarray(b, dt)
    return np.where(y > 0, y, y * dt(slope)) if slope != 1.0 else y


def _mats(base, mats):
    return dict(base, **(mats or {}))


# ------------------------------------------------------------------------------------------------------------------------ the families
def conv3x3(x, w, b=None, slope=1.0, m=4, dt=np.float32, dot=None, mats=None, v_hook=None, border="zero"):
    """3x3 / stride 1 / pad 1 through F(m x m, 3x3), m = 2 or 4: tiles of m + 2 points at stride m from pixel -1"""
    mt = _mats(F23 if m == 2 else F43, mats)
    N, H, W, C = x.shape
    th, tw, n = -(-H // m), -(-W // m), m + 2
    V = planes(transform2d(mt["BT"], mt["BT"], gather(np.asarray(x, dt), idx(th, n, m, -1, 1, 0), idx(tw, n, m, -1, 1, 0), border), dt))
    U = weights(mt["G"], mt["G"], w, dt if m == 2 else np.float64, dt)
    outs = [finish(untile(transform2d(mt["AT"], mt["AT"], unplanes(M, n, n, N, th, tw), dt))[:, :H, :W], b, slope, dt)
            for M in _products(dot, V, U, v_hook, dt)]
    return _result(outs, dot)


PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))      # (py, px) of phase 2 py + px


def _phase_order(swap):
    return (0, 2, 1, 3) if swap else (0, 1, 2, 3)


def _phase_tiles(x, th, tw, mt, dt, border, swap):
    """V (36, T, 4 C) of the four phase images X^(py,px)[r][q] = x[2r + py][2q + px], phase-major"""
    Vs = [planes(transform2d(mt["BT"], mt["BT"], gather(x, idx(th, 6, 4, -1, 2, py), idx(tw, 6, 4, -1, 2, px), border), dt)) for py, px in PHASES]
    return np.concatenate([Vs[i] for i in _phase_order(swap)], axis=2)


def _sub_kernel(w, py, px, flip=False):
    """g[u][v] = w[2u + py][2v + px] (flip: u, v -> 2 - u, 2 - v), zero beyond the 5 taps"""
    g = np.zeros(w.shape[:2] + (3, 3), w.dtype)
    for u in range(3):
        for v in range(3):
            i, j = 2 * (2 - u if flip else u) + py, 2 * (2 - v if flip else v) + px
            if i < 5 and j < 5:
                g[:, :, u, v] = w[:, :, i, j]
    return g


def conv5x5s2(x, w, b=None, slope=1.0, dt=np.float32, dot=None, mats=None, v_hook=None, border="zero", swap_phase=False):
    """5x5 / stride 2 / pad 2 as the sum of four 3x3 / stride-1 / pad-1 convolutions of the phase images: K = 4 Cin, phase-major"""
    mt = _mats(F43, mats)
    N, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    th, tw = -(-Ho // 4), -(-Wo // 4)
    V = _phase_tiles(np.asarray(x, dt), th, tw, mt, dt, border, swap_phase)
    U = np.concatenate([weights(mt["G"], mt["G"], _sub_kernel(w, py, px), np.float64, dt) for py, px in PHASES], axis=1)
    outs = [finish(untile(transform2d(mt["AT"], mt["AT"], unplanes(M, 6, 6, N, th, tw), dt))[:, :Ho, :Wo], b, slope, dt)
            for M in _products(dot, V, U, v_hook, dt)]
    return _result(outs, dot)


def dgrad5x5s2(dy, w, H, W, dt=np.float32, dot=None, mats=None, v_hook=None, border="zero", swap_phase=False):
    """dX (N, H, W, Cin) of the 5x5 / stride-2 layer: one F(4x4, 3x3) transform of dY, K = Cout, N = 4 Cin phase-major with the flipped
    sub-kernels, the 4x4 block of phase (py, px) scattered to the pixels (2r + py, 2q + px)"""
    mt = _mats(F43, mats)
    N, Ho, Wo, Co = dy.shape
    assert (Ho, Wo) == ((H + 1) // 2, (W + 1) // 2)
    Ci = w.shape[1]
    th, tw = -(-Ho // 4), -(-Wo // 4)
    V = planes(transform2d(mt["BT"], mt["BT"], gather(np.asarray(dy, dt), idx(th, 6, 4, -1, 1, 0), idx(tw, 6, 4, -1, 1, 0), border), dt))
    Us = [weights(mt["G"], mt["G"], _sub_kernel(w, py, px, flip=True).transpose(1, 0, 2, 3), np.float64, dt) for py, px in PHASES]
    U = np.concatenate([Us[i] for i in _phase_order(swap_phase)], axis=2)
    outs = []
    for M in _products(dot, V, U, v_hook, dt):
        Y = untile(transform2d(mt["AT"], mt["AT"], unplanes(M, 6, 6, N, th, tw), dt))
        dx = np.zeros((N, H, W, Ci), dt)
        for ph, (py, px) in enumerate(PHASES):
            part = dx[:, py::2, px::2]
            part[...] = Y[:, :part.shape[1], :part.shape[2], ph * Ci:(ph + 1) * Ci]
        outs.append(dx)
    return _result(outs, dot)


def wgrad(x, dy, S=1, dt=np.float32, dot=None, mats=None, v_hook=None, border="zero", swap_phase=False):
    """dW (Cout, Cin, k, k) through F(3x3, 4x4) per 4x4 tile of dY: V = the forward's input transform (S = 2: of the phase images),
    D = G4 g G4^T, dM[p] = sum over tiles and batch V[p]^T D[p], dW = A3^T dM A3; S = 2: the 3x3 of phase (py, px) are the taps
    (2u + py, 2v + px) of the 5x5 gradient.  The contraction runs over T: wrap a model product in padded()."""
    mt = _mats(F34, mats)
    N, H, W, C = x.shape
    Ho, Wo, Co = dy.shape[1:]
    assert (Ho, Wo) == ((H, W) if S == 1 else ((H + 1) // 2, (W + 1) // 2))
    th, tw = -(-Ho // 4), -(-Wo // 4)
    x = np.asarray(x, dt)
    if S == 1:
        V = planes(transform2d(mt["BT"], mt["BT"], gather(x, idx(th, 6, 4, -1, 1, 0), idx(tw, 6, 4, -1, 1, 0), border), dt))
    else:
        V = _phase_tiles(x, th, tw, mt, dt, border, swap_phase)
    D = planes(transform2d(mt["G"], mt["G"], gather(np.asarray(dy, dt), idx(th, 4, 4, 0, 1, 0), idx(tw, 4, 4, 0, 1, 0), border), dt))
    if v_hook is not None:
        V = np.asarray(v_hook(V), dt)
    outs = []
    for dM in _products(dot, V.transpose(0, 2, 1), D, None, dt):                                      # (36, K, Co)
        R = transform2d(mt["AT"], mt["AT"], dM.reshape(6, 6, -1, Co).transpose(2, 3, 0, 1)[..., None], dt)[..., 0]   # (K, Co, 3, 3)
        if S == 1:
            dw = np.ascontiguousarray(R.transpose(1, 0, 2, 3))
        else:
            dw = np.zeros((Co, C, 5, 5), dt)
            for ph, (py, px) in enumerate(PHASES):
                part = dw[:, :, py::2, px::2]
                part[...] = R[ph * C:(ph + 1) * C].transpose(1, 0, 2, 3)[:, :, :part.shape[2], :part.shape[3]]
        outs.append(dw)
    return _result(outs, dot)


def conv3x3s2(x, w, b=None, slope=1.0, dt=np.float32, dot=None, mats=None, v_hook=None, border="zero"):
    """3x3 / stride 2 / pad 1 through its phase images: per axis the even phase E[r] = x[2r] meets the tap w1 (identity on 4 points), the
    odd phase O[r] = x[2r + 1] the taps w0, w2 (F(4, 2), 5 points from O[i0 - 1]).  81 planes: ee 16, eo 20, oe 20, oo 25.
    (tools/wino_s2_proto.py is the prototype of this algorithm; here it takes the product callable and the defects of the controls.)"""
    mt = _mats(F42, mats)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    th, tw = -(-Ho // 4), -(-Wo // 4)
    I4, ONE = np.eye(4), np.ones((4, 1))
    axis = {0: (I4, ONE, I4, [1], 0, 0), 1: (mt["BT"], mt["G"], mt["AT"], [0, 2], -1, 1)}      # BT, G, AT, taps, first point, phase
    x = np.asarray(x, dt)
    Vs, Us = [], []
    for py, px in PHASES:
        (By, Gy, _, ty, oy, qy), (Bx, Gx, _, tx, ox, qx) = axis[py], axis[px]
        Vs.append(planes(transform2d(By, Bx, gather(x, idx(th, len(By), 4, oy, 2, qy), idx(tw, len(Bx), 4, ox, 2, qx), border), dt)))
        Us.append(weights(Gy, Gx, w[:, :, ty][:, :, :, tx], np.float64, dt))
    V, U = np.concatenate(Vs, axis=0), np.concatenate(Us, axis=0)
    outs = []
    for M in _products(dot, V, U, v_hook, dt):
        acc, p0 = None, 0
        for py, px in PHASES:                    # the kernel's order: ee, + eo, + oe, + oo
            Ay, Ax = axis[py][2], axis[px][2]
            ny, nx = Ay.shape[1], Ax.shape[1]
            Y = transform2d(Ay, Ax, unplanes(M[p0:p0 + ny * nx], ny, nx, N, th, tw), dt)
            acc, p0 = Y if acc is None else acc + Y, p0 + ny * nx
        outs.append(finish(untile(acc)[:, :Ho, :Wo], b, slope, dt))
    return _result(outs, dot)


# ------------------------------------------------------------------------------------------------------------------------ references
def _t(a, perm):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(*perm)


def ref_conv(x, w, b, k, stride, slope=1.0):
    """torch's float64 conv2d of the same numbers, NHWC; pad = k // 2"""
    import torch.nn.functional as F

    y = F.conv2d(_t(x, (0, 3, 1, 2)), _t(w, (0, 1, 2, 3)), None if b is None else _t(b, (0,)), stride=stride, padding=k // 2)
    return F.leaky_relu(y, slope).permute(0, 2, 3, 1).numpy()


def ref_dgrad(dy, w, H, W, stride):
    import torch.nn.functional as F

    k = w.shape[2]
    xs = _t(np.zeros((dy.shape[0], H, W, w.shape[1])), (0, 3, 1, 2)).requires_grad_(True)
    F.conv2d(xs, _t(w, (0, 1, 2, 3)), None, stride=stride, padding=k // 2).backward(_t(dy, (0, 3, 1, 2)))
    return xs.grad.permute(0, 2, 3, 1).numpy()


def ref_wgrad(x, dy, k, stride):
    import torch.nn.functional as F

    ws = _t(np.zeros((dy.shape[3], x.shape[3], k, k)), (0, 1, 2, 3)).requires_grad_(True)
    F.conv2d(_t(x, (0, 3, 1, 2)), ws, None, stride=stride, padding=k // 2).backward(_t(dy, (0, 3, 1, 2)))
    return ws.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------------ the measure
def _per_unit(got, ref, unit):
    diff = np.abs(np.asarray(got).astype(np.float64) - ref)
    # a tile whose every product is zero has to be exactly zero
    return np.where(unit > 0, diff / np.where(unit > 0, unit, 1.0), np.where(diff == 0, 0.0, np.inf))


def tile_max(unit, my, mx):
    """(N, H, W, C): every element replaced by the maximum over its own my x mx tile (tiles from pixel 0, the last ones partial)"""
    N, H, W, C = unit.shape
    th, tw = -(-H // my), -(-W // mx)
    u = np.zeros((N, th * my, tw * mx, C), unit.dtype)
    u[:, :H, :W] = unit
    u = u.reshape(N, th, my, tw, mx, C)
    return np.broadcast_to(u.max(axis=(2, 4), keepdims=True), u.shape).reshape(N, th * my, tw * mx, C)[:, :H, :W]


def map_error(got, ref, unit, tile):
    """|got - ref| / unit per element of an NHWC map, unit = the maximum of conv(|x|, |w|) + |b| over the element's own output tile: a
    Winograd output carries the rounding of its whole tile"""
    return _per_unit(got, ref, tile_max(unit, tile, tile))


def taps_error(got, ref, unit, wide=None):
    """the same for a weight gradient (Cout, Cin, k, k): unit = the maximum over the taps of the element's (co, ci) pair.
    wide (the sparse class): the maximum runs over every offset two pixels of one tile can have (wide_unit), the taps among them.
    Unlike a map, a weight gradient does not carry the rounding of its own taps' products alone: a pixel of X and a pixel of dY of the
    same tile that no tap pairs (offset outside the kernel) still meet in V (.) D and cancel only in exact arithmetic.  On dense data
    every offset sums about the same and the taps' maximum stands for all; on sparse data a pair whose taps meet one small product, or
    none, sits next to large products at other offsets, and the f32 model itself is then 1e-4 or infinite in the taps' unit.  Where
    the wide unit is zero, V or D of every tile is zero and dW must be an exact zero."""
    u = unit.max(axis=(2, 3), keepdims=True)
    if wide is not None:
        u = np.maximum(u, wide.max(axis=(2, 3), keepdims=True))
    return _per_unit(got, ref, np.broadcast_to(u, unit.shape))


def wide_unit(x, dy, S):
    """sum |x| |dy| per pixel offset, over every offset two pixels of one tile can have: x row 4 ty - 1 + a (a < 6) against dY row 4 ty + i
    (i < 4) is -4 .. 4 (S = 2, phase images: 2 (a - i - 1) + py = -8 .. 9, inside a 19-tap window)"""
    return ref_wgrad(np.abs(x), np.abs(dy), 9 if S == 1 else 19, S)


# ------------------------------------------------------------------------------------------------------------------------ the data
def make_input(kind, rng, shape):
    """one NHWC map of an input class, float32"""
    x = rng.standard_normal(shape)
    if kind == "lrelu":
        x = np.where(x > 0, x, 0.1 * x)
    elif kind == "dc":
        x = x + 8.0
    elif kind == "sparse":      # about 2 % of the (pixel, channel) entries: a quarter of the channels of 8 % of the pixels, so that whole
        #                         tiles stay zero (spread evenly, 2 % leave no 6 x 6 tile of 32 channels empty); the last image all zero
        x = np.where((rng.random(shape[:3] + (1,)) < 0.08) & (rng.random(shape) < 0.25), x, 0.0)
        if shape[0] > 1:
            x[-1] = 0.0
    else:
        assert kind == "randn", kind
    return x.astype(np.float32)


def make_weights(rng, Cout, Cin, k, fan=None):
    return (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(k * k * (fan or Cin))).astype(np.float32)


class Case(object):
    """one problem of a family: data, float64 reference, unit, and run(dt=, dot=, defects) of the numpy model on it.  Read-only."""

    def __init__(self, family, kind, N, H, W, Cin, Cout, seed, bias=True, slope=0.1):
        assert family in FAMILIES and kind in INPUT_CLASSES
        rng = np.random.default_rng(seed)
        self.family, self.kind, self.shape = family, kind, (N, H, W, Cin, Cout)
        self.k = k = 5 if family in ("conv5x5s2", "dgrad5x5s2", "wgrad_s2") else 3
        self.stride = s = 1 if family in ("f2x2", "f4x4", "wgrad_s1") else 2
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        self.out_hw = (Ho, Wo)
        self.b, self.slope = None, 1.0
        if family in ("wgrad_s1", "wgrad_s2"):
            self.x = make_input(kind, rng, (N, H, W, Cin))
            self.dy = (make_input(kind if kind == "sparse" else "randn", rng, (N, Ho, Wo, Cout)) / np.sqrt(N * Ho * Wo)).astype(np.float32)
            self.ref = ref_wgrad(self.x, self.dy, k, s)
            self.unit = ref_wgrad(np.abs(self.x), np.abs(self.dy), k, s)
            self.wide = wide_unit(self.x, self.dy, s) if kind == "sparse" else None
        elif family == "dgrad5x5s2":
            self.dy = make_input(kind, rng, (N, Ho, Wo, Cout))
            self.w = make_weights(rng, Cout, Cin, k)
            self.ref = ref_dgrad(self.dy, self.w, H, W, s)
            self.unit = ref_dgrad(np.abs(self.dy), np.abs(self.w), H, W, s)
        else:
            self.x = make_input(kind, rng, (N, H, W, Cin))
            self.w = make_weights(rng, Cout, Cin, k)
            if bias and kind != "sparse":
                self.b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
            self.slope = slope
            self.ref = ref_conv(self.x, self.w, self.b, k, s, slope)
            self.unit = ref_conv(np.abs(self.x), np.abs(self.w), None if self.b is None else np.abs(self.b), k, s)
        for a in (getattr(self, n, None) for n in ("x", "dy", "w", "b", "ref", "unit")):
            if a is not None:
                a.setflags(write=False)

    def run(self, dt=np.float32, dot=None, **defects):
        f = self.family
        H, W = self.shape[1:3]
        if f in ("f2x2", "f4x4"):
            return conv3x3(self.x, self.w, self.b, self.slope, 2 if f == "f2x2" else 4, dt, dot, **defects)
        if f == "conv5x5s2":
            return conv5x5s2(self.x, self.w, self.b, self.slope, dt, dot, **defects)
        if f == "conv3x3s2":
            return conv3x3s2(self.x, self.w, self.b, self.slope, dt, dot, **defects)
        if f == "dgrad5x5s2":
            return dgrad5x5s2(self.dy, self.w, H, W, dt, dot, **defects)
        if isinstance(dot, (tuple, list)):
            dot = tuple(padded(d) if d else d for d in dot)
        elif dot is not None:
            dot = padded(dot)
        return wgrad(self.x, self.dy, self.stride, dt, dot, **defects)

    def error(self, got):
        """per element, in units of the element's output tile (see map_error / taps_error)"""
        f = self.family
        if f in ("wgrad_s1", "wgrad_s2"):
            return taps_error(got, self.ref, self.unit, self.wide)
        return map_error(got, self.ref, self.unit, 2 if f == "f2x2" else 8 if f == "dgrad5x5s2" else 4)
