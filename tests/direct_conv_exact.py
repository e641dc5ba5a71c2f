"""Host-side model of the direct convolution stack (csrc/conv_gather.hip, conv_bf16_tiles.hip, conv_first.hip, wgrad.hip and the host
planning in csrc/conv.hip) on data for which the float64 result is the expected value BIT FOR BIT.  No GPU.

These kernels are sums of products with f32 accumulation.  When every operand is an integer (after the rounding the kernel applies)
and  sum |a_i| |b_i| + |bias| + |prior content|  over an output element's whole reduction stays below 2^24, every partial sum, in
whatever order and through whatever split-K slabs it is formed, is an integer below 2^24 and so exact in float32.  LeakyReLU with
slope 0.25 and the weight gradient's scale 0.5 are powers of two: the epilogues are exact too.  assert_exact_domain() checks that
condition for a case before the kernel is called; then np.array_equal with reference() is the test, with no bar.

Data classes (one seeded generator per case, every array read-only):
  ints     activations, dy, y_act in {-3 .. 3}, weights in {-2 .. 2}, bias in {-4 .. 4}
  x_ties   the FIRST operand of the family's product is +-(257 + 2 j), j in 0 .. 7: nine-bit odd integers, each exactly half way
           between two bf16 values, so round-to-nearest-even changes it and (for odd j) truncation gives another value; the second
           operand is in {-1, 0, 1}.  First operand: x (forward, deconvolution, weight gradient); the weights (input gradient)
  w_ties   the roles swapped: the SECOND operand (forward / deconvolution: the weights; gradients: dy / dz) carries the ties
No product ever has ties in both operands.

reference(problem, pipe) is torch's float64 result on the CPU (conv2d, torch.nn.grad.conv2d_input / conv2d_weight, conv_transpose2d +
crop); on the bf16 pipe the operands the kernel rounds go through .float().bfloat16().double() first.  fault(...) returns the
reference with one defect of the kind these kernels can have; tests/test_direct_conv_exact_host.py shows that the sweep sees each.
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.25            # LeakyReLU slope and mask_slope of the folded gradient
SCALE = 0.5             # scale of the OIHW weight-gradient entry
LIMIT = float(1 << 24)
CLASSES = ("ints", "x_ties", "w_ties")
FAMILIES = ("fwd", "dgrad", "wgrad", "deconv")
FAULTS = ("last_column_tap", "phase_extent", "row_tile_padding", "truncation", "wgrad_block", "accumulate_overwrites")

Geometry = collections.namedtuple("Geometry", "k s p")
K3S1, K3S2, K5S2, K7S2 = Geometry(3, 1, 1), Geometry(3, 2, 1), Geometry(5, 2, 2), Geometry(7, 2, 3)
DECONV = Geometry(4, 2, 0)

EDGE = tuple(range(1, 11)) + (15, 16, 17, 31, 32, 33)
SWEEP = tuple((h, w) for h in EDGE for w in EDGE)
SMALL_BATCH = tuple((h, w) for h in (1, 2, 3) for w in (1, 2, 3))      # N = 5: one row tile holds pixels of several images


def out_hw(H, W, g):
    return (H + 2 * g.p - g.k) // g.s + 1, (W + 2 * g.p - g.k) // g.s + 1


# ---------------------------------------------------------------------------------------------------------------- rounding
def rne(a):
    """float64 array -> bf16 (round to nearest even) -> float64: what v_cvt_pk_bf16_f32 and dim_f32_to_bf16 do"""
    return torch.from_numpy(np.array(a, dtype=np.float64)).float().bfloat16().double().numpy()


def truncate(a):
    """float64 array -> bf16 by dropping the low 16 bits of the float32 -> float64: the rounding a kernel must NOT do"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64)


def exact(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- data
def _draw(rng, what, shape):
    if what == "act":
        a = rng.integers(-3, 4, shape)
    elif what == "weight":
        a = rng.integers(-2, 3, shape)
    elif what == "bias":
        a = rng.integers(-4, 5, shape)
    elif what == "unit":
        a = rng.integers(-1, 2, shape)
    elif what == "ties":
        a = (257 + 2 * rng.integers(0, 8, shape)) * (2 * rng.integers(0, 2, shape) - 1)
    else:
        raise ValueError(what)
    a = a.astype(np.float64)
    a.setflags(write=False)
    return a


def _operands(kind):
    """what the first and the second operand of the family's product are drawn from"""
    return {"ints": ("act", "weight"), "x_ties": ("ties", "unit"), "w_ties": ("unit", "ties")}[kind]


class Problem(object):
    """the operands of one case, float64 integers, activations NHWC, weights in the reference layout:
    fwd      x (N,H,W,Cin), w (Cout,Cin,k,k), b (Cout), prior (N,Ho,Wo,Cout)               first operand x, second w
    dgrad    dy (N,Ho,Wo,Cout), w (Cout,Cin,k,k), y_act, prior (N,H,W,Cin), db_prior (Cin)   first operand w, second dy
    wgrad    x (N,H,W,Cin), dz (N,Ho,Wo,Cout), prior (Cout,Cin,k,k)                          first operand x, second dz
    deconv   x (N,H,W,Cin), w (Cin,Cout,4,4), b (Cout); the output window (OH, OW) is an argument of reference()"""

    def __init__(self, family, g, kind, N, H, W, Cin, Cout):
        assert family in FAMILIES and kind in CLASSES
        self.family, self.g, self.kind, self.N, self.H, self.W, self.Cin, self.Cout = family, g, kind, N, H, W, Cin, Cout
        self.key = (family, tuple(g), kind, N, H, W, Cin, Cout)
        rng = np.random.default_rng(zlib.crc32(repr(self.key).encode()))
        first, second = _operands(kind)
        self.Ho, self.Wo = (2 * H + 2, 2 * W + 2) if family == "deconv" else out_hw(H, W, g)
        k = g.k
        if family == "fwd":
            self.x, self.w = _draw(rng, first, (N, H, W, Cin)), _draw(rng, second, (Cout, Cin, k, k))
            self.b, self.prior = _draw(rng, "bias", (Cout,)), _draw(rng, "act", (N, max(self.Ho, 0), max(self.Wo, 0), Cout))
        elif family == "dgrad":
            self.w, self.dy = _draw(rng, "weight" if kind == "ints" else first, (Cout, Cin, k, k)), _draw(rng, "act" if kind == "ints" else second, (N, self.Ho, self.Wo, Cout))
            self.y_act, self.prior, self.db_prior = _draw(rng, "act", (N, H, W, Cin)), _draw(rng, "act", (N, H, W, Cin)), _draw(rng, "bias", (Cin,))
        elif family == "wgrad":
            self.x, self.dz = _draw(rng, "act" if kind == "ints" else first, (N, H, W, Cin)), _draw(rng, "act" if kind == "ints" else second, (N, self.Ho, self.Wo, Cout))
            self.prior = _draw(rng, "weight", (Cout, Cin, k, k))
        else:
            self.x, self.w, self.b = _draw(rng, first, (N, H, W, Cin)), _draw(rng, second, (Cin, Cout, 4, 4)), _draw(rng, "bias", (Cout,))

    def pair(self):
        """(first, second) operand of the product, as the kernel's two matrix operands"""
        f = self.family
        return (self.w, self.dy) if f == "dgrad" else (self.x, self.dz) if f == "wgrad" else (self.x, self.w)


@functools.lru_cache(maxsize=24)
def problem(family, g, kind, N, H, W, Cin, Cout):
    return Problem(family, g, kind, N, H, W, Cin, Cout)


# ---------------------------------------------------------------------------------------------------------------- float64 operations
def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))      # a copy: the problems' arrays are read-only


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def lrelu(a, slope=SLOPE):
    return np.where(a > 0, a, a * slope)


def conv_pre(x, w, b, g):
    """conv(x NHWC, w OIHW) + b, NHWC float64, before the activation"""
    return _nhwc(F.conv2d(_nchw(x), _t(w), None if b is None else _t(b), stride=g.s, padding=g.p))


def conv_input_grad(dy, w, g, H, W):
    N, Cin = dy.shape[0], w.shape[1]
    return _nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), _t(w), _nchw(dy), stride=g.s, padding=g.p))


def conv_weight_grad(x, dz, g, Cin, Cout):
    return torch.nn.grad.conv2d_weight(_nchw(x), (Cout, Cin, g.k, g.k), _nchw(dz), stride=g.s, padding=g.p).numpy()


def deconv_pre(x, w, b, OH, OW, crop=1):
    full = F.conv_transpose2d(_nchw(x), _t(w), None if b is None else _t(b), stride=2)
    return _nhwc(full[:, :, crop:crop + OH, crop:crop + OW])


# ---------------------------------------------------------------------------------------------------------------- reference
def _rounders(pipe, rounding):
    """pipe "f32": nothing is rounded (also conv1's three-term path, which is exact on these integers); "bf16": both matrix operands
    are (activations on their way into LDS, weights through to_bf16 of the packed array; the bf16 weight gradient: x and dz)"""
    assert pipe in ("f32", "bf16")
    return (exact, exact) if pipe == "f32" else (rounding, rounding)


@functools.lru_cache(maxsize=48)
def _reference(p, pipe, rounding, variant):
    r1, r2 = _rounders(pipe, rounding)
    a, b = p.pair()
    a, b = r1(a), r2(b)
    f, g = p.family, p.g
    if f == "fwd":
        out = lrelu(conv_pre(a, b, p.b, g))
    elif f == "dgrad":
        out = conv_input_grad(b, a, g, p.H, p.W)
    elif f == "wgrad":
        out = conv_weight_grad(a, b, g, p.Cin, p.Cout)
    else:
        OH, OW = variant
        out = lrelu(deconv_pre(a, b, p.b, OH, OW))
    out.setflags(write=False)
    return out


def reference(p, pipe="f32", accumulate=False, window=None, rounding=rne):
    """the expected output of one call, float64, read-only: fwd y (N,Ho,Wo,Cout) = LeakyReLU_0.25(conv + b) [+ prior]; dgrad dx
    (N,H,W,Cin) [+ prior]; wgrad dW (Cout,Cin,k,k) [+ prior]; deconv y (N,OH,OW,Cout) for window = (OH, OW), crop 1.
    Cached per (family, geometry, class, size, pipe): the tiles of one geometry share it"""
    out = _reference(p, pipe, rounding, window)
    if accumulate:
        out = out + p.prior
        out.setflags(write=False)
    return out


def folded(p, pipe="bf16", accumulate_db=False, rounding=rne):
    """dim_conv2d_dgrad_bf16_lrelu: dz = dX * (y_act > 0 ? 1 : 0.25) and db (+)= its column sums (multiples of 1/4, exact)"""
    dz = reference(p, pipe, rounding=rounding) * np.where(p.y_act > 0, 1.0, SLOPE)
    db = dz.sum((0, 1, 2)) + (p.db_prior if accumulate_db else 0.0)
    return dz, db


# ---------------------------------------------------------------------------------------------------------------- the exact domain
@functools.lru_cache(maxsize=8)
def _magnitude(p, pipe, window, rounding):
    r1, r2 = _rounders(pipe, rounding)
    a, b = p.pair()
    a, b = np.abs(r1(a)), np.abs(r2(b))
    f, g = p.family, p.g
    if f == "fwd":
        return conv_pre(a, b, np.abs(p.b), g)
    if f == "dgrad":
        return conv_input_grad(b, a, g, p.H, p.W)
    if f == "wgrad":
        return conv_weight_grad(a, b, g, p.Cin, p.Cout)
    return deconv_pre(a, b, np.abs(p.b), *window)


def magnitude(p, pipe="f32", accumulate=False, window=None, fold=False, rounding=rne):
    """per output element: sum |a_i| |b_i| over the whole reduction + |bias| + |prior| (what the element's partial sums are bounded by).
    fold: the bound of 4 db, the column sums of dz in units of 1/4, behind them"""
    m = _magnitude(p, pipe, window, rounding)
    if accumulate:
        m = m + np.abs(p.prior)
    if fold:
        m = np.concatenate([m.reshape(-1), 4.0 * (m.sum((0, 1, 2)) + np.abs(p.db_prior))])
    return m


def assert_exact_domain(p, pipe="f32", accumulate=False, window=None, fold=False, rounding=rne, limit=LIMIT):
    """the condition under which equality with reference() is legitimate; -> the largest bound of the case"""
    r1, r2 = _rounders(pipe, rounding)
    a, b = p.pair()
    extra = [p.b] if p.family in ("fwd", "deconv") else [p.prior] + ([p.y_act, p.db_prior] if p.family == "dgrad" else [])
    for name, v in (("first operand", r1(a)), ("second operand", r2(b))) + tuple(("other", e) for e in extra):
        assert np.array_equal(v, np.round(v)), "{}: {} is not all integers".format(p.key, name)
    tie = lambda v: bool(np.any(np.abs(v) > 255))
    assert not (tie(a) and tie(b)), "{}: ties in both operands of one product".format(p.key)
    m = magnitude(p, pipe, accumulate, window, fold, rounding)
    worst = float(m.max()) if m.size else 0.0
    assert worst < limit, "{}: sum |a||b| + |bias| + |prior| reaches {:.4g} >= {:.4g}: outside the exact domain".format(p.key, worst, limit)
    return worst


# ---------------------------------------------------------------------------------------------------------------- faults
def _row_tile_padding(p, a, b, rows):
    """forward: GEMM rows m = (n, ho, wo) in tiles of `rows`; a tile takes the image of its first row for the padding test of all its
    rows, so a row of a later image is tested at ho + (n - n0) Ho and loses every tap whose input row then falls outside [0, H)"""
    g, N, Ho, Wo = p.g, p.N, p.Ho, p.Wo
    per_kh = []
    for kh in range(g.k):
        wk = np.zeros_like(b)
        wk[:, :, kh, :] = b[:, :, kh, :]
        per_kh.append(conv_pre(a, wk, None, g))
    out = np.zeros_like(per_kh[0])
    for m in range(N * Ho * Wo):
        n, ho, wo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
        n0 = (m // rows * rows) // (Ho * Wo)
        for kh in range(g.k):
            hi = (ho + (n - n0) * Ho) * g.s - g.p + kh
            if 0 <= hi < p.H or n == n0:
                out[n, ho, wo] += per_kh[kh][n, ho, wo]
    return lrelu(out + p.b)


def fault(name, p, pipe="f32", accumulate=False, rows=64):
    """reference(p, pipe, accumulate) with one defect:
    last_column_tap        fwd: the last output column loses the tap that reads the image's last column
    phase_extent           dgrad, stride 2: the even row phase is computed with the odd phase's extent H / 2, so for odd H its last
                           row, H - 1, is never written (stays 0; with accumulate: stays the prior content)
    row_tile_padding       fwd: see _row_tile_padding
    truncation             bf16 pipe: operands truncated to bf16, not rounded to nearest even
    wgrad_block            wgrad: the 8 x 8 pixel block at the bottom right of the last image is left out
    accumulate_overwrites  an accumulate call that stores the result over the prior content"""
    assert name in FAULTS
    f, g = p.family, p.g
    if name == "truncation":
        return reference(p, pipe, accumulate, rounding=truncate)
    if name == "accumulate_overwrites":
        return reference(p, pipe, False)
    r1, r2 = _rounders(pipe, rne)
    a, b = p.pair()
    a, b = r1(a), r2(b)
    out = np.array(reference(p, pipe, False))
    if name == "last_column_tap":
        assert f == "fwd"
        wo = p.Wo - 1
        kw = p.W - 1 - (wo * g.s - g.p)             # the tap of the last output column that reads input column W - 1
        pre = conv_pre(a, b, p.b, g)
        if 0 <= kw < g.k:
            wk = np.zeros_like(b)
            wk[:, :, :, kw] = b[:, :, :, kw]
            pre[:, :, wo] -= conv_pre(a, wk, None, g)[:, :, wo]
        out = lrelu(pre)
    elif name == "phase_extent":
        assert f == "dgrad" and g.s == 2
        if p.H % 2:
            out[:, p.H - 1] = 0.0
    elif name == "row_tile_padding":
        assert f == "fwd"
        out = _row_tile_padding(p, a, b, rows)
    elif name == "wgrad_block":
        assert f == "wgrad"
        dz = np.array(b)
        dz[-1, (p.Ho - 1) // 8 * 8:, (p.Wo - 1) // 8 * 8:] = 0.0
        out = conv_weight_grad(a, dz, g, p.Cin, p.Cout)
    return out + p.prior if accumulate else out


def packed_floats(Cin, Cout, k):
    """the packed weights dim_conv2d_wgrad writes: chunks of 32 x Cout (behind them a first-layer buffer holds the three-term image)"""
    return (-(-k * k // 4) if Cin == 8 else k * k * (Cin // 32)) * 32 * Cout


def packed(w):
    """(Cout, Cin, k, k) -> the packed layout restated with numpy indexing: [chunk][Cout][32], a chunk = (32-channel slice, kh, kw) for
    Cin % 32 == 0; for Cin 8 a chunk = 4 taps x 8 channels, the taps flat over kh x kw and the last chunk padded with zero taps"""
    w = np.asarray(w)
    cout, cin, kh, kw = w.shape
    if cin == 8:
        taps = -(-kh * kw // 4) * 4
        wt = np.zeros((cout, taps, 8), dtype=w.dtype)
        wt[:, :kh * kw] = w.reshape(cout, 8, kh * kw).transpose(0, 2, 1)
        return wt.reshape(cout, taps // 4, 32).transpose(1, 0, 2).reshape(-1)
    return w.reshape(cout, cin // 32, 32, kh * kw).transpose(1, 3, 0, 2).reshape(-1)


def mismatch(got, want):
    """-> None when got == want numerically everywhere (-0.0 == 0.0), else (count, first index, got there, wanted there)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(~(got == want))
    i = tuple(int(v) for v in bad[0])
    return len(bad), i, float(got[i]), float(want[i])
