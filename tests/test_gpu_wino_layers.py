"""The Winograd layers (csrc/winograd.hip, csrc/wino_s2.hip: input transform, plane GEMMs, output transform) against torch's float64
convolution of the same f32 numbers, PER OUTPUT ELEMENT in units of the element's own output tile (tests/wino_reference.py: map_error,
taps_error), on every input class and on every small map.

Bar: BAR_FACTOR x the worst element of the numpy model of the same family on the same data (wino_reference.Case.run), its plane
product six_product_dot where the three-term kernel runs (split on and GEMM tile 4, 5 or 7) and f32_pipe_dot where the f32 pipe runs
(split off, or tile 3 / 6, which have no three-term kernel; the weight gradient's plane product is the f32 wgrad kernel whatever the
switch).  tests/test_wino_reference_host.py shows on the model what this bar catches and the layer tests' 1e-4 max|ref| + 2e-5 does not.

Every call writes into a 7.0-filled wider buffer (channels outside the window must keep their 7.0), reads inputs whose pad channels are
NaN, and works in a NaN workspace of exactly the queried size with 7.0-filled guard words behind it.

The small-map sweeps take the layer's default GEMM tile at Cout = 64, which is tile 3: the f32 pipe under either switch (both are run
and must agree bit for bit).  So that the three-term kernel meets every small map too, each size runs once more at Cout = 128 on
tile 7 with the switch on.

Measured on an MI355X: DESIGN.md, "The Winograd layers pinned per output element"."""
import numpy as np
import pytest
import torch

import wino_reference as wr
from test_split_terms import BAR_FACTOR, f32_pipe_dot, six_product_dot

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPLIT_TILES = (4, 5, 7)
PAD_IN, PAD_OUT, COFF, GUARD = 8, 16, 4, 4096
FORWARD = ("f2x2", "f4x4", "conv5x5s2", "conv3x3s2")
REFUSED = {f: () for f in wr.FAMILIES}      # (H, W) the library refuses with DIM_ERR_ARG, per family: none
S1_SIZES = [(h, w) for h in range(1, 10) for w in range(1, 10)]
S2_EDGE = tuple(range(1, 11)) + (15, 16, 17)
S2_SIZES = [(h, w) for h in S2_EDGE for w in S2_EDGE]


@pytest.fixture
def arithmetic(hip_lib):
    """sets the arithmetic of the plane GEMMs for the calls of one test; the default (three terms) is back afterwards"""
    from lib.hip import ops

    try:
        yield ops.set_winograd_split
    finally:
        ops.set_winograd_split(True)


def dev(a):
    return torch.tensor(a, device=DEV)      # a copy: the cases' arrays are read-only


def padded(a):
    """(N, H, W, C) -> device (N, H, W, C + PAD_IN), the pad channels NaN: nothing may read them"""
    t = torch.full(a.shape[:3] + (a.shape[3] + PAD_IN,), float("nan"), device=DEV)
    t[..., :a.shape[3]] = dev(a)
    return t


def model(c, three):
    """worst element of the numpy model on the case's data, its plane product the three-term or the f32-pipe sum; once per case"""
    memo = c.__dict__.setdefault("_model", {})
    if three not in memo:
        memo[three] = c.error(c.run(dot=six_product_dot if three else f32_pipe_dot)).max()
    return memo[three]


class Layer(object):
    """the library's layer of a wino_reference.Case: packs the weights once; run() is one call on guarded buffers"""

    def __init__(self, c):
        from lib.hip import ops

        self.c, f = c, c.family
        self.lib = ops.lib()
        self.bias = None if c.b is None else dev(c.b)
        if f in ("f2x2", "f4x4"):
            self.m = 2 if f == "f2x2" else 4
            self.wp = ops.winograd_pack_weight(dev(c.w), m=self.m)
        elif f == "conv5x5s2":
            self.wp = ops.winograd5x5s2_pack_weight(dev(c.w))
        elif f == "conv3x3s2":
            self.wp = ops.winograd3x3s2_pack_weight(dev(c.w))
        elif f == "dgrad5x5s2":
            self.wp = ops.winograd5x5s2_dgrad_pack_weight(dev(c.w))

    def run(self, tile=0, images=slice(None), bias="own", splits=1, what=""):
        """-> the output window on the host, or None when the library refused the call (DIM_ERR_ARG, nothing written: checked)"""
        from lib.hip import capi, ops

        c, f, L = self.c, self.c.family, self.lib
        _, H, W, Cin, Cout = c.shape
        Ho, Wo = c.out_hw
        bias = self.bias if isinstance(bias, str) else bias
        wgrad = f in ("wgrad_s1", "wgrad_s2")
        if f == "dgrad5x5s2":
            src = padded(c.dy[images])
            n = src.shape[0]
            need, out, coff, C = L.dim_winograd5x5s2_workspace_floats(n, H, W, Cin, Cout), (n, H, W, Cin + PAD_OUT), 0, Cin
        elif wgrad:
            src, dy = padded(c.x[images]), padded(c.dy[images])
            n = src.shape[0]
            need = L.dim_conv2d_wgrad_winograd_workspace_floats(n, H, W, Cin, Cout, c.stride, splits)
        else:
            src = padded(c.x[images])
            n = src.shape[0]
            need = (L.dim_winograd_workspace_floats(n, H, W, Cin, Cout, self.m) if f in ("f2x2", "f4x4") else
                    L.dim_winograd5x5s2_workspace_floats(n, H, W, Cin, Cout) if f == "conv5x5s2" else
                    L.dim_winograd3x3s2_workspace_floats(n, H, W, Cin, Cout))
            out, coff, C = (n, Ho, Wo, Cout + PAD_OUT), COFF, Cout
        ws = torch.full((need + GUARD,), float("nan"), device=DEV)
        ws[need:] = 7.0
        y = torch.full((Cout, Cin, c.k, c.k), float("nan"), device=DEV) if wgrad else torch.full(out, 7.0, device=DEV)
        try:
            if f in ("f2x2", "f4x4"):
                ops.conv2d_fwd_winograd(src, Cin, self.wp, bias, Cout, slope=c.slope, tile=tile, out=y, out_coff=coff, workspace=ws[:need], m=self.m)
            elif f == "conv5x5s2":
                ops.conv2d_fwd_winograd5x5s2(src, Cin, self.wp, bias, Cout, slope=c.slope, tile=tile, out=y, out_coff=coff, workspace=ws[:need])
            elif f == "conv3x3s2":
                ops.conv2d_fwd_winograd3x3s2(src, Cin, self.wp, bias, Cout, slope=c.slope, tile=tile, out=y, out_coff=coff, workspace=ws[:need])
            elif f == "dgrad5x5s2":
                ops.conv2d_dgrad_winograd5x5s2(src, Cout, self.wp, y, Cin, tile=tile, workspace=ws[:need])
            else:
                ops.conv2d_wgrad_winograd(src, Cin, dy, Cout, y, S=c.stride, splits=splits, workspace=ws[:need])
        except capi.DeepIMHipError as e:
            assert "error -1:" in str(e), (what, str(e))
            torch.cuda.synchronize()
            assert wgrad or bool((y == 7.0).all()), (what, "refused, but wrote")
            return None
        got = y.cpu().numpy()
        assert bool((ws[need:] == 7.0).all()), (what, "wrote behind its workspace of %d floats" % need)
        if wgrad:
            assert np.isfinite(got).all(), (what, "not every element of dW written / finite")
            return got
        assert np.all(got[..., :coff] == 7.0) and np.all(got[..., coff + C:] == 7.0), (what, "wrote outside its channel window")
        return got[..., coff:coff + C]


def three_term(split, tile, c):
    """does the three-term kernel run?  (the switch on, a tile that has one; tile 0 = auto is tile 3 below 1024 tiles or Nout % 128 != 0)"""
    nout = 4 * c.shape[3] if c.family == "dgrad5x5s2" else c.shape[4]
    assert tile or c.shape[0] * 25 < 1024 or nout % 128
    return bool(split) and tile in SPLIT_TILES and nout % 128 == 0 and c.family not in ("wgrad_s1", "wgrad_s2")


def within_bar(c, got, split, tile, what):
    """the per-element bar of one run; -> (worst element, the model's worst element)"""
    e = c.error(got)
    m = model(c, three_term(split, tile, c))
    bar = BAR_FACTOR * m
    print("%-40s tile %d %-11s GPU %.3e  model %.3e  bar %.3e" % (what, tile, "three terms" if three_term(split, tile, c) else "f32 pipe", e.max(), m, bar))
    assert e.max() <= bar, (what, tile, split, e.max(), bar, np.unravel_index(e.argmax(), e.shape))
    return e.max(), m


def table(rows):
    for (family, kind, arith), (g, m) in sorted(rows.items()):
        print("TABLE | %s | %s | %s | %.2e | %.2e |" % (family, kind, arith, g, m))


def note(rows, key, gm):
    rows[key] = max(rows.get(key, (0.0, 0.0)), gm)


def several_tiles(family):
    return (9, 11) if family in ("f2x2", "f4x4", "wgrad_s1") else (17, 21)


# ---------------------------------------------------------------------------------------------------------------- per-family cases
@pytest.mark.parametrize("kind", wr.INPUT_CLASSES)
@pytest.mark.parametrize("family", FORWARD)
def test_forward_layers(arithmetic, family, kind):
    """one map of several tiles with remainders on both axes, bias + slope 0.1, Cout 128 on the tiles 3, 4, 6, 7 (randn: Cout 256 on
    tile 5 too; lrelu: no bias, slope 1, Cout 64 on the default tile as well); the sparse class has three images, the last one zero"""
    H, W = several_tiles(family)
    N = 3 if kind == "sparse" else 2
    runs = [(wr.Case(family, kind, N, H, W, 32, 128, 11), (3, 4, 6, 7))]
    if kind == "randn":
        runs.append((wr.Case(family, kind, N, H, W, 32, 256, 12), (5,)))
    if kind == "lrelu":
        runs.append((wr.Case(family, kind, N, H, W, 32, 64, 13, bias=False, slope=1.0), (0,)))
    rows = {}
    for c, tiles in runs:
        layer = Layer(c)
        for split, tile in [(0, t) for t in tiles] + [(1, t) for t in tiles if t in SPLIT_TILES]:
            arithmetic(bool(split))
            what = "%s %s Cout %d" % (family, kind, c.shape[4])
            got = layer.run(tile=tile, what=what)
            assert got is not None, what
            note(rows, (family, kind, "three terms" if three_term(split, tile, c) else "f32 pipe"), within_bar(c, got, split, tile, what))
            if kind == "sparse":
                assert np.all(got[-1] == 0), (what, "the zero image of the batch is not zero")
    table(rows)


@pytest.mark.parametrize("kind", wr.INPUT_CLASSES)
def test_input_gradient_5x5s2(arithmetic, kind):
    """dX of the 5x5 / stride-2 layer on 17 x 21 (dY 9 x 11): K = Cout = 64, N = 4 Cin = 128, tiles 3 (auto), 4, 6, 7"""
    c = wr.Case("dgrad5x5s2", kind, 3 if kind == "sparse" else 2, 17, 21, 32, 64, 21)
    layer, rows = Layer(c), {}
    for split, tile in ((0, 0), (0, 4), (0, 6), (0, 7), (1, 0), (1, 4), (1, 7)):
        arithmetic(bool(split))
        got = layer.run(tile=tile, what="dgrad5x5s2 " + kind)
        note(rows, ("dgrad5x5s2", kind, "three terms" if three_term(split, tile, c) else "f32 pipe"), within_bar(c, got, split, tile, "dgrad5x5s2 " + kind))
        if kind == "sparse":
            assert np.all(got[-1] == 0)
    table(rows)


@pytest.mark.parametrize("kind", wr.INPUT_CLASSES)
@pytest.mark.parametrize("S", [1, 2])
def test_weight_gradient(arithmetic, S, kind):
    """dW through F(3x3, 4x4): pixel splits 1 and 3 (the sum over tiles in one and in three slabs), under both switches (the same
    kernels: bit-identical)"""
    family = "wgrad_s%d" % S
    H, W = several_tiles(family)
    c = wr.Case(family, kind, 2, H, W, 64 if S == 1 else 32, 64, 31)
    layer, rows, first = Layer(c), {}, {}
    for split in (0, 1):
        arithmetic(bool(split))
        for splits in (1, 3):
            got = layer.run(splits=splits, what="%s %s splits %d" % (family, kind, splits))
            note(rows, (family, kind, "f32 pipe"), within_bar(c, got, split, 0, "%s %s splits %d" % (family, kind, splits)))
            np.testing.assert_array_equal(first.setdefault(splits, got), got)
    table(rows)


# ---------------------------------------------------------------------------------------------------------------- small maps
def sweep(arithmetic, family, sizes, three):
    """every size: N = 2, class lrelu; Cout 64 on the default tile under both switches, or (three) Cout 128 on tile 7 with the switch on.
    Per element bar, sentinels and guards (Layer.run), the second image alone = the second image of the batch, bit for bit"""
    wgrad = family in ("wgrad_s1", "wgrad_s2")
    Cin = 64 if family == "wgrad_s1" else 32
    refused, worst = [], {}
    for H, W in sizes:
        for Cout, tile, splits in (((128, 7, (1,)),) if three else ((64, 0, (0, 1)),)):
            c = wr.Case(family, "lrelu", 2, H, W, Cin, Cout, 1000 + 20 * H + W)
            layer, what, first = Layer(c), "%s %dx%d Cout %d" % (family, H, W, Cout), None
            for split in splits:
                arithmetic(bool(split))
                got = layer.run(tile=tile, what=what)
                if got is None:
                    refused.append((H, W))
                    continue
                e, m = c.error(got).max(), model(c, three_term(split, tile, c))
                assert e <= BAR_FACTOR * m, (what, split, e, m, np.unravel_index(c.error(got).argmax(), got.shape))
                key = "three terms" if three_term(split, tile, c) else "f32 pipe"
                worst[key] = max(worst.get(key, (0.0, 0.0, None)), (e / m, e, (H, W)))
                if first is not None:        # Cout 64: tile 3 under either switch
                    np.testing.assert_array_equal(got, first, err_msg=what)
                first = got
                if not wgrad:
                    alone = layer.run(tile=tile, images=slice(1, 2), what=what + " second image alone")
                    np.testing.assert_array_equal(alone[0], got[1], err_msg=what)
    for key, (ratio, e, hw) in sorted(worst.items()):
        print("SWEEP | %s | %s | worst GPU / model %.2f at %dx%d (GPU %.2e) | %d sizes" % (family, key, ratio, hw[0], hw[1], e, len(sizes)))
    assert sorted(set(refused)) == sorted(REFUSED[family]), (family, "refused sizes", sorted(set(refused)))


SWEEPS = [(f, t) for f in wr.FAMILIES for t in (False, True) if not (t and f.startswith("wgrad"))]


@pytest.mark.parametrize("family,three", [s for s in SWEEPS if s[0] in ("f2x2", "f4x4", "wgrad_s1")],
                         ids=lambda v: v if isinstance(v, str) else "three-terms-tile7" if v else "default-tile")
def test_small_maps_stride1(arithmetic, family, three):
    """every (H, W) in 1 .. 9: maps inside one tile on both axes, smaller than the halo, one pixel"""
    sweep(arithmetic, family, S1_SIZES, three)


@pytest.mark.parametrize("family,three", [s for s in SWEEPS if s[0] not in ("f2x2", "f4x4", "wgrad_s1")],
                         ids=lambda v: v if isinstance(v, str) else "three-terms-tile7" if v else "default-tile")
def test_small_maps_stride2(arithmetic, family, three):
    """every (H, W) in {1 .. 10, 15, 16, 17}: H or W = 1 leaves the odd phase image empty"""
    sweep(arithmetic, family, S2_SIZES, three)


# ---------------------------------------------------------------------------------------------------------------- bias alignment
@pytest.mark.parametrize("family", FORWARD)
def test_bias_at_an_odd_float_offset(arithmetic, family):
    """the bias of a flat parameter blob is only 4-byte aligned: a view at float offsets 1 and 3 of a larger buffer gives the bits of an
    aligned copy (wino_s2_output_kernel reads it element by element; wino_output_kernel / wino4_output_kernel as 16- / 8-byte vectors)"""
    H, W = several_tiles(family)
    c = wr.Case(family, "lrelu", 2, H, W, 32, 64, 41)
    layer = Layer(c)
    arithmetic(True)
    want = layer.run(what=family + " aligned bias")
    within_bar(c, want, 1, 0, family + " aligned bias")
    for off in (1, 3):
        blob = torch.full((c.shape[4] + 8,), float("nan"), device=DEV)
        blob[off:off + c.shape[4]] = layer.bias
        view = blob[off:off + c.shape[4]]
        assert view.data_ptr() % 8 == 4
        np.testing.assert_array_equal(layer.run(bias=view, what="%s bias at float offset %d" % (family, off)), want)
