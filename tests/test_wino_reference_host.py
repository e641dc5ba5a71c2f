"""tests/wino_reference.py checked against itself (no GPU): with float64 every family is the convolution; with float32 it is the model
whose worst element sets the bar of tests/test_gpu_wino_layers.py -- and that bar (BAR_FACTOR x the intact model's worst element, per
element in units of the element's output tile) catches, on the model, the defects a layer-level bar lets through.

Why this file: the layer tests of tests/test_gpu_ops.py hold the Winograd layers to 1e-4 max|ref| + 2e-5 (2e-6 for the weight
gradient).  On the DC class (randn + 8, max|ref| about 25) one transform coefficient off by one part in 4096 passes that bar in every
family (F(2x2)'s B^T excepted: all its coefficients are +-1 and meet the whole offset).  The per-element bar catches every one.

Controls, each on the model with both plane products, each against BAR_FACTOR x the intact model's worst element on the same data:
  (a) one coefficient of B^T, of G, of A^T times 1 + 2^-12 -- the coefficient the old bar sees least on the DC class (COEFFICIENT)
  (b) V of one plane rounded to bf16 -- again the plane the old bar sees least (BF16_PLANE)
  (c) pixels outside the map replicate the edge instead of being zero
  (d) py and px exchanged in the phase-major channel order of the 5x5 / stride-2 families
All clear the new bar in every family and input class (smallest margin: 3.3 x the bar, A^T[3][4] = -1/8 of the 5x5 / stride-2
forward layer on the DC class).

What the old bar does with (a) and (b) on the DC class is asserted both ways: it lets them pass, except for the pairs in
OLD_BAR_CATCHES, which it catches.  That list is longer than was expected when this file was planned: one plane of V in bf16 is 1.8 .. 3.8
times over the old bar in every family but the 3x3 / stride-2 one (a plane carries an eighth-bit error into a sum the output
transform weights by up to 8 x 8).  The old bar's blind spot is the coefficients, not a plane in bf16."""
import numpy as np
import pytest

import wino_reference as wr
from test_split_terms import BAR_FACTOR, bf16_rne, f32_pipe_dot, six_product_dot

DOTS = (six_product_dot, f32_pipe_dot)
BASE = dict(f2x2=wr.F23, f4x4=wr.F43, conv5x5s2=wr.F43, dgrad5x5s2=wr.F43, wgrad_s1=wr.F34, wgrad_s2=wr.F34, conv3x3s2=wr.F42)
# (row, column) of the scaled coefficient per matrix: of all non-zero ones the one whose defect is smallest under the old bar on "dc"
COEFFICIENT = dict(f2x2=dict(BT=(3, 1), G=(3, 2), AT=(1, 2)),
                   f4x4=dict(BT=(1, 3), G=(3, 0), AT=(3, 4)),
                   conv5x5s2=dict(BT=(2, 2), G=(3, 0), AT=(3, 4)),
                   dgrad5x5s2=dict(BT=(2, 2), G=(3, 0), AT=(3, 4)),
                   wgrad_s1=dict(BT=(2, 2), G=(4, 3), AT=(0, 3)),
                   wgrad_s2=dict(BT=(2, 2), G=(4, 3), AT=(0, 3)),
                   conv3x3s2=dict(BT=(2, 3), G=(2, 0), AT=(3, 2)))
BF16_PLANE = dict(f2x2=15, conv3x3s2=68)      # every other family: plane 14 = (2, 2)
OLD_BAR_CATCHES = {("f2x2", "BT")} | {(f, "bf16") for f in wr.FAMILIES if f != "conv3x3s2"}


def case(family, kind, H=None, W=None, seed=7):
    s1 = family in ("f2x2", "f4x4", "wgrad_s1")
    return wr.Case(family, kind, 2, H or (9 if s1 else 17), W or (11 if s1 else 21), 64 if family == "wgrad_s1" else 32, 64, seed)


def old_bar(c):
    return 1e-4 * np.abs(c.ref).max() + (2e-6 if c.family.startswith("wgrad") else 2e-5)


def controls(family):
    def scaled(name):
        m = BASE[family][name].copy()
        m[COEFFICIENT[family][name]] *= 1 + 2.0 ** -12
        return dict(mats={name: m})

    def one_plane_bf16(V):
        V = V.copy()
        p = BF16_PLANE.get(family, 14)
        V[p] = bf16_rne(V[p])
        return V

    ctl = dict(BT=scaled("BT"), G=scaled("G"), AT=scaled("AT"), bf16=dict(v_hook=one_plane_bf16), edge=dict(border="edge"))
    if family in ("conv5x5s2", "dgrad5x5s2", "wgrad_s2"):
        ctl["phase"] = dict(swap_phase=True)
    return ctl


SMALL = [(1, 5), (5, 1), (2, 2), (1, 1), (7, 6)]


@pytest.mark.parametrize("family", wr.FAMILIES)
def test_float64_is_the_convolution(family):
    """maps that do not divide into tiles, 1 x W, H x 1, 2 x 2, 1 x 1, and the several-tile map of the controls: 1e-11 of max|ref|"""
    for H, W in SMALL + [(None, None)]:
        for kind in ("lrelu", "dc"):
            c = case(family, kind, H, W)
            err = np.abs(c.run(np.float64) - c.ref).max()
            assert err <= 1e-11 * np.abs(c.ref).max(), (family, c.shape, kind, err)


@pytest.mark.parametrize("family", wr.FAMILIES)
def test_model_worst_element_and_controls(family):
    for kind in wr.INPUT_CLASSES:
        c = case(family, kind)
        intact = [c.error(y).max() for y in c.run(dot=DOTS)]
        print("%-11s %-6s model worst element: three terms %.2e, f32 pipe %.2e   (old bar %.1e = %.0f x the f32 model's absolute error)"
              % (family, kind, intact[0], intact[1], old_bar(c), old_bar(c) / np.abs(c.run(dot=f32_pipe_dot) - c.ref).max()))
        assert max(intact) < 4e-6, (family, kind, intact)      # f32 accuracy: a few 2^-24 of the tile's sum |x w|, times the transforms' gain
        for name, defect in controls(family).items():
            ys = c.run(dot=DOTS, **defect)
            over = min(c.error(y).max() / (BAR_FACTOR * i) for y, i in zip(ys, intact))
            old = max(np.abs(y - c.ref).max() for y in ys) / old_bar(c)
            print("    %-5s %10.1f x the new bar, %8.2f x the old" % (name, over, old))
            assert over > 1.0, (family, kind, name, over)
            if kind == "dc" and name in ("BT", "G", "AT", "bf16"):
                assert (old > 1.0) == ((family, name) in OLD_BAR_CATCHES), (family, name, old)


def test_sparse_maps_hold_exact_zeros():
    """the zero rule of the measure is not vacuous: the sparse class has whole zero tiles and they are exact zeros in the f32 model;
    the weight gradient has pairs whose taps meet no product and are not exact zeros (wr.taps_error)"""
    for family in ("f4x4", "conv5x5s2", "dgrad5x5s2", "conv3x3s2"):
        c = case(family, "sparse")
        zero = wr.tile_max(c.unit, *(2 * (8 if family == "dgrad5x5s2" else 4,))) == 0
        # one zero image in every family; zero tiles beside live ones where a tile covers few pixels (a stride-2 tile covers 11 x 11)
        assert zero[1].all() and not zero[0].all() and (zero[0].any() or family != "f4x4"), (family, zero[0].mean())
        assert np.all(c.run(dot=six_product_dot)[zero] == 0), family
    c = case("wgrad_s1", "sparse")
    dw = c.run(dot=f32_pipe_dot)
    no_tap = np.broadcast_to(c.unit.max(axis=(2, 3), keepdims=True) == 0, dw.shape)
    assert c.wide is not None and no_tap.mean() > 0.1 and np.any(dw[no_tap] != 0) and np.isinf(wr.taps_error(dw, c.ref, c.unit).max())
    assert np.isfinite(c.error(dw)).all()
    assert np.all(dw[np.broadcast_to(c.wide.max(axis=(2, 3), keepdims=True) == 0, dw.shape)] == 0)


def test_measure_rejects_a_nonzero_in_a_zero_tile():
    c = case("f4x4", "sparse")
    y = c.run().copy()
    zero = wr.tile_max(c.unit, 4, 4) == 0
    y[tuple(np.argwhere(zero)[0])] = 1e-30
    assert np.isinf(c.error(y).max())
