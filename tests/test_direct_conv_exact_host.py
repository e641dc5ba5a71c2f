"""tests/direct_conv_exact.py on the host: the exact domain holds for everything tests/test_gpu_direct_conv_exact.py enumerates, the
assertion fires outside it, and every fault a direct kernel can have changes at least one element on some size of the sweep."""
import numpy as np
import pytest

import direct_conv_exact as dc
import test_gpu_direct_conv_exact as gpu
from direct_conv_exact import K3S1, K3S2, K5S2, Geometry


@pytest.mark.parametrize("name,plan,args", gpu.PLANS, ids=["-".join([n] + [gpu.ident(a) for a in args]) for n, _, args in gpu.PLANS])
def test_every_enumerated_case_is_inside_the_exact_domain(name, plan, args):
    """sum |a||b| + |bias| + |prior| < 2^24 per output element and integer operands after rounding, for every (family, geometry, class,
    size, pipe, accumulate, window) of the GPU file's plan, once each; refused runs have no output to bound"""
    seen, worst = set(), 0.0
    for r in plan(*args):
        what = (r.key, r.pipe, r.accumulate, r.window, r.fold)
        if what in seen or gpu.refusal(r):
            continue
        seen.add(what)
        worst = max(worst, dc.assert_exact_domain(dc.problem(*r.key), r.pipe, r.accumulate, r.window, r.fold))
    print("%s%s: %d cases, largest bound %.4g of %.4g" % (name, tuple(gpu.ident(a) for a in args), len(seen), worst, dc.LIMIT))
    assert seen and worst < dc.LIMIT


def test_the_refused_runs_are_a_small_named_part_of_the_plans():
    """the refusal table takes out of the sweeps only tile 9 at Cout 64 / stride 2"""
    names = set()
    for _, plan, args in gpu.PLANS:
        names |= {gpu.refusal(r) for r in plan(*args)} - {None}
    assert names == {gpu.T9_STRIDE2}
    assert all(gpu.refusal(r) for r in gpu.REFUSALS)


def test_the_domain_assertion_fires_on_a_widened_case():
    """the 5x5 forward widened from the sweeps' 96 channels: 1024 are still inside (271 x 25600 + 4 < 2^24), 4096 are not; and ties in
    both operands of a product are refused whatever the size"""
    p = dc.Problem("fwd", K5S2, "x_ties", 1, 5, 5, 1024, 64)
    assert 4e6 < dc.assert_exact_domain(p, "f32") < dc.LIMIT
    with pytest.raises(AssertionError, match="outside the exact domain"):
        dc.assert_exact_domain(dc.Problem("fwd", K5S2, "x_ties", 1, 5, 5, 4096, 64), "f32")
    with pytest.raises(AssertionError, match="outside the exact domain"):
        dc.assert_exact_domain(p, "f32", limit=float(1 << 20))
    both = dc.Problem("fwd", K5S2, "x_ties", 1, 5, 5, 32, 64)
    both.w = dc.Problem("fwd", K5S2, "w_ties", 1, 5, 5, 32, 64).w
    with pytest.raises(AssertionError, match="ties in both operands"):
        dc.assert_exact_domain(both, "f32")
    frac = dc.Problem("fwd", K3S1, "ints", 1, 3, 3, 32, 64)
    frac.x = frac.x * 0.5
    with pytest.raises(AssertionError, match="not all integers"):
        dc.assert_exact_domain(frac, "f32")
    tie = dc.Problem("wgrad", K3S1, "x_ties", 1, 3, 3, 32, 64)
    dc.assert_exact_domain(tie, "bf16")                   # rounded ties are integers (multiples of 2 or 4)
    assert not np.array_equal(dc.rne(tie.x), tie.x)


SIZES = [(1, 1), (2, 3), (3, 3), (4, 7), (5, 5), (8, 8), (9, 16), (16, 17)]


def differs(want, got):
    return dc.mismatch(got, want) is not None


@pytest.mark.parametrize("kind", dc.CLASSES)
def test_each_fault_changes_an_element_on_some_size(kind):
    seen = {f: [] for f in dc.FAULTS}
    for H, W in SIZES:
        for g in (K3S1, K5S2):
            p = dc.problem("fwd", g, kind, 2, H, W, 32, 64)
            if differs(dc.reference(p, "bf16"), dc.fault("last_column_tap", p, "bf16")):
                seen["last_column_tap"].append((g, H, W))
            if differs(dc.reference(p, "bf16", True), dc.fault("accumulate_overwrites", p, "bf16", True)):
                seen["accumulate_overwrites"].append((g, H, W))
        d = dc.problem("dgrad", K3S2, kind, 2, H, W, 32, 64)
        if differs(dc.reference(d, "bf16"), dc.fault("phase_extent", d, "bf16")):
            seen["phase_extent"].append((H, W))
            assert H % 2 == 1                     # even H: both row phases have H / 2 rows
        w = dc.problem("wgrad", K3S1, kind, 2, H, W, 32, 64)
        if differs(dc.reference(w, "bf16"), dc.fault("wgrad_block", w, "bf16")):
            seen["wgrad_block"].append((H, W))
    for H, W in dc.SMALL_BATCH:                   # 5 images of up to 9 pixels: a 64-row tile holds all of them
        p = dc.problem("fwd", K3S1, kind, 5, H, W, 32, 64)
        if differs(dc.reference(p, "bf16"), dc.fault("row_tile_padding", p, "bf16")):
            seen["row_tile_padding"].append((H, W))
    for f in ("last_column_tap", "accumulate_overwrites", "phase_extent", "wgrad_block", "row_tile_padding"):
        print(f, kind, seen[f])
        assert seen[f], (f, kind)
    assert len(seen["last_column_tap"]) == 2 * len(SIZES)      # the image's last column always has a tap of the last output column


@pytest.mark.parametrize("family,g", [("fwd", K3S1), ("fwd", K5S2), ("dgrad", K3S2), ("wgrad", K3S1), ("deconv", dc.DECONV)], ids=gpu.ident)
def test_truncation_is_invisible_to_ints_and_visible_to_the_ties(family, g):
    """A kernel that truncated its operands to bf16 instead of rounding them to nearest even would pass every size of the `ints` class:
    integers up to 4 are bf16 values, no rounding happens at all.  That is why the ties classes exist: +-(257 + 2 j) lies half way
    between two bf16 values, nearest-even and truncation disagree for odd j, and the fault shows in whichever operand carries them"""
    window = (4, 6) if family == "deconv" else None
    for H, W in ((2, 3), (5, 5), (9, 16)):
        p = dc.problem(family, g, "ints", 2, H, W, 32, 64)
        assert not differs(dc.reference(p, "bf16", window=window), dc.reference(p, "bf16", window=window, rounding=dc.truncate)), (family, H, W)
        for kind in ("x_ties", "w_ties"):
            p = dc.problem(family, g, kind, 2, H, W, 32, 64)
            assert differs(dc.reference(p, "bf16", window=window), dc.reference(p, "bf16", window=window, rounding=dc.truncate)), (family, kind, H, W)
            # ... and on the f32 pipe nothing is rounded at all: the reference is the unrounded one
            assert differs(dc.reference(p, "bf16", window=window), dc.reference(p, "f32", window=window)), (family, kind, H, W)


def test_rounding_models():
    ties = np.array([257.0, 259.0, 261.0, 263.0, 265.0, 267.0, 269.0, 271.0, -259.0])
    np.testing.assert_array_equal(dc.rne(ties), [256, 260, 260, 264, 264, 268, 268, 272, -260])
    np.testing.assert_array_equal(dc.truncate(ties), [256, 258, 260, 262, 264, 266, 268, 270, -258])
    small = np.arange(-4.0, 5.0)
    np.testing.assert_array_equal(dc.rne(small), small)
    np.testing.assert_array_equal(dc.truncate(small), small)


def test_packed_layout_and_mismatch_report():
    w = np.arange(64 * 32 * 9, dtype=np.float64).reshape(64, 32, 3, 3)
    pk = dc.packed(w).reshape(9, 64, 32)
    assert pk[4, 7, 5] == w[7, 5, 1, 1] and pk.size == dc.packed_floats(32, 64, 3)
    w8 = np.arange(64 * 8 * 49, dtype=np.float64).reshape(64, 8, 7, 7)
    p8 = dc.packed(w8).reshape(13, 64, 32)
    assert p8[1, 3, 8 * 2 + 5] == w8[3, 5, 0, 6] and np.all(p8[12, :, 8:] == 0) and p8.size == dc.packed_floats(8, 64, 7)
    a = np.zeros((2, 3, 4, 5))
    assert dc.mismatch(-a, a) is None                     # -0.0 equals 0.0
    b = a.copy()
    b[1, 2, 0, 3] = 1.0
    b[1, 2, 3, 4] = 2.0
    assert dc.mismatch(b, a) == (2, (1, 2, 0, 3), 1.0, 0.0)
    assert gpu.clamped_splits(2, 9, 11, 100) == 7 and gpu.clamped_splits(2, 9, 11, 2) == 2 and gpu.clamped_splits(1, 30, 40, 7, 20) == 7
