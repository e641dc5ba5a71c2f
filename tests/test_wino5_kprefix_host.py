"""The forward 5x5 / stride-2 Winograd layer without the zero blocks of its transformed weights, on the CPU in float64
(tools/wino5_kprefix_proto.py is the numpy statement of csrc/winograd.hip's skipping and of wino_gemm_plan's partition): the dropped
weight blocks are exactly zero, the form that never reads them equals the direct convolution, and the plane GEMMs' ranges are those
of the full K, so that no item is shared by more than two workgroups and every item is cut where it was cut before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import wino5_kprefix_proto as proto  # noqa: E402


def test_23_blocks_are_dropped_in_11_planes():
    dropped = [(p, ph) for p in range(36) for ph in range(4) if not proto.live(p, ph)]
    assert len(dropped) == 23
    assert sorted({p for p, _ in dropped}) == [5, 11, 17, 23, 29, 30, 31, 32, 33, 34, 35]
    assert all(proto.live(p, 0) for p in range(36))          # phase (0,0) is live everywhere: an item always begins with a live chunk
    assert [ph for ph in range(4) if proto.live(35, ph)] == [0]
    assert [ph for ph in range(4) if proto.live(30, ph)] == [0, 1] and [ph for ph in range(4) if proto.live(5, ph)] == [0, 2]


def test_dropped_weight_blocks_are_exactly_zero():
    rng = np.random.RandomState(3)
    C, Co = 4, 3
    U = proto.pack(rng.randn(Co, C, 5, 5))
    for p in range(36):
        for ph in range(4):
            blk = U[p, ph * C:(ph + 1) * C]
            if proto.live(p, ph):
                assert np.any(blk != 0.0), (p, ph)
            else:
                assert np.all(blk == 0.0), (p, ph)


def test_input_transform_stores_the_live_blocks_and_nothing_else():
    rng = np.random.RandomState(4)
    C = 2
    V, _ = proto.input_transform(rng.randn(9, 13, C))
    for p in range(36):
        for ph in range(4):
            blk = V[:, p, ph * C:(ph + 1) * C]
            assert (not np.isnan(blk).any()) if proto.live(p, ph) else np.isnan(blk).all(), (p, ph)


@pytest.mark.parametrize("shape", [(8, 8, 3, 2), (9, 11, 4, 3), (16, 24, 2, 2), (7, 10, 2, 4), (15, 21, 3, 2), (1, 1, 2, 2)])
def test_skipping_form_equals_direct_convolution(shape):
    H, W, C, Co = shape
    rng = np.random.RandomState(sum(shape))
    x, w = rng.randn(H, W, C), rng.randn(Co, C, 5, 5)
    ref = proto.conv_direct(x, w)
    got = proto.conv_wino5(x, w)    # holes are NaN in V: a contraction that read them would not be finite
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


# (N, H, W, Cin, Cout), tiles: the shapes of tests/test_gpu_wino5_kprefix.py and the two layers at 16 pairs
PLAN_CASES = [((1, 6, 9, 32, 64), (3,)), ((2, 30, 40, 64, 128), (3, 4, 6, 7)), ((1, 16, 24, 32, 256), (5,)), ((16, 116, 160, 32, 128), (4,)),
              ((16, 240, 320, 64, 128), (4,)), ((16, 120, 160, 128, 256), (5,)), ((5, 22, 30, 64, 128), (3, 4)), ((2, 22, 30, 64, 128), (3, 4))]


@pytest.mark.parametrize("case", PLAN_CASES)
def test_no_item_is_shared_by_more_than_two_workgroups(case):
    (N, H, W, C, Cout), tiles = case
    T = N * (-(-((H + 1) // 2) // 4)) * (-(-((W + 1) // 2) // 4))
    for tile in tiles:
        for slots in (256, 512, 768, 1024, 1280):           # resident workgroups of the kernels: 1 .. 5 per CU
            ranges, items, alive = proto.plan(T, C, Cout, tile, slots)
            assert ranges[0][0] == 0 and ranges[-1][1] == items[-1][1]
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            assert min(e - b for b, e in ranges) >= 4 * C // 32, (tile, slots)   # a range is at least one item long ...
            csum = np.concatenate([[0], np.cumsum(alive)])
            assert min(csum[e] - csum[b] for b, e in ranges) >= 1                # ... so it holds the live first chunk of some item
            assert proto.workgroups_per_item(ranges, items, alive).max() <= 2, (tile, slots)
            assert alive.sum() * 144 == len(alive) * 121
