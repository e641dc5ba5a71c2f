"""Forward 5x5 / stride-2 Winograd layers with the zero blocks of their transformed weights skipped (csrc/winograd.hip: 23 of the 144
(phase, plane) blocks are neither stored in V nor multiplied; csrc/wino_gemm.hip: the cursors step over their chunks) against
torch-CPU float64, in both arithmetics of the plane GEMMs.  The shapes put range boundaries inside items with and without skipped
chunks, and have more items than resident workgroups; a NaN-filled workspace shows that the holes of V are never read and that
everything read is written."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout), tiles
CASES = [((1, 6, 9, 32, 64), (3,)),               # 2 tile rows, 36 items of 4, 2 or 1 multiplied chunks
         ((2, 30, 40, 64, 128), (3, 4, 6, 7)),
         ((1, 16, 24, 32, 256), (5,)),
         ((16, 116, 160, 32, 128), (4,))]         # 1368 items: more than the resident workgroups
IDS = ["x".join(map(str, c[0])) for c in CASES]


@pytest.fixture(params=[1, 0], ids=["bf16x3", "f32"])
def wino_split(request, hip_lib):
    """both arithmetics of the plane GEMMs: three bf16 terms / six MFMA products (the default), and the f32 matrix pipe"""
    from lib.hip import ops

    ops.set_winograd_split(bool(request.param))
    yield request.param
    ops.set_winograd_split(True)


@functools.lru_cache(maxsize=None)
def problem(shape):
    """inputs and the float64 reference of one shape, computed once and shared (read-only) by the tests below"""
    import torch.nn.functional as F

    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape) + 29)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 5, 5), generator=g) * (1.0 / np.sqrt(25 * Cin))
    b = torch.randn((Cout,), generator=g) * 0.1
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=2), 0.1).permute(0, 2, 3, 1).numpy()
    ref.setflags(write=False)
    return x.permute(0, 2, 3, 1).contiguous(), w, b, ref


def run(shape, tile, workspace=None):
    from lib.hip import ops

    x, w, b, ref = problem(shape)
    N, H, W, Cin, Cout = shape
    wp = ops.winograd5x5s2_pack_weight(w.to("cuda:0"))
    y = ops.conv2d_fwd_winograd5x5s2(x.to("cuda:0"), Cin, wp, b.to("cuda:0"), Cout, slope=0.1, tile=tile, workspace=workspace)
    return y.cpu().numpy(), ref


def check(y, ref, what):
    assert y.shape == ref.shape
    assert np.isfinite(y).all(), what
    err, bar = np.abs(y - ref).max(), 1e-4 * np.abs(ref).max() + 2e-5
    print("%s: max err %.3e, bar %.3e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vs_f64(hip_lib, case, wino_split):
    shape, tiles = case
    for tile in tiles:
        y, ref = run(shape, tile)
        check(y, ref, (shape, tile))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nan_workspace_vs_f64(hip_lib, case, wino_split):
    """the same calls on a workspace full of NaN: finite and within the bar only if the GEMMs never read what the input transform
    does not store (the 23 skipped blocks of every tile row) and the transform stores all they read"""
    shape, tiles = case
    N, H, W, Cin, Cout = shape
    need = hip_lib.dim_winograd5x5s2_workspace_floats(N, H, W, Cin, Cout)
    for tile in tiles:
        ws = torch.full((need,), float("nan"), device="cuda:0")
        y, ref = run(shape, tile, workspace=ws)
        check(y, ref, (shape, tile, "NaN workspace"))


@pytest.mark.parametrize("case", [CASES[0], CASES[-1]], ids=[IDS[0], IDS[-1]])
def test_same_call_twice_is_bit_identical(hip_lib, case, wino_split):
    shape, tiles = case
    y0, _ = run(shape, tiles[0])
    y1, _ = run(shape, tiles[0])
    np.testing.assert_array_equal(y0, y1)


def test_unit_taps_name_a_wrong_phase_or_plane(hip_lib, wino_split):
    """64 output channels, 25 of them one unit tap each (channel 5 i + j: tap (i, j) of input channel 5 i + j), the rest random: with a
    wrong phase / plane skipped or misplaced the channel of the misplaced tap is far off, and the message names it"""
    import torch.nn.functional as F
    from lib.hip import ops

    N, H, W, Cin, Cout = 2, 15, 21, 32, 64
    g = torch.Generator().manual_seed(91)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 5, 5), generator=g) * (1.0 / np.sqrt(25 * Cin))
    w[:25] = 0.0
    for k in range(25):
        w[k, k, k // 5, k % 5] = 1.0
    ref = F.conv2d(x.double(), w.double(), None, stride=2, padding=2).permute(0, 2, 3, 1).numpy()
    wp = ops.winograd5x5s2_pack_weight(w.to("cuda:0"))
    bias = torch.zeros((Cout,), device="cuda:0")
    y = ops.conv2d_fwd_winograd5x5s2(x.permute(0, 2, 3, 1).contiguous().to("cuda:0"), Cin, wp, bias, Cout, slope=1.0, tile=3).cpu().numpy()
    assert np.isfinite(y).all()
    bar = 1e-4 * np.abs(ref).max() + 2e-5
    err = np.abs(y - ref).max(axis=(0, 1, 2))
    bad = ["tap (%d,%d): %.2e" % (k // 5, k % 5, err[k]) for k in range(25) if err[k] > bar]
    assert not bad, bad
    assert err.max() <= bar, (int(err.argmax()), err.max())
