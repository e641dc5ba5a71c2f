"""GPU: the 5x5 / stride-2 forward with an item map (csrc/wino_balance.hip) gives the bits of the forward without one.

N = 2, H = W = 68 -> 34 x 34 outputs, 9 x 9 tiles per image, T = 162 GEMM rows = two row tiles of 128, the second partly empty.
DIM_WINO_MAX_G caps the stream-K ranges at 7 or 13, so that a range is several items long (with the device's own G every range of
so small a problem is one item and nothing can change places) and most range boundaries fall inside an item."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 2, 68, 68
LAYERS = [(32, 128, 4), (64, 128, 4), (64, 256, 5)]   # (Cin, Cout, GEMM tile): 4 or 8 chunks per item


@pytest.fixture(params=[1, 0], ids=["bf16x3", "f32pipe"])
def wino_split(request, hip_lib):
    """both arithmetics of the plane GEMMs; the f32 matrix pipe ignores the table"""
    from lib.hip import ops

    ops.set_winograd_split(bool(request.param))
    yield request.param
    ops.set_winograd_split(True)


@functools.lru_cache(maxsize=None)
def problem(cin, cout):
    """inputs and the float64 reference of one layer, computed once and shared (read-only)"""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(100 * cin + cout)
    x = torch.randn((N, cin, H, W), generator=g)
    w = torch.randn((cout, cin, 5, 5), generator=g) * (1.0 / np.sqrt(25 * cin))
    b = torch.randn((cout,), generator=g) * 0.1
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=2), 0.1).permute(0, 2, 3, 1).numpy()
    return x.permute(0, 2, 3, 1).contiguous(), w, b, ref


@pytest.mark.parametrize("max_g", [7, 13])
@pytest.mark.parametrize("cin,cout,tile", LAYERS)
def test_item_map_keeps_the_bits(hip_lib, monkeypatch, wino_split, cin, cout, tile, max_g):
    from lib.hip import ops

    monkeypatch.setenv("DIM_WINO_MAX_G", str(max_g))
    x, w, b, ref = problem(cin, cout)
    xd, bd = x.to("cuda:0"), b.to("cuda:0")
    wp = ops.winograd5x5s2_pack_weight(w.to("cuda:0"))
    item_map = ops.wino_item_map_create(N, H, W, cin, cout, tile)
    hdr, table = item_map.query()
    print("Cin {} Cout {} tile {} G {}: live max {} -> {}, {} of {} slots moved".format(
        cin, cout, tile, hdr["G"], hdr["live_max_before"], hdr["live_max_after"], hdr["moved"], hdr["items"]))
    assert (hdr["T"], hdr["K"], hdr["Cout"], hdr["tile"], hdr["G"]) == (162, 4 * cin, cout, tile, max_g)
    assert hdr["moved"] > 0 and sorted(table.tolist()) == list(range(hdr["items"]))

    def run(m):
        return ops.conv2d_fwd_winograd5x5s2(xd, cin, wp, bd, cout, slope=0.1, tile=tile, item_map=m).cpu()

    plain, mapped, again = run(None), run(item_map), run(item_map)
    assert torch.equal(mapped, plain)
    assert torch.equal(again, mapped)
    bar = 1e-4 * np.abs(ref).max() + 2e-5
    for y in (plain, mapped):
        assert np.abs(y.numpy() - ref).max() <= bar
    other = ops.wino_item_map_create(1, H, W, cin, cout, tile)   # T = 81: not this run's plan -> the plain forward
    assert other.query()[0]["T"] == 81
    assert torch.equal(run(other), plain)
