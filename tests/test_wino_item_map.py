"""CPU: the item-slot permutation that evens out the live work of the stream-K ranges of the 5x5 / stride-2 plane GEMMs
(csrc/wino_balance.hip), read through dim_wino_item_map_plan -- host arithmetic, no device.

The live work of every range is recomputed here from the table alone (the phase masks of csrc/common.h wino5_phase_mask), so the
header's figures are checked against a second implementation."""
import numpy as np
import pytest

FLAGSHIP = [(19200, 256, 128, 4, 512),   # conv2 at 16 pairs: tile 4, two workgroups per CU
            (4800, 512, 256, 5, 256)]    # conv3 at 16 pairs: tile 5, one workgroup per CU
# the shapes of tests/test_gpu_wino_balance.py: N = 2, H = W = 68 -> T = 162 tile rows, K = 4 Cin
SMALL = [(162, 4 * cin, cout, tile, g) for cin, cout, tile in ((32, 128, 4), (64, 128, 4), (64, 256, 5)) for g in (7, 13)]
TILE_SHAPE = {4: (128, 128), 5: (128, 256)}


@pytest.fixture(scope="module")
def plan(hip_lib):
    from lib.hip import ops

    return ops.wino_item_map_plan


def phase_mask(p):
    return (0x3 if p >= 30 else 0xF) & (0x5 if p % 6 == 5 else 0xF)


def geometry(T, K, Cout, tile, G):
    BM, BN = TILE_SHAPE[tile]
    MT, NTN, nch = -(-T // BM), Cout // BN, K // 32
    items = 36 * MT * NTN
    per, rem = divmod(items * nch, G)
    first = [w * per + min(w, rem) for w in range(G + 1)]
    return MT, NTN, nch, items, per, rem, first


def live_per_range(table, T, K, Cout, tile, G):
    MT, NTN, nch, items, _, _, first = geometry(T, K, Cout, tile, G)
    q = nch // 4
    live = np.zeros((items, nch), dtype=np.int64)     # live[s][ch]: is chunk ch of slot s multiplied
    for s in range(items):
        m = phase_mask(int(table[s]) // NTN // MT)
        for ph in range(4):
            live[s, ph * q:(ph + 1) * q] = (m >> ph) & 1
    flat = live.reshape(-1)
    return np.array([flat[first[w]:first[w + 1]].sum() for w in range(G)])


def cut_slots(T, K, Cout, tile, G):
    nch, first = geometry(T, K, Cout, tile, G)[2], geometry(T, K, Cout, tile, G)[6]
    return sorted({first[w] // nch for w in range(1, G) if first[w] % nch})


@pytest.mark.parametrize("shape", FLAGSHIP + SMALL)
def test_table_is_a_permutation_with_fixed_cuts_and_no_worse_maximum(plan, shape):
    hdr, table = plan(*shape)
    MT, NTN, nch, items, per, rem, _ = geometry(*shape)
    assert (hdr["T"], hdr["K"], hdr["Cout"], hdr["tile"], hdr["G"]) == shape
    assert (hdr["items"], hdr["nch"], hdr["per"], hdr["rem"]) == (items, nch, per, rem)
    assert sorted(table.tolist()) == list(range(items))
    cuts = cut_slots(*shape)
    assert cuts, "no cut inside an item: the case checks nothing about fixed points"
    assert all(table[s] == s for s in cuts)
    before, after = live_per_range(np.arange(items), *shape), live_per_range(table, *shape)
    print("{}: live per range before min {} mean {:.1f} max {}, after min {} mean {:.1f} max {}, moved {}".format(
        shape, before.min(), before.mean(), before.max(), after.min(), after.mean(), after.max(), hdr["moved"]))
    assert before.sum() == after.sum()
    assert (hdr["live_max_before"], hdr["live_max_after"]) == (before.max(), after.max())
    assert after.max() <= before.max()
    assert hdr["moved"] == int((table != np.arange(items)).sum())
    assert (hdr["moved"] == 0) == (after.max() == before.max())   # nothing gained: identity


@pytest.mark.parametrize("shape", FLAGSHIP + SMALL)
def test_builder_is_deterministic(plan, shape):
    (h0, t0), (h1, t1) = plan(*shape), plan(*shape)
    assert h0 == h1 and np.array_equal(t0, t1)


@pytest.mark.parametrize("shape", FLAGSHIP)
def test_flagship_maximum_is_within_half_an_item_of_the_mean(plan, shape):
    hdr, table = plan(*shape)
    after = live_per_range(table, *shape)
    assert hdr["moved"] > 0
    assert after.max() <= after.mean() + hdr["nch"] / 2, (after.max(), after.mean())


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_move_items(plan, shape):
    """the GPU test's shapes are not vacuous, and a range stays within the 64 slots a workgroup keeps in one register"""
    hdr, _ = plan(*shape)
    assert hdr["moved"] > 0 and hdr["live_max_after"] < hdr["live_max_before"]
    assert hdr["per"] // hdr["nch"] + 2 <= 64


@pytest.mark.parametrize("shape", FLAGSHIP + SMALL)
def test_identity_without_skipping(plan, shape):
    hdr, table = plan(*shape, skip5=False)
    assert hdr["moved"] == 0 and np.array_equal(table, np.arange(hdr["items"]))


def test_identity_when_a_range_needs_more_than_64_slots(plan):
    hdr, table = plan(19200, 128, 128, 4, 7)     # 5400 items of 4 chunks in 7 ranges
    assert hdr["per"] // hdr["nch"] > 64
    assert hdr["moved"] == 0 and np.array_equal(table, np.arange(hdr["items"]))
