"""tests/guard_arena.py on CPU tensors: the layout it promises, and negative controls -- a write of one word just past or just before
the payload, or into a neighbouring channel of a window, must make the check fail and name the word; an exact-size write passes."""
import numpy as np
import pytest
import torch

import guard_arena as ga

CPU = "cpu"


def _words(t):
    return t.contiguous().view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF


@pytest.mark.parametrize("numel,dtype", [(1, torch.float32), (1000, torch.float32), (77, torch.float64), (13, torch.int32),
                                          (5, torch.bfloat16), (0, torch.float32), (300000, torch.float32)])
def test_layout(numel, dtype):
    a = ga.GuardArena(numel, dtype=dtype, device=CPU, fill=ga.INF_WORD)
    v = a.view()
    assert v.numel() == numel and v.dtype == dtype and (numel == 0 or v.data_ptr() == a.address())
    assert a.address() % 256 == 0
    assert a.begin >= ga.MIN_GUARD_BYTES and a.flat.numel() - a.end >= ga.MIN_GUARD_BYTES
    assert a.begin >= a.nbytes and a.flat.numel() - a.end >= a.nbytes          # guards at least as large as the payload
    if a.nbytes % 4 == 0 and numel:
        assert (_words(a.payload_bytes()) == ga.INF_WORD).all()
    front = a.flat[a.begin - 4096:a.begin]
    assert front.data_ptr() % 4 == 0 and (_words(front) == ga.GUARD_WORD).all()
    a.check("untouched")
    v.zero_()                                                                   # an exact-size write passes
    a.check("exact-size write")
    if dtype == torch.float32 and numel:
        assert np.isnan(np.float32(ga.GuardArena(numel, device=CPU).view()[0]))  # the default fill is NaN
        assert torch.isinf(ga.GuardArena(numel, device=CPU, fill=ga.INF_WORD).view()).all()


@pytest.mark.parametrize("align,phase", [(16, 8), (8, 4), (4, 0), (256, 64), (16, 0)])
def test_alignment_is_exactly_the_requested_one(align, phase):
    a = ga.GuardArena(24, dtype=torch.int32, device=CPU, align=align, phase=phase)
    assert a.address() % align == phase
    a.view().fill_(5)
    a.check("aligned payload")
    with pytest.raises(ValueError):
        ga.GuardArena(3, dtype=torch.float64, device=CPU, align=16, phase=4)     # not a multiple of the element size


def test_view_aliases_the_payload_and_fills():
    a = ga.GuardArena(24, device=CPU, fill=ga.ZERO_WORD)
    v = a.view((2, 3, 4))
    assert v.shape == (2, 3, 4) and float(v.abs().sum()) == 0.0
    v[1, 2, 3] = 6.5
    assert float(a.view()[23]) == 6.5
    a.fill(ga.NAN_WORD)
    assert torch.isnan(v).all()
    a.fill_from(torch.arange(5, dtype=torch.float32))
    np.testing.assert_array_equal(a.view().numpy(), np.arange(24) % 5)
    a.fill_from(torch.arange(100, dtype=torch.float32))
    np.testing.assert_array_equal(a.view().numpy(), np.arange(24))
    a.check("fills stay inside")


def test_one_word_past_the_payload_fails():
    a = ga.GuardArena(100, device=CPU)
    a.flat[a.end:a.end + 4].view(torch.float32)[0] = 1.0
    with pytest.raises(AssertionError, match=r"behind the payload: words 100 \.\. 100 "):
        a.check("overrun")


def test_one_word_before_the_payload_fails():
    a = ga.GuardArena(100, device=CPU)
    a.flat[a.begin - 4:a.begin].view(torch.float32)[0] = 0.0
    with pytest.raises(AssertionError, match=r"before the payload: words -1 \.\. -1 "):
        a.check("underrun")


def test_first_and_last_touched_word_are_named():
    a = ga.GuardArena(64, device=CPU)
    a.flat[a.end + 8:a.end + 12] = 0
    a.flat[a.end + 4000:a.end + 4004] = 0
    with pytest.raises(AssertionError, match=r"words 66 \.\. 1064 "):
        a.check("two stray stores")


def test_far_end_of_a_guard_is_watched():
    a = ga.GuardArena(8, device=CPU)
    a.flat[-1] = 0
    with pytest.raises(AssertionError, match="behind the payload"):
        a.check("last byte")
    b = ga.GuardArena(8, device=CPU)
    b.flat[0] = 0
    with pytest.raises(AssertionError, match="before the payload"):
        b.check("first byte")


def test_window_exact_write_passes_and_neighbour_fails():
    w = ga.ChannelWindow((2, 3, 12), 4, 6, device=CPU)
    assert torch.isnan(w.tensor).all()
    w.tensor[..., 4:10] = 1.5                                                   # exactly the window
    w.check("window write")
    np.testing.assert_array_equal(w.inside(), np.full((2, 3, 6), 1.5, dtype=np.float32))
    w.tensor[1, 2, 10] = 1.5                                                    # the channel behind it
    with pytest.raises(AssertionError, match=r"channel 10 of row 5 "):
        w.check("neighbour behind")
    w2 = ga.ChannelWindow((5, 12), 4, 6, device=CPU)
    w2.tensor[0, 3] = 0.0                                                       # the channel before it
    with pytest.raises(AssertionError, match=r"channel 3 of row 0 "):
        w2.check("neighbour before")


def test_window_rewriting_the_sentinel_value_with_other_bits_fails():
    """bit for bit: another NaN is not the sentinel"""
    w = ga.ChannelWindow((4, 8), 0, 4, device=CPU)
    w.tensor[2, 5] = float("nan")
    with pytest.raises(AssertionError, match="channel 5 of row 2"):
        w.check("another NaN")


def test_window_guards_are_checked_too():
    w = ga.dense((3, 8), device=CPU)
    w.tensor.fill_(2.0)
    w.check("dense write")
    w.arena.flat[w.arena.end:w.arena.end + 4] = 0
    with pytest.raises(AssertionError, match="behind the payload: words 24 .. 24 "):
        w.check("one word past a dense output")
    with pytest.raises(ValueError):
        ga.ChannelWindow((3, 8), 4, 6, device=CPU)
