"""The colour-segmentation kernels of csrc/track_seg.hip on the device, each through its lib.hip.ops wrapper, against
tests/track_seg_reference.py (the rule of include/deepim_hip.h in numpy):
  dim_track_seg_mask    mask bit for bit and counts exactly: boxes inside the frame, cut by every border, of one pixel, empty and wholly
                        outside; a track without a model; histograms with ties, NaN and inf; the status bit; outputs and workspace
                        between guard words, NaN-filled workspace, a second call on dirty outputs
  dim_track_seg_learn   counts and seg_age exactly, seg_hist bit for bit (both sides IEEE float32 division, subtraction, multiplication,
                        addition), skipped tracks untouched, depth_fg NULL and given, depth planes with 0, negatives, NaN and +inf, a
                        chain of three updates from the device's own state, every pixel in one bin
  both                  every argument error returns DIM_ERR_ARG with nothing written"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_seg_reference as S  # noqa: E402
from guard_arena import NAN_WORD, SENTINEL_WORD, GuardArena  # noqa: E402

DEV = "cuda:0"
# (P, H, W, bits): a lone track with 8 bins (one word of the bit table); the 16-byte path; the one-pixel path (W % 4 != 0) with the
# largest LDS-counted histogram; more tracks than a block has waves; several tiles and bands with the full 32768-bin histogram
SHAPES = [(1, 4, 8, 1), (3, 5, 12, 2), (3, 5, 13, 3), (17, 6, 16, 2), (2, 40, 64, 5)]
SKIP_BIT = 4096


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def box_kinds(H, W):
    """{min_x, max_x, min_y, max_y}: inside, cut by left and top, cut by right and bottom, empty (as the rasteriser returns it), wholly
    outside on either side (further than the largest margin), one pixel, cut by all four borders, inverted on one axis only"""
    return [(1, W - 2, 1, H - 2), (-3, W // 2, -2, H // 2), (W // 2, W + 5, H // 2, H + 4), (W, -1, H, -1), (W + 10, W + 20, 0, H - 1),
            (-20, -12, 0, 3), (2, 2, 1, 1), (-4, W + 3, -4, H + 3), (1, W - 2, 2, 1)]


def boxes(P, H, W, shift):
    kinds = box_kinds(H, W)
    return np.asarray([kinds[(p + shift) % len(kinds)] for p in range(P)], np.int32)


def frame(rng, H, W, cell=2):
    """colour cells of `cell` pixels from a small palette: neighbours share bins, and every bin of a coarse histogram is hit"""
    base = rng.randint(0, 256, size=((H + cell - 1) // cell, (W + cell - 1) // cell, 3))
    return np.kron(base, np.ones((cell, cell, 1), np.int64))[:H, :W].astype(np.uint8)


def histograms(rng, P, NB):
    h = rng.randint(0, 4, size=(P, 2, NB)).astype(np.float32) / np.float32(4)    # many ties
    h[:, 0] += (rng.randint(0, 2, size=(P, NB)) * 0.5).astype(np.float32)      # ... and a foreground that wins more often than not
    flat = h.reshape(-1)
    n = max(flat.size // 16, 4)
    for value in (np.nan, np.inf, -np.inf):
        flat[rng.randint(0, flat.size, size=n)] = value
    return h


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for P, H, W, bits in SHAPES:
        rng = np.random.RandomState(100 * P + W + bits)
        NB = 1 << (3 * bits)
        age = rng.randint(1, 5, size=P).astype(np.int32)
        age[rng.randint(0, P)] = 0
        out[(P, H, W, bits)] = dict(frames=[frame(rng, H, W) for _ in range(3)], hist=histograms(rng, P, NB), age=age)
    return out


# ------------------------------------------------------------------------------------------------ mask
@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("P,H,W,bits", SHAPES)
def test_mask_matches_reference(ops, scenes, P, H, W, bits, radius):
    sc = scenes[(P, H, W, bits)]
    fr, hist = sc["frames"][0], sc["hist"]
    d_fr, d_hist = dev(fr), dev(hist)
    all_fg = np.stack([np.ones_like(hist[:, 0]), np.zeros_like(hist[:, 1])], axis=1)
    n_kinds = len(box_kinds(H, W))
    seen_fg = seen_nomodel = False
    mask, cnt = GuardArena(P * H * W), GuardArena(2 * P, dtype=torch.int32)
    work = GuardArena(ops.lib().dim_track_seg_workspace_bytes(P, H, W, bits) // 4, dtype=torch.int32)
    for margin in (0, 1, 3):
        for shift in range(0, n_kinds, 1 if P < 3 else 3):
            bb = boxes(P, H, W, shift)
            models = [(hist, d_hist, sc["age"])]
            if P == 1:   # the lone track with a model as well, and with one that calls every colour foreground
                models += [(hist, d_hist, np.ones(P, np.int32)), (all_fg, dev(all_fg), np.ones(P, np.int32))]
            for hist, d_hist, age in models:
                want_mask, want_cnt, want_bits = S.seg_mask(fr, bb, hist, age, bits, margin, radius)
                mask.fill(SENTINEL_WORD), cnt.fill(SENTINEL_WORD), work.fill(NAN_WORD)
                status = dev(np.full(P, 5, np.int32))
                for call in ("first", "second, on what the first left"):
                    ops.track_seg_mask(d_fr, dev(bb), d_hist, dev(age), bits, margin, radius, mask=mask.view((P, 1, H, W)),
                                       counts=cnt.view((P, 2)), status=status, workspace=work.view())
                    what = "mask P {} {}x{} bits {} radius {} margin {} shift {}: {} call".format(P, H, W, bits, radius, margin, shift, call)
                    for a in (mask, cnt, work):
                        a.check(what)
                    got_mask, got_cnt = host(mask.view((P, 1, H, W))), host(cnt.view((P, 2)))
                    assert np.array_equal(got_cnt, want_cnt), (what, got_cnt, want_cnt)
                    assert got_mask.tobytes() == want_mask.tobytes(), what
                    assert np.array_equal(host(status), 5 | want_bits), what
                seen_fg = seen_fg or (want_cnt[:, 1] > 0).any()
                seen_nomodel = seen_nomodel or (want_bits != 0).any()
    assert seen_fg and seen_nomodel, "the scenes mark nothing: the comparison guards nothing"


def test_mask_on_an_unaligned_plane_and_without_status(ops, scenes):
    """W % 4 == 0 but the mask starts 4 bytes off a 16-byte boundary: the same bits through scalar stores; status may be NULL"""
    P, H, W, bits = 3, 5, 12, 2
    sc = scenes[(P, H, W, bits)]
    bb, age = boxes(P, H, W, 0), np.ones(P, np.int32)
    want_mask, want_cnt, _ = S.seg_mask(sc["frames"][0], bb, sc["hist"], age, bits, 1, 1)
    mask = GuardArena(P * H * W, fill=SENTINEL_WORD, align=16, phase=4)
    _, cnt = ops.track_seg_mask(dev(sc["frames"][0]), dev(bb), dev(sc["hist"]), dev(age), bits, 1, 1, mask=mask.view((P, 1, H, W)))
    mask.check("unaligned mask")
    assert np.array_equal(host(cnt), want_cnt) and host(mask.view((P, 1, H, W))).tobytes() == want_mask.tobytes()


# ------------------------------------------------------------------------------------------------ learn
def depth_planes(rng, P, H, W):
    """depth_drawn from the boundary values; depth_fg: the same plane with some drawn pixels hidden (0) -- and a few junk values"""
    pool = np.asarray([0.0, -1.0, np.nan, np.inf, 0.5, 0.75, 0.5, 0.75, 1e-30], np.float32)
    drawn = pool[rng.randint(0, len(pool), size=(P, 1, H, W))]
    fg = np.where(rng.rand(P, 1, H, W) < 0.3, np.float32(0), drawn).astype(np.float32)
    junk = rng.rand(P, 1, H, W) < 0.1
    fg[junk] = pool[rng.randint(0, len(pool), size=int(junk.sum()))]
    return drawn, fg


@pytest.mark.parametrize("with_fg", [False, True], ids=["fg-null", "fg-given"])
@pytest.mark.parametrize("P,H,W,bits", SHAPES)
def test_learn_chain_matches_reference(ops, scenes, P, H, W, bits, with_fg):
    sc = scenes[(P, H, W, bits)]
    NB = 1 << (3 * bits)
    rng = np.random.RandomState(7 * P + H + bits)
    min_pixels, margin = 3, 1
    hist = GuardArena(P * 2 * NB, fill=SENTINEL_WORD)
    hist.view((P, 2, NB)).copy_(dev(np.nan_to_num(sc["hist"], nan=0.25, posinf=0.5, neginf=0.0)))
    age_t = dev(np.where(np.arange(P) % 2 == 0, 0, sc["age"]).astype(np.int32))
    if P > 1:
        age_t[P - 1] = (1 << 30) - 1     # reaches the cap on the first update and stays there
    cnt = GuardArena(2 * P, dtype=torch.int32, fill=SENTINEL_WORD)
    work = GuardArena(ops.lib().dim_track_seg_workspace_bytes(P, H, W, bits) // 4, dtype=torch.int32)   # NaN bits
    n_kinds = len(box_kinds(H, W))
    updated = skipped = 0
    for step, (rate, shift) in enumerate(((0.25, 0), (0.1, 1), (1.0, 7))):
        fr = sc["frames"][step]
        drawn, fg = depth_planes(rng, P, H, W)
        bb = boxes(P, H, W, shift if P > 1 else (0, 7, 6)[step])
        flags = rng.randint(0, 2, size=P).astype(np.int32) * 64
        if P > 1:
            flags[step % P] |= SKIP_BIT
        before_h, before_a = host(hist.view((P, 2, NB))), host(age_t)
        want_h, want_a, want_c = S.seg_learn(fr, drawn, fg if with_fg else None, bb, flags, SKIP_BIT, bits, margin, rate, min_pixels, before_h,
                                             before_a)
        ops.track_seg_learn(dev(fr), dev(drawn), dev(bb), hist.view((P, 2, NB)), age_t, bits, margin, rate, min_pixels,
                            depth_fg=dev(fg) if with_fg else None, flags=dev(flags), skip_mask=SKIP_BIT, counts=cnt.view((P, 2)),
                            workspace=work.view())
        what = "learn P {} {}x{} bits {} step {}".format(P, H, W, bits, step)
        for a in (hist, cnt, work):
            a.check(what)
        got_h, got_a, got_c = host(hist.view((P, 2, NB))), host(age_t), host(cnt.view((P, 2)))
        assert np.array_equal(got_c, want_c), (what, got_c, want_c)
        assert np.array_equal(got_a, want_a), (what, got_a, want_a)
        assert got_h.tobytes() == want_h.tobytes(), (what, np.argwhere(got_h.view(np.uint32) != want_h.view(np.uint32))[:4])
        same = got_a == before_a
        for p in np.nonzero(same & (before_a < (1 << 30)))[0]:     # skipped: bit for bit
            assert got_h[p].tobytes() == before_h[p].tobytes(), (what, p)
        updated += int((got_a != before_a).sum())
        skipped += int(same.sum())
    assert updated > 0 and (skipped > 0 or P == 1), (updated, skipped)
    if P > 1:
        assert host(age_t)[P - 1] <= 1 << 30


def test_learn_without_flags_matches_reference(ops, scenes):
    P, H, W, bits = 2, 40, 64, 5
    sc, NB = scenes[(P, H, W, bits)], 1 << 15
    rng = np.random.RandomState(3)
    drawn, _ = depth_planes(rng, P, H, W)
    bb = np.asarray([(5, 50, 4, 30), (20, 70, -3, 44)], np.int32)
    hist, age = dev(np.zeros((P, 2, NB), np.float32)), dev(np.zeros(P, np.int32))
    want_h, want_a, want_c = S.seg_learn(sc["frames"][1], drawn, None, bb, None, 0, bits, 3, 0.1, 64, host(hist), host(age))
    cnt = ops.track_seg_learn(dev(sc["frames"][1]), dev(drawn), dev(bb), hist, age, bits, 3, 0.1, 64)
    assert np.array_equal(host(cnt), want_c) and np.array_equal(host(age), want_a) and want_a.tolist() == [1, 1]
    assert host(hist).tobytes() == want_h.tobytes()
    for k in range(2):
        assert abs(float(want_h[0, k].astype(np.float64).sum()) - 1.0) < 1e-4     # each histogram sums to about 1


@pytest.mark.parametrize("P,H,W,bits", [(3, 5, 12, 2), (2, 40, 64, 5)], ids=["lds-counters", "global-counters"])
def test_learn_with_every_pixel_in_one_bin(ops, P, H, W, bits):
    """the contended case of the atomics: one colour over the whole frame, so each class of a track adds into one counter"""
    NB = 1 << (3 * bits)
    fr = np.empty((H, W, 3), np.uint8)
    fr[:] = (200, 17, 99)
    drawn = np.zeros((P, 1, H, W), np.float32)
    drawn[:, :, H // 4:3 * H // 4, W // 4:3 * W // 4] = 0.5
    bb = np.asarray([(0, W - 1, 0, H - 1)] * P, np.int32)
    hist, age = dev(np.zeros((P, 2, NB), np.float32)), dev(np.zeros(P, np.int32))
    cnt = ops.track_seg_learn(dev(fr), dev(drawn), dev(bb), hist, age, bits, 0, 0.1, 1)
    want_h, want_a, want_c = S.seg_learn(fr, drawn, None, bb, None, 0, bits, 0, 0.1, 1, np.zeros((P, 2, NB), np.float32), np.zeros(P, np.int32))
    n_f = (3 * H // 4 - H // 4) * (3 * W // 4 - W // 4)
    assert np.array_equal(host(cnt), want_c) and want_c.tolist() == [[n_f, H * W - n_f]] * P
    got = host(hist)
    assert got.tobytes() == want_h.tobytes()
    c = int(S.color_bins(fr[:1, :1], bits)[0, 0])
    assert (got[:, :, c] == 1.0).all() and got.sum() == 2 * P


# ------------------------------------------------------------------------------------------------ argument errors
def test_entries_refuse_bad_arguments(ops):
    P, H, W, bits = 2, 4, 8, 2
    NB = 1 << (3 * bits)
    lib, cur = ops.lib(), ops.current_stream()
    fr, bb = dev(np.zeros((H, W, 3), np.uint8)), dev(np.asarray([(0, W - 1, 0, H - 1)] * P, np.int32))
    depth = dev(np.full((P, 1, H, W), 0.5, np.float32))
    outs = dict(mask=GuardArena(P * H * W, fill=SENTINEL_WORD), counts=GuardArena(2 * P, dtype=torch.int32, fill=SENTINEL_WORD),
                hist=GuardArena(P * 2 * NB, fill=SENTINEL_WORD), age=GuardArena(P, dtype=torch.int32, fill=SENTINEL_WORD),
                status=GuardArena(P, dtype=torch.int32, fill=SENTINEL_WORD),
                work=GuardArena(lib.dim_track_seg_workspace_bytes(P, H, W, bits) // 4, dtype=torch.int32, fill=SENTINEL_WORD))
    before = {k: host(a.view()).tobytes() for k, a in outs.items()}
    ptr = {k: a.address() for k, a in outs.items()}

    def mask_args(**kw):
        a = dict(frame=fr.data_ptr(), bbox=bb.data_ptr(), hist=ptr["hist"], age=ptr["age"], P=P, H=H, W=W, bits=bits, margin=1, radius=1,
                 work=ptr["work"], mask=ptr["mask"], counts=ptr["counts"], status=ptr["status"])
        a.update(kw)
        return [a[k] for k in ("frame", "bbox", "hist", "age", "P", "H", "W", "bits", "margin", "radius", "work", "mask", "counts", "status")]

    def learn_args(**kw):
        a = dict(frame=fr.data_ptr(), drawn=depth.data_ptr(), fg=None, bbox=bb.data_ptr(), flags=None, skip=0, P=P, H=H, W=W, bits=bits,
                 margin=1, rate=0.1, min_pixels=1, work=ptr["work"], hist=ptr["hist"], age=ptr["age"], counts=ptr["counts"])
        a.update(kw)
        return [a[k] for k in ("frame", "drawn", "fg", "bbox", "flags", "skip", "P", "H", "W", "bits", "margin", "rate", "min_pixels", "work",
                               "hist", "age", "counts")]

    shared = [dict(P=0), dict(P=-1), dict(H=0), dict(W=0), dict(H=4097, W=4096), dict(bits=0), dict(bits=6), dict(margin=-1),
              dict(frame=None), dict(bbox=None), dict(hist=None), dict(age=None), dict(work=None), dict(counts=None),
              dict(hist=ptr["hist"] + 2), dict(bbox=bb.data_ptr() + 1), dict(work=ptr["work"] + 4)]
    bad_mask = shared + [dict(radius=-1), dict(radius=5), dict(mask=None), dict(mask=ptr["mask"] + 2), dict(status=ptr["status"] + 1)]
    bad_learn = shared + [dict(rate=-0.01), dict(rate=1.5), dict(rate=float("nan")), dict(rate=float("inf")), dict(min_pixels=0),
                          dict(drawn=None), dict(drawn=depth.data_ptr() + 2), dict(fg=depth.data_ptr() + 1), dict(flags=ptr["status"] + 3)]
    for kw in bad_mask:
        assert lib.dim_track_seg_mask(*mask_args(**kw), cur) == -1, kw
        assert lib.dim_last_error().startswith(b"track_seg_mask"), kw
    for kw in bad_learn:
        assert lib.dim_track_seg_learn(*learn_args(**kw), cur) == -1, kw
        assert lib.dim_last_error().startswith(b"track_seg_learn"), kw
    for bad in ((0, H, W, bits), (P, 0, W, bits), (P, H, 0, bits), (P, H, W, 0), (P, H, W, 6)):
        assert lib.dim_track_seg_workspace_bytes(*bad) == 0
    for k, a in outs.items():
        a.check("argument errors: " + k)
        assert host(a.view()).tobytes() == before[k], "an argument error wrote into " + k
    # and the good calls go through on the same buffers
    outs["age"].view().fill_(0)
    depth[:, :, :, :W // 2] = 0.0     # half of every region is background
    assert lib.dim_track_seg_learn(*learn_args(), cur) == 0
    assert lib.dim_track_seg_mask(*mask_args(), cur) == 0
    assert host(outs["age"].view()).tolist() == [1, 1] and host(outs["counts"].view()).tolist() == [H * W, 0] * P
