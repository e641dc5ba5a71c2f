"""CPU: the numpy restatement of the tracker's colour segmentation (tests/track_seg_reference.py) against its own definitions, the
settings and refusals of deepim.core.tracker for TEST.TRACK_SEG, the colour ranges of the synthetic video, and a sanity run of the
reference alone on toy frames."""
import numpy as np
import pytest

import track_seg_reference as S


# ---------------------------------------------------------------- the majority filter
@pytest.mark.parametrize("radius", [0, 1, 2, 4])
def test_box_sum_majority_equals_the_definition(radius):
    H, W = 9, 11
    rng = np.random.RandomState(radius)
    # regions touching every border, one-pixel regions (a corner, an edge, the inside), the whole frame, and none
    regions = [(0, W - 1, 0, H - 1), (0, 4, 0, 3), (6, W - 1, 5, H - 1), (0, W - 1, 3, 3), (4, 4, 0, H - 1), (0, 0, 0, 0), (W - 1, W - 1, 4, 4),
               (5, 5, 4, 4), (2, 8, 1, 7), None]
    for reg in regions:
        inside = S.region_plane(reg, H, W)
        for density in (0.3, 0.5, 0.8):
            raw = (rng.rand(H, W) < density) & inside
            got, want = S.majority(raw, inside, radius), S.majority_brute(raw, inside, radius)
            assert np.array_equal(got, want), (reg, radius, density)
            if radius == 0:
                assert np.array_equal(got, raw)
            if reg is None:
                assert not got.any()


def test_region_rule():
    H, W = 10, 20
    assert S.region((3, 8, 2, 5), 0, H, W) == (3, 8, 2, 5)
    assert S.region((3, 8, 2, 5), 4, H, W) == (0, 12, 0, 9)
    assert S.region((W, -1, H, -1), 50, H, W) is None          # the rasteriser's empty box stays empty whatever the margin
    assert S.region((3, 8, 5, 4), 2, H, W) is None             # inverted on one axis
    assert S.region((25, 30, 2, 5), 3, H, W) is None           # outside after clipping
    assert S.region((25, 30, 2, 5), 6, H, W) == (19, 19, 0, 9)
    assert S.region((-9, -2, 2, 5), 2, H, W) == (0, 0, 0, 7)
    assert S.color_bins(np.asarray([[[255, 0, 128]]], np.uint8), 2)[0, 0] == (3 << 4) | (0 << 2) | 2


def test_mask_rule_on_a_hand_made_case():
    """2 bits: the frame holds two colours; the model calls one foreground.  A tie and a NaN are background"""
    H, W, bits = 6, 8, 2
    fr = np.zeros((H, W, 3), np.uint8)
    fr[:, 4:] = (255, 255, 255)
    a, b = int(S.color_bins(fr, bits)[0, 0]), int(S.color_bins(fr, bits)[0, 7])
    hist = np.zeros((3, 2, 64), np.float32)
    hist[0, 0, b], hist[0, 1, b] = 0.6, 0.5                      # b foreground
    hist[1, 0, b], hist[1, 1, b] = 0.5, 0.5                      # a tie
    hist[2, 0, b], hist[2, 1, b] = np.nan, 0.1                   # NaN
    hist[:, 0, a], hist[:, 1, a] = 0.1, 0.9
    box = np.asarray([(1, 6, 1, 4)] * 3, np.int32)
    mask, counts, status = S.seg_mask(fr, box, hist, np.asarray([1, 1, 1], np.int32), bits, 0, 0)
    want = np.zeros((H, W), np.float32)
    want[1:5, 4:7] = 1
    assert np.array_equal(mask[0, 0], want) and not mask[1:].any() and not status.any()
    assert counts.tolist() == [[24, 12], [24, 0], [24, 0]]
    mask, counts, status = S.seg_mask(fr, box, hist, np.asarray([0, 1, 1], np.int32), bits, 0, 0)
    assert not mask.any() and status.tolist() == [S.STATUS_TRACK_SEG_NO_MODEL, 0, 0] and counts[0].tolist() == [24, 0]


# ---------------------------------------------------------------- the learn rule, branch by branch
def _learn_scene():
    H, W, bits = 8, 12, 2
    rng = np.random.RandomState(4)
    fr = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    depth = np.zeros((1, 1, H, W), np.float32)
    depth[0, 0, 2:6, 3:9] = 0.5                     # 24 foreground pixels; the frame's other 72 are background at margin >= 3
    box = np.asarray([(3, 8, 2, 5)], np.int32)
    return fr, depth, box, bits


def test_learn_branch_table():
    fr, depth, box, bits = _learn_scene()
    NB = 64
    old = np.full((1, 2, NB), 1.0 / NB, np.float32)
    call = lambda flags, min_pixels, hist, age, rate=0.25, margin=8: S.seg_learn(  # noqa: E731
        fr, depth, None, box, flags, 4096, bits, margin, rate, min_pixels, hist, np.asarray([age], np.int32))
    bins = S.color_bins(fr, bits)
    h_f = np.bincount(bins[2:6, 3:9].ravel(), minlength=NB).astype(np.float32) / np.float32(24)
    # skipped by flag: the counts are still written
    hist, age, counts = call(np.asarray([4096 | 1], np.int32), 1, old, 3)
    assert hist.tobytes() == old.tobytes() and age.tolist() == [3] and counts.tolist() == [[24, 72]]
    # a flag outside the mask does not skip
    assert call(np.asarray([8192], np.int32), 1, old, 3)[1].tolist() == [4]
    # skipped by the foreground count, and by the background count (margin 0: the region is the box, no background in it)
    for min_pixels, margin, want in ((25, 8, [24, 72]), (1, 0, [24, 0]), (73, 8, [24, 72])):
        hist, age, counts = call(None, min_pixels, old, 3, margin=margin)
        assert hist.tobytes() == old.tobytes() and age.tolist() == [3] and counts.tolist() == [want]
    # first update: the frame's histograms as they are, whatever the old rows held (NaN included) and whatever the rate
    junk = np.full((1, 2, NB), np.nan, np.float32)
    hist, age, _ = call(None, 24, junk, 0, rate=0.0)
    assert age.tolist() == [1] and hist[0, 0].tobytes() == h_f.tobytes() and abs(float(hist[0, 1].sum()) - 1) < 1e-6
    assert call(None, 24, junk, -5)[1].tolist() == [1]
    # blended update: float32, each operation rounded once
    hist, age, _ = call(None, 1, old, 1)
    want = old[0, 0] + np.float32(0.25) * (h_f - old[0, 0])
    assert want.dtype == np.float32 and hist[0, 0].tobytes() == want.tobytes() and age.tolist() == [2]
    assert call(None, 1, old, 1, rate=0.0)[0].tobytes() == old.tobytes()
    assert call(None, 1, old, 1, rate=1.0)[0][0, 0].tobytes() == (old[0, 0] + (h_f - old[0, 0])).tobytes()
    # the age cap
    assert call(None, 1, old, (1 << 30) - 1)[1].tolist() == [1 << 30]
    hist, age, _ = call(None, 1, old, 1 << 30)
    assert age.tolist() == [1 << 30] and hist.tobytes() != old.tobytes()


def test_learn_classes_with_a_visible_plane():
    """depth_fg given: drawn but hidden is neither class; values that are not a depth (0, negative, NaN, +inf) are not drawn"""
    fr, depth, box, bits = _learn_scene()
    fg = depth.copy()
    fg[0, 0, 2:6, 3:5] = 0.0                        # 8 pixels hidden
    depth[0, 0, 0, 0], depth[0, 0, 0, 1], depth[0, 0, 0, 2], depth[0, 0, 0, 3] = -1.0, np.nan, np.inf, 0.0
    _, _, counts = S.seg_learn(fr, depth, fg, box, None, 0, bits, 8, 0.1, 1, np.zeros((1, 2, 64), np.float32), np.zeros(1, np.int32))
    assert counts.tolist() == [[16, 72]]


# ---------------------------------------------------------------- settings and refusals
@pytest.fixture
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    config.TEST.INIT_MASK = "box_rendered"
    yield config
    reset_config()


def test_segmentation_defaults(cfg):
    from deepim.core.tracker import segmentation_settings, track_settings

    assert segmentation_settings(cfg) == dict(mode="none", bits=5, margin=16, radius=2, rate=0.1, min_pixels=64)
    # track_settings is what it was
    assert track_settings(cfg) == dict(motion="velocity", damping=1.0, window=10, lost_rot_deg=10.0, lost_trans=0.01, score="none",
                                       min_score=0.5, depth_tau=0.02, pose="loop")
    for key in ("TRACK_SEG", "TRACK_SEG_BITS", "TRACK_SEG_MARGIN", "TRACK_SEG_SMOOTH", "TRACK_SEG_RATE", "TRACK_SEG_MIN_PIXELS"):
        del cfg.TEST[key]     # a configuration from before the keys existed
    assert segmentation_settings(cfg) == dict(mode="none", bits=5, margin=16, radius=2, rate=0.1, min_pixels=64)


@pytest.mark.parametrize("key,bad", [("TRACK_SEG", "colour"), ("TRACK_SEG", None), ("TRACK_SEG_BITS", 0), ("TRACK_SEG_BITS", 6),
                                     ("TRACK_SEG_BITS", 2.5), ("TRACK_SEG_BITS", True), ("TRACK_SEG_MARGIN", -1), ("TRACK_SEG_MARGIN", 1.5),
                                     ("TRACK_SEG_SMOOTH", -1), ("TRACK_SEG_SMOOTH", 5), ("TRACK_SEG_SMOOTH", 0.5), ("TRACK_SEG_RATE", -0.1),
                                     ("TRACK_SEG_RATE", 1.01), ("TRACK_SEG_RATE", float("nan")), ("TRACK_SEG_RATE", float("inf")),
                                     ("TRACK_SEG_RATE", True), ("TRACK_SEG_MIN_PIXELS", 0), ("TRACK_SEG_MIN_PIXELS", 2.5)])
def test_segmentation_settings_name_the_bad_key(cfg, key, bad):
    from deepim.core.tracker import Tracker, segmentation_settings

    cfg.TEST[key] = bad
    with pytest.raises(ValueError, match="TEST." + key + r"\b"):
        segmentation_settings(cfg)
    with pytest.raises(ValueError, match="TEST." + key + r"\b"):    # and the constructor, before any device work
        Tracker(cfg, None, object(), 2)


def test_silhouette_stage_refusals(cfg):
    from deepim.core.tracker import Tracker, refuse_for_tracking, segmentation_settings, track_settings

    T = cfg.TEST
    T.SIL_ITER = 2
    with pytest.raises(ValueError, match=r"TEST\.SIL_ITER > 0 is not supported \(a frame carries no segmentation\)"):
        refuse_for_tracking(cfg)                                    # TRACK_SEG none: today's refusal, word for word
    with pytest.raises(ValueError, match=r"TEST\.SIL_ITER"):
        Tracker(cfg, None, object(), 2)
    T.TRACK_SEG = "color"
    refuse_for_tracking(cfg)
    assert segmentation_settings(cfg)["mode"] == "color"
    T.TRACK_POSE = "sil"
    assert track_settings(cfg)["pose"] == "sil"
    T.SIL_MASK = "pred"
    with pytest.raises(ValueError, match=r"TEST\.SIL_MASK"):
        segmentation_settings(cfg)
    with pytest.raises(ValueError, match=r"TEST\.SIL_MASK"):
        Tracker(cfg, None, object(), 2)
    T.SIL_MASK = "observed"
    T.TRACK_SEG_MARGIN, T.SIL_MAX_PX = 12, 12.5                     # ceil(12.5) = 13 > 12
    with pytest.raises(ValueError, match=r"TEST\.TRACK_SEG_MARGIN.*TEST\.SIL_MAX_PX"):
        segmentation_settings(cfg)
    T.TRACK_SEG_MARGIN = 13
    assert segmentation_settings(cfg)["margin"] == 13
    # TRACK_POSE sil needs the stage on, with or without a segmentation
    T.SIL_ITER = 0
    with pytest.raises(ValueError, match=r"TEST\.TRACK_POSE 'sil' needs its stage switched on \(TEST\.SIL_ITER > 0\)"):
        track_settings(cfg)
    # a margin below the gate is no matter while the stage is off
    T.TRACK_POSE, T.TRACK_SEG_MARGIN = "loop", 0
    assert segmentation_settings(cfg)["margin"] == 0


# ---------------------------------------------------------------- the synthetic video's colour ranges
def test_color_ranges_of_the_synthetic_video():
    from lib.dataset.synthetic_sequences import background, color_ranges, restrict_colors

    assert color_ranges(None, "x") is None
    assert color_ranges((96, 255), "x").tolist() == [[96, 255]] * 3
    assert color_ranges(((0, 10), (20, 30), (40, 50)), "x").tolist() == [[0, 10], [20, 30], [40, 50]]
    for bad in ((10, 5), (-1, 5), (0, 256), ((0, 1), (2, 3)), 7):
        with pytest.raises(ValueError, match="background_colors"):
            color_ranges(bad, "background_colors")
    bg = background(3, 16, 24)
    out = restrict_colors(bg, color_ranges(((0, 159), (10, 10), (200, 255)), "x"))
    assert out.dtype == np.uint8 and out.shape == bg.shape
    assert out[..., 0].max() <= 159 and (out[..., 1] == 10).all() and out[..., 2].min() >= 200
    assert np.array_equal(restrict_colors(bg, color_ranges((0, 255), "x")), bg)       # the full range is the identity
    ramp = np.arange(256, dtype=np.uint8).reshape(-1, 1, 1).repeat(3, axis=2)
    assert (np.diff(restrict_colors(ramp, color_ranges((96, 255), "x"))[:, 0, 0].astype(int)) >= 0).all()


# ---------------------------------------------------------------- the reference alone on toy frames
def _toy_frame(H, W, cx, cy, radius, seed, obj_range, bg_range, tex_seed=99):
    """a textured disc (4-pixel colour cells that move with it) over a seeded 4-pixel cell background -> (frame, depth, box)"""
    from lib.dataset.synthetic_sequences import color_ranges, restrict_colors

    rng = np.random.RandomState(seed)
    cells = lambda r, n: np.kron(r.randint(0, 256, size=(n, n, 3)), np.ones((4, 4, 1), np.int64)).astype(np.uint8)  # noqa: E731
    bg = restrict_colors(cells(rng, max(H, W) // 4 + 1)[:H, :W], color_ranges(bg_range, "bg"))
    tex = restrict_colors(cells(np.random.RandomState(tex_seed), 2 * radius // 4 + 2), color_ranges(obj_range, "obj"))
    yy, xx = np.mgrid[:H, :W]
    disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= radius ** 2
    fr = bg.copy()
    fr[disc] = tex[(yy - cy + radius)[disc], (xx - cx + radius)[disc]]
    depth = np.where(disc, np.float32(0.8), np.float32(0)).astype(np.float32)[None, None]
    ys, xs = np.nonzero(disc)
    return fr, depth, np.asarray([(xs.min(), xs.max(), ys.min(), ys.max())], np.int32), disc


TOY_OBJECT, TOY_BACKGROUND = (96, 255), (0, 159)


def test_reference_segments_a_moved_disc():
    """Learnt on one frame, segmented on the next: the same disc 6 pixels further, over a new background.  Object colours in 96..255
    and background colours in 0..159 per channel (they share 96..159), bits 5, radius 2, margin 16: the reference's mask has IoU
    0.996 with the disc (measured; what is lost is the rim the majority filter rounds off; the bar is the 0.95 the feature is specified
    with).  Measured with the same toy for comparison: disjoint ranges (128..255 over 0..127) 0.996; both uniform in 0..255 0.994 at
    bits 5 and 0.959 at bits 4, where background cells start to fall into the disc's bins"""
    H, W, bits, margin, radius = 120, 160, 5, 16, 2
    fr0, depth0, box0, _ = _toy_frame(H, W, 70, 60, 30, 1, TOY_OBJECT, TOY_BACKGROUND)
    fr1, _, box1, disc1 = _toy_frame(H, W, 76, 60, 30, 2, TOY_OBJECT, TOY_BACKGROUND)
    hist, age, counts = S.seg_learn(fr0, depth0, None, box0, None, 0, bits, margin, 0.1, 64, np.zeros((1, 2, 1 << 15), np.float32),
                                    np.zeros(1, np.int32))
    assert age.tolist() == [1] and counts[0, 0] == depth0.astype(bool).sum() and counts[0, 1] > 64
    mask, cnt, status = S.seg_mask(fr1, box1, hist, age, bits, margin, radius)
    got = S.iou(mask[0, 0] > 0, disc1)
    print("toy IoU at bits 5, radius 2: {:.3f}".format(got))
    assert not status.any() and cnt[0, 1] == mask.sum()
    assert got >= 0.95, got
