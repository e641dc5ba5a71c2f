"""CPU: the rules of dim_vis_overlay as tests/vis_reference.py restates them, on hand-written scenes with the expected bytes written
out; and the host side of TEST.VISUALIZE that needs no GPU: the settings, the file names, the order of a video's frames, the refusals."""
import numpy as np
import pytest

import vis_reference as vr

MEANS = np.array([103.939, 116.779, 123.68], dtype=np.float32)   # B, G, R
GREEN, RED, GREY = (0, 255, 0), (0, 0, 255), (191, 191, 191)


def _grey(B, H, W, level=100.0):
    """an image_observed blob whose base colour is `level` in every channel (level + mean - mean is exact for these numbers' rint)"""
    img = np.empty((B, 3, H, W), dtype=np.float32)
    for c in range(3):
        img[:, c] = np.float32(level) - MEANS[2 - c]
    return img


def _rows(*rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def _layer(mask):
    return np.asarray(mask, dtype=np.float32)[None, None]   # (L=1, B=1, H, W)


def _painted(out, colour, base=100):
    """-> bool map of the pixels that hold `colour`; every other pixel must hold the base colour"""
    hit = (out == np.asarray(colour, dtype=np.uint8)).all(-1)
    assert ((out == base).all(-1) | hit).all()
    return hit


BLOCK = _rows(".......",
              ".......",
              "..###..",
              "..###..",
              "..###..",
              ".......",
              ".......")


def test_block_radius_0_is_its_ring():
    out, counts = vr.overlay(_grey(1, 7, 7), MEANS, _layer(BLOCK), [GREEN + (256, 0)], 0)
    assert np.array_equal(_painted(out[0], GREEN), _rows(".......",
                                                         ".......",
                                                         "..###..",
                                                         "..#.#..",
                                                         "..###..",
                                                         ".......",
                                                         "......."))
    assert counts.tolist() == [[[8, 9]]]
    assert out[0, 3, 3].tolist() == [100, 100, 100] and out[0, 2, 2].tolist() == [0, 255, 0] and out.dtype == np.uint8


def test_block_radius_1_is_the_ring_grown_by_one():
    out, counts = vr.overlay(_grey(1, 7, 7), MEANS, _layer(BLOCK), [GREEN + (256, 0)], 1)
    assert np.array_equal(_painted(out[0], GREEN), _rows(".......",
                                                         ".#####.",
                                                         ".#####.",
                                                         ".#####.",
                                                         ".#####.",
                                                         ".#####.",
                                                         "......."))
    assert counts.tolist() == [[[25, 9]]]


def test_single_pixel_and_depth_values_and_nan():
    lay = np.zeros((1, 1, 5, 5), dtype=np.float32)
    lay[0, 0, 2, 2] = 0.73        # a depth, not a 0/1 mask
    lay[0, 0, 0, 0] = np.nan      # not inside
    lay[0, 0, 4, 4] = -1.0        # not inside
    out, counts = vr.overlay(_grey(1, 5, 5), MEANS, lay, [RED + (256, 0)], 0)
    assert np.array_equal(_painted(out[0], RED), _rows(".....", ".....", "..#..", ".....", "....."))
    assert counts.tolist() == [[[1, 1]]]
    out, counts = vr.overlay(_grey(1, 5, 5), MEANS, lay, [RED + (256, 0)], 3)   # the square is clipped to the frame
    assert _painted(out[0], RED).all() and counts.tolist() == [[[25, 1]]]


def test_block_cut_by_the_frame_has_no_outline_along_the_border():
    corner = _rows("###....",
                   "###....",
                   "###....",
                   ".......",
                   ".......",
                   ".......",
                   ".......")
    out, counts = vr.overlay(_grey(1, 7, 7), MEANS, _layer(corner), [GREEN + (256, 0)], 0)
    assert np.array_equal(_painted(out[0], GREEN), _rows("..#....",
                                                         "..#....",
                                                         "###....",
                                                         ".......",
                                                         ".......",
                                                         ".......",
                                                         "......."))
    assert counts.tolist() == [[[5, 9]]]
    full = np.ones((7, 7), dtype=bool)   # the object covers the frame: no edge at all
    out, counts = vr.overlay(_grey(1, 7, 7), MEANS, _layer(full), [GREEN + (256, 0)], 3)
    assert (out == 100).all() and counts.tolist() == [[[0, 49]]]


def test_one_by_one_frame_has_no_edge():
    out, counts = vr.overlay(_grey(1, 1, 1), MEANS, _layer([[1.0]]), [GREEN + (256, 64)], 2)
    assert counts.tolist() == [[[0, 1]]]
    # inside, not marked, fill alpha 64: (100 * 192 + colour * 64 + 128) >> 8
    assert out.tolist() == [[[[75, 139, 75]]]]


def test_two_layers_later_wins_and_fill_sits_under_a_later_edge():
    a = _rows("......", ".###..", ".###..", ".###..", "......", "......")
    b = _rows("......", "......", "..###.", "..###.", "..###.", "......")
    layers = np.stack([a, b]).astype(np.float32)[:, None]
    blue = (200, 0, 0)
    out, counts = vr.overlay(_grey(1, 6, 6), MEANS, layers, [blue + (256, 128), GREEN + (128, 0)], 0)
    o = out[0]
    assert counts.tolist() == [[[8, 9], [8, 9]]]
    assert o[1, 1].tolist() == [200, 0, 0]                 # the first layer's edge alone
    # (2,2): the first layer's interior (fill, alpha 128: 100 -> 150, 50, 50), then the second layer's edge over it at alpha 128:
    # B (150 * 128 + 128) >> 8 = 75, G (50 * 128 + 255 * 128 + 128) >> 8 = 153, R (50 * 128 + 128) >> 8 = 25
    assert o[2, 2].tolist() == [75, 153, 25]
    # (2,3): both mark.  The first paints 200, 0, 0; the second blends over THAT: B 100, G (255 * 128 + 128) >> 8 = 128, R 0
    assert o[2, 3].tolist() == [100, 128, 0]
    assert o[3, 3].tolist() == [200, 0, 0]                 # the first layer's edge; inside the second, not marked, no fill: unchanged
    assert o[4, 4].tolist() == [50, 178, 50]               # the second layer's edge over the base: (100 * 128 + c * 128 + 128) >> 8
    out1, _ = vr.overlay(_grey(1, 6, 6), MEANS, layers, [blue + (256, 128), GREEN + (256, 0)], 0)
    assert out1[0, 2, 3].tolist() == [0, 255, 0] and out1[0, 2, 2].tolist() == [0, 255, 0]   # at alpha 256 the later one wins outright


def test_blend_ends_and_rounding_halves():
    c, colour = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(vr.blend(c, colour, 0), c) and np.array_equal(vr.blend(c, colour, 256), colour)
    # alpha 128 is the mean with the half rounded up
    assert [int(vr.blend(1, 0, 128)), int(vr.blend(0, 1, 128)), int(vr.blend(3, 0, 128)), int(vr.blend(255, 254, 128))] == [1, 1, 2, 255]
    assert int(vr.blend(10, 20, 128)) == 15 and int(vr.blend(100, 200, 64)) == 125
    lay = _layer([[1.0, 0.0]])   # a 1 x 2 frame: pixel 0 is an edge
    out, _ = vr.overlay(_grey(1, 1, 2, level=1.0), MEANS, lay, [(0, 1, 2) + (128, 0)], 0)
    assert out.tolist() == [[[[1, 1, 2], [1, 1, 1]]]]


def test_base_colour_clamps_rounds_half_to_even_and_zeroes_nan():
    img = np.zeros((1, 3, 1, 6), dtype=np.float32)
    want = [-5.0, 300.0, np.nan, 100.5, 101.5, 255.4]
    for c in range(3):
        img[0, c, 0] = np.asarray(want, dtype=np.float32)
    out = vr.base_colour(img, np.zeros(3, dtype=np.float32))
    assert out[0, 0].tolist() == [[0] * 3, [255] * 3, [0] * 3, [100] * 3, [102] * 3, [255] * 3]
    # plane c holds BGR channel 2 - c, and the means are given in B, G, R order
    img = np.zeros((1, 3, 1, 1), dtype=np.float32)
    img[0, :, 0, 0] = [10.0, 20.0, 30.0]   # planes R, G, B
    assert vr.base_colour(img, [1.0, 2.0, 3.0])[0, 0, 0].tolist() == [31, 22, 13]
    img[0, 0, 0, 0] = np.inf
    assert vr.base_colour(img, [1.0, 2.0, 3.0])[0, 0, 0].tolist() == [31, 22, 255]


# ---- the host side of TEST.VISUALIZE

@pytest.fixture()
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    yield config
    reset_config()


def test_settings_defaults(cfg):
    from deepim.core.visualize import vis_dir, vis_settings

    assert tuple(vis_settings(cfg)) == ("", 64, 1, 256, 0, True, False, False)
    assert cfg.TEST.VISUALIZE is False
    cfg.output_path = "/some/where"
    assert vis_dir(cfg).replace("\\", "/") == "/some/where/vis"
    cfg.TEST.VIS_DIR = "pictures"
    assert vis_dir(cfg) == "pictures"


@pytest.mark.parametrize("key,bad", [("VIS_DIR", 3), ("VIS_MAX_PAIRS", -1), ("VIS_MAX_PAIRS", 1.5), ("VIS_RADIUS", 4), ("VIS_RADIUS", -1),
                                     ("VIS_RADIUS", True), ("VIS_EDGE_ALPHA", 257), ("VIS_EDGE_ALPHA", -1), ("VIS_FILL_ALPHA", 300),
                                     ("VIS_FILL_ALPHA", 0.5), ("VIS_ZOOM", 1), ("VIS_VIDEO", "yes"), ("VIS_VIDEO_ZOOM", 0)])
def test_settings_name_the_bad_key(cfg, key, bad):
    from deepim.core.visualize import vis_settings

    cfg.TEST[key] = bad
    with pytest.raises(ValueError, match="TEST." + key):
        vis_settings(cfg)


def test_settings_accept_the_ends(cfg):
    from deepim.core.visualize import vis_settings

    cfg.TEST.update(VIS_MAX_PAIRS=0, VIS_RADIUS=3, VIS_EDGE_ALPHA=0, VIS_FILL_ALPHA=256, VIS_ZOOM=False, VIS_VIDEO=True)
    assert tuple(vis_settings(cfg))[1:] == (0, 3, 0, 256, False, True, False)
    cfg.TEST.update(VISUALIZE=True, VIS_VIDEO_ZOOM=True)
    with pytest.raises(ValueError, match="VIS_VIDEO_ZOOM.*VIS_ZOOM"):
        vis_settings(cfg)


def test_hypotheses_and_coarse_are_refused_with_visualize(cfg):
    from deepim.core.visualize import vis_settings

    cfg.TEST.HYP_NUM = 4
    vis_settings(cfg)   # VISUALIZE off: nothing to refuse
    cfg.TEST.VISUALIZE = True
    with pytest.raises(ValueError, match="TEST.VISUALIZE.*TEST.HYP_NUM"):
        vis_settings(cfg)
    cfg.TEST.HYP_NUM = 1
    cfg.TEST.COARSE_VIEWS = 12
    with pytest.raises(ValueError, match="TEST.VISUALIZE.*TEST.COARSE_VIEWS"):
        vis_settings(cfg)
    cfg.TEST.COARSE_VIEWS = 0
    vis_settings(cfg)


def test_file_names():
    from deepim.core import visualize as v

    assert v.pair_dir_name(7, "ape") == "pair_000007_ape"
    assert v.frame_names(2, ()) == ["iter_00", "iter_01", "iter_02"]
    assert v.frame_names(1, ("sil", "icp")) == ["iter_00", "iter_01", "icp", "sil"]   # in the order the stages run
    assert v.frame_file("iter_03") == "iter_03.png" and v.frame_file("iter_03", zoom=True) == "iter_03_zoom.png"
    assert v.frame_file("icp", zoom=True) == "icp_zoom.png"


def test_gif_frame_order_holds_the_ends_five_times():
    from deepim.core import visualize as v

    names = ["iter_00", "iter_01", "iter_02", "icp"]
    assert v.gif_frame_order(names) == ["iter_00"] * 5 + ["iter_01", "iter_02"] + ["icp"] * 5
    zoom_in = [v.zoom_in_name(s) for s in (1, 2, 3)]
    assert zoom_in == ["zoom_in_1", "zoom_in_2", "zoom_in_3"]
    assert v.gif_frame_order(names, zoom_in) == zoom_in + ["iter_00"] * 5 + ["iter_01", "iter_02"] + ["icp"] * 5
    assert v.gif_frame_order(["iter_00", "iter_01"]) == ["iter_00"] * 5 + ["iter_01"] * 5
    assert v.gif_frame_order(["iter_00"]) == ["iter_00"] * 5


def test_zoom_in_windows_follow_the_tool():
    from deepim.core.visualize import zoom_in_factors

    z = zoom_in_factors([[0.4, 0.5, 0.3, -0.6]])
    assert z.shape == (3, 1, 4) and z.dtype == np.float32
    # delta = (1 - wx) / 3 on BOTH sides, the centre in thirds; the last window has the pair's width and centre
    np.testing.assert_allclose(z[:, 0], [[0.8, 0.8, 0.1, -0.2], [0.6, 0.6, 0.2, -0.4], [0.4, 0.4, 0.3, -0.6]], rtol=1e-6)


def test_layer_styles_follow_the_tool():
    from deepim.core.visualize import VisSettings, layer_styles

    s = VisSettings("", 64, 1, 200, 64, True, False, False)
    assert layer_styles(s, True, 3).tolist() == [[191, 191, 191, 200, 0], [0, 0, 255, 200, 0], [0, 255, 0, 200, 64]]
    assert layer_styles(s, True, 2).tolist() == [[191, 191, 191, 200, 0], [0, 0, 255, 200, 0]]
    assert layer_styles(s, False, 2).tolist() == [[0, 0, 255, 200, 0], [0, 255, 0, 200, 64]]


def test_entry_point_takes_the_vis_flags():
    import os
    from conftest import PKG

    src = open(os.path.join(PKG, "deepim", "test.py")).read()
    assert "NotImplementedError" not in src and "TEST.VISUALIZE = True" in src
