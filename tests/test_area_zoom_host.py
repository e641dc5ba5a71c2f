"""tests/area_zoom_reference.py (the area-filtered zoom sampler, its network input and its tap rule) pinned to the oracle's unchanged
BilinearSampler on shifted grids, shown equal to tests/source_size_reference.py where one sample is taken, its named mutants shown to
change an output on the inputs the GPU tests use, the tap rule at its boundaries, what the filter does to a pattern finer than a
network pixel, and the configuration keys TEST.ZOOM_FILTER / TEST.ZOOM_AREA_MAX_TAPS.  No GPU."""
import os

import numpy as np
import pytest

import area_zoom_reference as R
import source_size_reference as S

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs")
MINIFYING = tuple(p for p in R.SIZE_PAIRS if p != ((6, 8), (12, 16)))     # (6,8)->(12,16) magnifies: taps (1,1) but for the 1e30 row


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def same_bits(got, want, what):
    """every float32 equal, none NaN (only the sign of a zero escapes: the oracle multiplies a corner by its validity, the kernels and
    the restatement select)"""
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    np.testing.assert_array_equal(got, want, err_msg=what)


def _planes(Hs, Ws):
    inp = R.zoom_inputs(Hs, Ws)
    return inp, np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1)


def oracle_mean(x, zf, Hn, Wn, n_xy):
    """the mean of oracle.zoom.bilinear_sampler over the grids shifted by the sub-sample offsets, summed ky outer / kx inner"""
    from oracle import zoom as oz

    out = np.empty(x.shape[:2] + (Hn, Wn), f32)
    sx, sy = f32(2.0 / (Wn - 1)), f32(2.0 / (Hn - 1))
    for b in range(x.shape[0]):
        wx, wy, tx, ty = zf[b]
        nx, ny = int(n_xy[b, 0]), int(n_xy[b, 1])
        acc = None
        for oy in R.offsets(ny):
            for ox in R.offsets(nx):
                xt = f32(-1) + (np.arange(Wn, dtype=f32) + ox) * sx
                yt = f32(-1) + (np.arange(Hn, dtype=f32) + oy) * sy
                grid = np.empty((1, 2, Hn, Wn), f32)
                grid[0, 0] = np.broadcast_to((wx * xt + tx)[None, :], (Hn, Wn))
                grid[0, 1] = np.broadcast_to((wy * yt + ty)[:, None], (Hn, Wn))
                r = oz.bilinear_sampler(x[b:b + 1], grid)[0]
                acc = r if acc is None else acc + r
        out[b] = acc / f32(nx * ny)
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS)
def test_sampler_equals_the_mean_of_the_oracle_sampler_on_shifted_grids(src, net):
    from oracle import zoom as oz

    (Hs, Ws), (Hn, Wn) = src, net
    inp, x4 = _planes(Hs, Ws)
    zf = R.ZOOM_FACTORS
    n_xy = R.taps(zf, Hs, Ws, Hn, Wn)
    with np.errstate(over="ignore", invalid="ignore"):
        # with every offset 0 the hand-built grid is the oracle's own GridGenerator
        one = np.ones_like(n_xy)
        same_bits(oracle_mean(x4, zf, Hn, Wn, one), oz.bilinear_sampler(x4, oz._grid_from_factor(zf, Hn, Wn)), "grid {}->{}".format(src, net))
        for name, x in (("planes", x4), ("image", inp["io"])):
            want = oracle_mean(x, zf, Hn, Wn, n_xy)
            assert np.all(np.isfinite(want))
            same_bits(R.zoom_sample_area(x, zf, Hn, Wn), want, "{} {}->{}".format(name, src, net))
        pm = R.ZOOM_MEANS.reshape(1, 3, 1, 1)
        want = (oracle_mean((inp["io"] + pm).astype(f32), zf, Hn, Wn, n_xy) - pm).astype(f32)
        same_bits(R.zoom_sample_area(inp["io"], zf, Hn, Wn, add=R.ZOOM_MEANS), want, "image with means {}->{}".format(src, net))
        binarised = np.where(inp["depth_like"] > f32(0.2), f32(1), f32(0)).astype(f32)
        same_bits(R.zoom_sample_area(inp["depth_like"], zf, Hn, Wn, pre=1), oracle_mean(binarised, zf, Hn, Wn, n_xy), "bin02")


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS)
def test_one_tap_is_the_bilinear_restatement(src, net):
    """with taps (1,1) -- max_taps = 1, or counts forced to 1 -- every bit is tests/source_size_reference.py's"""
    (Hs, Ws), (Hn, Wn) = src, net
    inp, x4 = _planes(Hs, Ws)
    zf, means = R.ZOOM_FACTORS, R.ZOOM_MEANS
    ones = np.ones((R.ZOOM_B, 2), np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        assert (R.taps(zf, Hs, Ws, Hn, Wn, max_taps=1) == 1).all()
        for pre in (0, 1):
            want = S.zoom_sample_src(x4, zf, Hn, Wn, pre=pre)
            np.testing.assert_array_equal(bits(R.zoom_sample_area(x4, zf, Hn, Wn, max_taps=1, pre=pre)), bits(want))
            np.testing.assert_array_equal(bits(R.zoom_sample_area(x4, zf, Hn, Wn, pre=pre, n_xy=ones)), bits(want))
        np.testing.assert_array_equal(bits(R.zoom_sample_area(inp["io"], zf, Hn, Wn, max_taps=1, add=means)),
                                      bits(S.zoom_sample_src(inp["io"], zf, Hn, Wn, add=means)))
        for mode in (0, 1, 2, 3):
            eo, er = (None, None) if mode == 1 else (inp["binary"], inp["depth_like"])
            got = R.net_input_area(inp["io"], inp["ir"], eo, er, zf, means, mode, Hn, Wn, max_taps=1)
            want = S.net_input_src(inp["io"], inp["ir"], eo, er, zf, means, mode, Hn, Wn)
            np.testing.assert_array_equal(bits(got["X"]), bits(want["X"]), err_msg="mode {}".format(mode))
        # and with max_taps = 4 the pairs whose counts are (1,1) keep those bits, the others do not
        n_xy = R.taps(zf, Hs, Ws, Hn, Wn)
        got, want = R.zoom_sample_area(x4, zf, Hn, Wn), S.zoom_sample_src(x4, zf, Hn, Wn)
        for b in range(R.ZOOM_B):
            if tuple(n_xy[b]) == (1, 1):
                np.testing.assert_array_equal(bits(got[b]), bits(want[b]), err_msg="pair {}".format(b))
            elif np.any(want[b] != 0):        # (the 1e30 window reads nothing with any count)
                assert (bits(got[b]) != bits(want[b])).any(), b


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_an_output(mutant):
    """on the size pairs and factors of the GPU test: the network input of every pair that shrinks the source differs"""
    with np.errstate(over="ignore", invalid="ignore"):
        for (Hs, Ws), (Hn, Wn) in MINIFYING:
            inp = R.zoom_inputs(Hs, Ws)
            args = (inp["io"], inp["ir"], inp["binary"], inp["depth_like"], R.ZOOM_FACTORS, R.ZOOM_MEANS, 0, Hn, Wn)
            good, bad = R.net_input_area(*args), R.net_input_area(*args, mutant=mutant)
            n = int((good["X"] != bad["X"]).sum())
            print("{} {}x{}->{}x{}: {} of {} lanes differ".format(mutant, Hs, Ws, Hn, Wn, n, good["X"].size))
            assert n > 0, (mutant, (Hs, Ws), (Hn, Wn))


def test_tap_rule_at_the_boundaries():
    """step + 0.5 exactly an integer in float32 and one ulp to either side; NaN -> 1; inf / 1e30 -> max_taps; negative w"""
    zf, want = R.boundary_cases()
    (Hs, Ws), (Hn, Wn) = R.BOUNDARY_SIZES
    assert R.ratio(Ws, Wn) == f32(2) and R.ratio(Hs, Hn) == f32(2)
    st = R.steps(zf, Hs, Ws, Hn, Wn)
    for row, centre in ((1, 1.5), (4, 2.5)):
        assert st[row, 0] == f32(centre) and st[row, 0] + f32(0.5) == f32(centre + 0.5)          # exactly on the boundary
        assert st[row - 1, 0] == np.nextafter(f32(centre), f32(0)) and st[row + 1, 0] == np.nextafter(f32(centre), f32(9))
        assert st[row - 1, 0] + f32(0.5) < f32(centre + 0.5)
    got = R.taps(zf, Hs, Ws, Hn, Wn, R.BOUNDARY_MAX_TAPS)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and (got[:, 0] == got[:, 1]).all()                              # wy = -wx: the step is |w|
    for max_taps in range(1, 9):
        n = R.taps(zf, Hs, Ws, Hn, Wn, max_taps)
        assert n.min() >= 1 and n.max() == max_taps


def test_offsets_are_centred_and_exactly_zero_for_one_tap():
    assert R.offsets(1).tolist() == [0.0] and np.signbit(R.offsets(1)[0]) == False  # noqa: E712
    for n in range(1, 9):
        o = R.offsets(n)
        assert o.dtype == f32 and len(o) == n
        np.testing.assert_allclose(o, (np.arange(n) + 0.5) / n - 0.5, rtol=0, atol=2 ** -25)
        np.testing.assert_array_equal(o, -o[::-1])
    # one tap: the first sample starts the sum and the division is by 1, so the bits are the bilinear restatement's, signed zeros
    # included (a plane of -0 comes out +0 from both: pre(x) + add is formed first)
    x = np.full((1, 1, 4, 4), -0.0, f32)
    np.testing.assert_array_equal(bits(R.zoom_sample_area(x, R.FULL_FRAME, 4, 4)), bits(S.zoom_sample_src(x, R.FULL_FRAME, 4, 4)))


@pytest.mark.parametrize("src,net", R.STRIPE_PAIRS)
def test_stripes_finer_than_a_network_pixel_come_out_grey(src, net):
    """vertical stripes of period 2 source pixels, full-frame window: the bilinear output swings (moire), the area output stays near
    the 127.5 a camera of the network's resolution would see.  The cap is a condition: at most 1/4 of the bilinear peak-to-peak."""
    (Hs, Ws), (Hn, Wn) = src, net
    x = R.stripe_source(Hs, Ws)
    n = R.taps(R.FULL_FRAME, Hs, Ws, Hn, Wn)
    assert n.min() >= 2
    area, bil = R.zoom_sample_area(x, R.FULL_FRAME, Hn, Wn), S.zoom_sample_src(x, R.FULL_FRAME, Hn, Wn)
    R.check_stripes(area, bil, "{}->{} taps {}".format(src, net, n[0].tolist()))


# ------------------------------------------------------------------------------------------------ configuration
@pytest.fixture()
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    yield config
    reset_config()


def test_defaults_and_bad_values(cfg):
    from deepim.symbols.deepIM_flownet import zoom_filter

    assert cfg.TEST.ZOOM_FILTER == "bilinear" and cfg.TEST.ZOOM_AREA_MAX_TAPS == 4
    cfg.TEST.FAST_TEST = True
    assert zoom_filter(cfg) == ("bilinear", 4)
    cfg.TEST.ZOOM_FILTER = "area"
    assert zoom_filter(cfg) == ("area", 4)
    for taps in (1, 8):
        cfg.TEST.ZOOM_AREA_MAX_TAPS = taps
        assert zoom_filter(cfg) == ("area", taps)
    for bad in (0, 9, -1, 2.5, "4", None, True):
        cfg.TEST.ZOOM_AREA_MAX_TAPS = bad
        with pytest.raises(ValueError, match="TEST.ZOOM_AREA_MAX_TAPS"):
            zoom_filter(cfg)
    cfg.TEST.ZOOM_AREA_MAX_TAPS = 4
    for bad in ("lanczos", "", None, "AREA"):
        cfg.TEST.ZOOM_FILTER = bad
        with pytest.raises(ValueError, match="TEST.ZOOM_FILTER"):
            zoom_filter(cfg)


def test_the_full_graph_and_training_refuse_the_area_filter(cfg):
    from deepim.core import loader as L
    from deepim.symbols.deepIM_flownet import zoom_filter

    cfg.TEST.ZOOM_FILTER = "area"
    cfg.TEST.FAST_TEST = False
    with pytest.raises(ValueError, match="TEST.ZOOM_FILTER 'area'.*FAST_TEST"):
        zoom_filter(cfg)
    cfg.network.PRED_FLOW = True
    with pytest.raises(ValueError, match="TEST.ZOOM_FILTER 'area'.*FAST_TEST"):
        zoom_filter(cfg)
    cfg.TEST.FAST_TEST = True
    assert zoom_filter(cfg) == ("area", 4)        # the shipped test configs: PRED_FLOW on, the heads not run
    with pytest.raises(ValueError, match="TEST.ZOOM_FILTER 'area'.*training"):
        L.TrainDataLoader(None, [], cfg, batch_size=1, device="cpu")
    with pytest.raises(ValueError, match="TEST.ZOOM_FILTER 'area'.*training"):
        L.refuse_zoom_filter_in_training(cfg)
    cfg.TEST.ZOOM_FILTER = "bilinear"
    L.refuse_zoom_filter_in_training(cfg)
    cfg.TEST.FAST_TEST = False
    assert zoom_filter(cfg) == ("bilinear", 4)


def test_the_960x1280_area_config_loads(cfg):
    import yaml

    from deepim.config.config import update_config
    from deepim.symbols.deepIM_flownet import source_size, zoom_filter

    update_config(os.path.join(CFGS, "deepim_hip_LM_ape_test_960x1280_area.yaml"))
    assert source_size(cfg) == (960, 1280) and zoom_filter(cfg) == ("area", 4)
    # everything else is the 960x1280 config
    a = yaml.safe_load(open(os.path.join(CFGS, "deepim_hip_LM_ape_test_960x1280.yaml")))
    b = yaml.safe_load(open(os.path.join(CFGS, "deepim_hip_LM_ape_test_960x1280_area.yaml")))
    assert b["TEST"].pop("ZOOM_FILTER") == "area" and b["TEST"].pop("ZOOM_AREA_MAX_TAPS") == 4
    assert a == b


def test_the_library_exports_the_area_entry_points(hip_lib):
    from lib.hip import capi

    for name in ("dim_zoom_planes_area", "dim_zoom_net_input_area", "dim_zoom_area_taps", "dim_refiner_set_zoom_filter"):
        assert name in capi.SIGNATURES, name
        assert getattr(hip_lib, name) is not None
