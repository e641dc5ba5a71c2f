"""tests/source_size_reference.py (the two-size zoom sampler and network input, the window rule at the source size) pinned to the oracle's
unchanged primitives, its named mutants shown to change an output on the inputs the GPU tests use, and the configuration checks of a
SCALES other than the network size.  No GPU."""
import os

import numpy as np
import pytest

import pixel_kernels_reference as P
import source_size_reference as R

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def same_bits(got, want, what):
    """every float32 equal, none NaN -- the comparison tests/test_pixel_kernels_host.py makes.  (Only the sign of a zero escapes it: the
    oracle multiplies a corner by its validity, the kernels and the restatement select, so an invalid negative corner is -0 there.)"""
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    np.testing.assert_array_equal(got, want, err_msg=what)


def _planes(Hs, Ws):
    inp = R.zoom_inputs(Hs, Ws)
    return inp, np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1)


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS + ((R.SAME_SIZE, R.SAME_SIZE),))
def test_sampler_equals_the_oracle_primitives(src, net):
    """zoom_sample_src == oracle.zoom.bilinear_sampler(x, oracle.zoom._grid_from_factor(zf, Hn, Wn)), bit for bit"""
    from oracle import zoom as oz

    (Hs, Ws), (Hn, Wn) = src, net
    inp, x4 = _planes(Hs, Ws)
    with np.errstate(over="ignore", invalid="ignore"):
        grid = oz._grid_from_factor(R.ZOOM_FACTORS, Hn, Wn)
        for name, x in (("planes", x4), ("image", inp["io"])):
            want = oz.bilinear_sampler(x, grid)
            assert want.shape == x.shape[:2] + (Hn, Wn) and np.all(np.isfinite(want))
            same_bits(R.zoom_sample_src(x, R.ZOOM_FACTORS, Hn, Wn), want, "{} {}->{}".format(name, src, net))
        pm = R.ZOOM_MEANS.reshape(1, 3, 1, 1)
        want = (oz.bilinear_sampler((inp["io"] + pm).astype(f32), grid) - pm).astype(f32)
        same_bits(R.zoom_sample_src(inp["io"], R.ZOOM_FACTORS, Hn, Wn, add=R.ZOOM_MEANS), want, "image with means {}->{}".format(src, net))
        binarised = np.where(inp["depth_like"] > f32(0.2), f32(1), f32(0)).astype(f32)
        same_bits(R.zoom_sample_src(inp["depth_like"], R.ZOOM_FACTORS, Hn, Wn, pre=1), oz.bilinear_sampler(binarised, grid), "bin02")


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS)
def test_net_input_equals_the_oracle(src, net):
    """net_input_src mode 0 == oracle.flownet.network_input of the oracle's zoomed tensors, bit for bit, lanes 0-5 (the mask lanes
    through oracle.zoom.mx_round)"""
    from oracle import flownet as of
    from oracle import zoom as oz

    (Hs, Ws), (Hn, Wn) = src, net
    inp = R.zoom_inputs(Hs, Ws)
    zf = R.ZOOM_FACTORS
    with np.errstate(over="ignore", invalid="ignore"):
        grid = oz._grid_from_factor(zf, Hn, Wn)
        pm = R.ZOOM_MEANS.reshape(1, 3, 1, 1)
        zio = (oz.bilinear_sampler((inp["io"] + pm).astype(f32), grid) - pm).astype(f32)
        zir = (oz.bilinear_sampler((inp["ir"] + pm).astype(f32), grid) - pm).astype(f32)
        zmo = oz.mx_round(oz.bilinear_sampler(inp["binary"], grid)).astype(f32)
        binarised = np.where(inp["depth_like"] > f32(0.2), f32(1), f32(0)).astype(f32)
        zmr = oz.mx_round(oz.bilinear_sampler(binarised, grid)).astype(f32)
        want = np.asarray(of.network_input(zio, zir, zmo, zmr), f32)      # (B,8,Hn,Wn)
        got = R.net_input_src(inp["io"], inp["ir"], inp["binary"], inp["depth_like"], zf, R.ZOOM_MEANS, 0, Hn, Wn)
    same_bits(np.ascontiguousarray(got["X"].transpose(0, 3, 1, 2)), np.ascontiguousarray(want), "network input {}->{}".format(src, net))


def test_equal_sizes_equal_the_same_size_restatement():
    H, W = R.SAME_SIZE
    inp, x4 = _planes(H, W)
    zf, means = R.ZOOM_FACTORS, R.ZOOM_MEANS
    with np.errstate(over="ignore", invalid="ignore"):
        for pre in (0, 1):
            same_bits(R.zoom_sample_src(x4, zf, H, W, pre=pre), P.zoom_sample(x4, zf, pre=pre), "planes pre={}".format(pre))
        same_bits(R.zoom_sample_src(inp["io"], zf, H, W, add=means), P.zoom_sample(inp["io"], zf, means), "image")
        for mode in (0, 1, 2, 3):
            eo, er = (None, None) if mode == 1 else (inp["binary"], inp["depth_like"])
            got = R.net_input_src(inp["io"], inp["ir"], eo, er, zf, means, mode, H, W)
            want = P.net_input(inp["io"], inp["ir"], eo, er, zf, means, mode)
            same_bits(got["X"], want["X"], "net_input mode {}".format(mode))
            if mode == 0:
                for g, w in zip(got["nchw"], want["nchw"]):
                    same_bits(g, w, "nchw")


@pytest.mark.parametrize("mutant", R.MUTANTS["sample"])
def test_every_sampler_mutant_changes_an_output(mutant):
    """on the size pairs and factors of the GPU test; per pair at least one lane of the network input differs, except where the mutant
    is the identity by construction (equal ratios leave `sizes_swapped` no room only when Hs == Ws, which no pair has)"""
    caught = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for (Hs, Ws), (Hn, Wn) in R.SIZE_PAIRS:
            inp = R.zoom_inputs(Hs, Ws)
            args = (inp["io"], inp["ir"], inp["binary"], inp["depth_like"], R.ZOOM_FACTORS, R.ZOOM_MEANS, 0, Hn, Wn)
            good, bad = R.net_input_src(*args), R.net_input_src(*args, mutant=mutant)
            n = int((good["X"] != bad["X"]).sum())
            print("{} {}x{}->{}x{}: {} of {} lanes differ".format(mutant, Hs, Ws, Hn, Wn, n, good["X"].size))
            assert n > 0, (mutant, (Hs, Ws), (Hn, Wn))
            caught += 1
    assert caught == len(R.SIZE_PAIRS)


def test_window_rule_at_the_source_size():
    """window == oracle.zoom.zoom_factor_from_valid(..., H=Hs, W=Ws) on masks with those boxes; the mutant (tx, ty from the network
    size) changes it; and for a source that is a 2x copy of a frame the window is the one of that frame with K / 2 (up to the boxes'
    quantisation: here the boxes are exact doubles, so up to float32 rounding)"""
    from oracle import zoom as oz

    Hs, Ws, Hn, Wn = 540, 720, 480, 640
    bo, br, pose, K = R.window_case(Hs, Ws)

    def mask(box):
        m = np.zeros((len(box), Hs, Ws), bool)
        for b, (x0, x1, y0, y1) in enumerate(box):
            m[b, y0:y1 + 1, x0:x1 + 1] = True
        return m
    want, empty = oz.zoom_factor_from_valid(mask(bo), mask(br), pose, K, Hs, Ws)
    assert not empty.any()
    got = R.window(bo, br, pose, K, Hs, Ws)
    same_bits(got, want, "window")
    bad = R.window(bo, br, pose, K, Hs, Ws, Hn, Wn, mutant="window_network")
    assert (bits(bad[:, 2:]) != bits(got[:, 2:])).all() and (bits(bad[:, :2]) == bits(got[:, :2])).all()
    # the same-size case is the existing restatement (an empty box aside)
    zf, status = P.zoom_factor(bo, br, pose, K, Hs, Ws)
    assert not status.any()
    same_bits(got, zf, "window vs pixel_kernels_reference.zoom_factor")


# ------------------------------------------------------------------------------------------------ configuration
@pytest.fixture()
def cfg():
    from deepim.config.config import config, reset_config

    reset_config()
    yield config
    reset_config()


def test_source_size_of_scales(cfg):
    from deepim.symbols.deepIM_flownet import source_size

    assert source_size(cfg) == (480, 640)
    for ok in ((540, 720), (960, 1280), (240, 320), (3, 4)):
        cfg.SCALES = [ok]
        assert source_size(cfg) == ok
    for bad in ((480, 720), (640, 480), (500, 500), (0, 0)):
        cfg.SCALES = [bad]
        with pytest.raises(ValueError, match="SCALES.*4:3"):
            source_size(cfg)
    cfg.SCALES = [(480, 640), (540, 720)]
    with pytest.raises(ValueError, match="SCALES.*one"):
        source_size(cfg)


def test_loaders_and_scales(cfg):
    """the test loader's check takes a 4:3 SCALES that names the files' size and nothing else; the train loader's still raises for a
    size other than the network's, and says that training there is out of scope"""
    from deepim.core import loader as L

    cfg.SCALES = [(540, 720)]
    L._check_common(cfg, 540, 720, test=True)
    with pytest.raises(ValueError, match="SCALES"):
        L._check_common(cfg, 480, 640, test=True)           # files of another size: there is no resize
    with pytest.raises(NotImplementedError, match="SCALES.*training.*out of scope"):
        L._check_common(cfg, 480, 640)
    with pytest.raises(NotImplementedError, match="SCALES.*training.*out of scope"):
        L.TrainDataLoader(None, [], cfg, batch_size=1, device="cpu")
    cfg.SCALES = [(540, 700)]
    with pytest.raises(ValueError, match="SCALES.*4:3"):
        L._check_common(cfg, 540, 700, test=True)


def test_stages_built_for_the_network_size_are_refused(cfg):
    """every stage that is not built at another source size raises a ValueError naming its key and SCALES; at the network size, and
    with all of them off, nothing is refused"""
    from deepim.core.tester import refuse_at_source_size

    cfg.TEST.FAST_TEST = True
    refuse_at_source_size(cfg, (540, 720))
    T = cfg.TEST
    for key, value, match in (("ICP_ITER", 2, "TEST.ICP_ITER"), ("HYP_NUM", 3, "TEST.HYP_NUM"), ("COARSE_VIEWS", 8, "TEST.COARSE_VIEWS"),
                              ("VSD", True, "TEST.VSD"), ("BOP_VSD", True, "TEST.BOP_VSD"), ("FLOW_PNP_ITER", 2, "TEST.FLOW_PNP_ITER")):
        old = T.get(key)
        T[key] = value
        refuse_at_source_size(cfg, (480, 640))
        with pytest.raises(ValueError, match=match + ".*SCALES"):
            refuse_at_source_size(cfg, (540, 720))
        T[key] = old
    with pytest.raises(ValueError, match="lit ModelNet renderer.*SCALES"):
        refuse_at_source_size(cfg, (540, 720), lit=True)
    cfg.network.PRED_FLOW, cfg.TEST.FAST_TEST = True, False
    with pytest.raises(ValueError, match="PRED_FLOW.*FAST_TEST.*SCALES"):
        refuse_at_source_size(cfg, (540, 720))
    refuse_at_source_size(cfg, (480, 640))


def test_the_960x1280_config_loads(cfg):
    from deepim.config.config import update_config
    from deepim.symbols.deepIM_flownet import source_size

    update_config(os.path.join(CFGS, "deepim_hip_LM_ape_test_960x1280.yaml"))
    assert source_size(cfg) == (960, 1280)
    K2 = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float64).reshape(3, 3)
    reset = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 0.5]])
    np.testing.assert_allclose(K2, 2 * reset, rtol=1e-7)
    # everything else is the shipped ape test config
    import yaml

    a = yaml.safe_load(open(os.path.join(CFGS, "deepim_hip_LM_ape_test.yaml")))
    b = yaml.safe_load(open(os.path.join(CFGS, "deepim_hip_LM_ape_test_960x1280.yaml")))
    a["SCALES"], b["SCALES"] = None, None
    a["dataset"]["INTRINSIC_MATRIX"] = b["dataset"]["INTRINSIC_MATRIX"] = None
    assert a == b


def test_the_library_exports_the_source_size_entry_points(hip_lib):
    from lib.hip import capi

    for name in ("dim_zoom_net_input_src", "dim_zoom_planes_src", "dim_refiner_create_src"):
        assert name in capi.SIGNATURES, name
        assert getattr(hip_lib, name) is not None
