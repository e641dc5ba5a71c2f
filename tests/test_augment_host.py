"""CPU: the host half of the photometric augmentation of observed training images (TRAIN.AUG_OBSERVED): the integer noise generator
of tests/augment_reference.py (statistics, a typed-in table), the blur taps and the draws of lib/utils/augment.py, the config defaults
and the argument errors of dim_augment_observed, which need no device."""
import ctypes
import random

import numpy as np
import pytest

import augment_reference as ref

SEEDS = (0, 1, 12345, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def noise_fields():
    return {s: ref.noise_planes(s, 480, 640) for s in SEEDS}


def _corr(a, b):
    return float(np.corrcoef(a.ravel().astype(np.float64), b.ravel().astype(np.float64))[0, 1])


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_statistics(noise_fields, seed):
    z = noise_fields[seed]
    assert z.dtype == np.float32 and z.shape == (3, 480, 640)
    z64 = z.astype(np.float64)
    assert abs(z64.mean()) < 0.01 and abs(z64.var() - 1.0) < 0.01
    assert np.abs(z).max() <= 3.4642
    assert abs(_corr(z[:, :, 1:], z[:, :, :-1])) < 0.01     # horizontal neighbours
    assert abs(_corr(z[:, 1:], z[:, :-1])) < 0.01           # vertical neighbours
    for a, b in ((0, 1), (1, 2), (0, 2)):                   # channels
        assert abs(_corr(z[a], z[b])) < 0.01


def test_generator_seeds_are_uncorrelated(noise_fields):
    assert abs(_corr(noise_fields[0], noise_fields[1])) < 0.01


# (seed, counter) -> mix(counter), h0, h1, the bits of n; computed once with Python integers and struct-rounded floats, typed in
TABLE = [((0, 0), 0x00000000, 0x00000000, 0x1EFEE872, 0xBFD74132),
         ((0, 1), 0x688990C0, 0x01FCE552, 0x15B131AA, 0xBFB5496F),
         ((1, 0), 0x00000000, 0x688990C0, 0xB9A61764, 0xBEB9E94B),
         ((12345, 307199), 0xBE199537, 0xC60B064B, 0x6A2D1A45, 0xBF97BCB4),
         ((12345, 921599), 0x0E85BF71, 0xF936D884, 0x74468EE3, 0x3FB85F40),
         ((2 ** 32 - 1, 0), 0x00000000, 0x6768824A, 0xDD9EE2B3, 0x3F933DC1),
         ((2 ** 32 - 1, 2 ** 32 - 1), 0x6768824A, 0x35E1E3A1, 0x273AD93B, 0x3E33F19F),
         ((0x9E3779B9, 614477), 0xB6C1BF38, 0x06F483A8, 0xD53BCDD3, 0x3E9E3646)]


def test_generator_table():
    assert int(ref.NOISE_SCALE.view(np.uint32)) == 0x37DDB3D7    # the float32 nearest to 2.6428997e-05
    for (seed, n), m, h0, h1, bits in TABLE:
        cnt = np.array([n], dtype=np.uint32)
        assert int(ref.mix(cnt)[0]) == m
        with np.errstate(over="ignore"):
            g0 = ref.mix(np.uint32(seed) + cnt * np.uint32(0x9E3779B9))
        assert int(g0[0]) == h0 and int(ref.mix(g0 ^ np.uint32(0x85EBCA6B))[0]) == h1
        val = ref.noise(seed, cnt)
        assert val.dtype == np.float32 and int(val.view(np.uint32)[0]) == bits, (seed, n, hex(int(val.view(np.uint32)[0])))
        s = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16)
        assert float(val[0]) == float(np.float32(s - 131070) * np.float32(2.6428997e-05))


# ---------------------------------------------------------------------------------------------------------------------- blur taps
@pytest.mark.parametrize("sigma,r", [(0.5, 2), (1.0, 3), (2.0, 6), (2.33, 7)])
def test_blur_taps(sigma, r):
    from lib.utils.augment import blur_radius, blur_taps

    got_r, taps = blur_taps(sigma)
    assert got_r == r == blur_radius(sigma) and taps.dtype == np.float32 and taps.shape == (15,)
    used = taps[:2 * r + 1]
    assert abs(float(used.astype(np.float64).sum()) - 1.0) < 1e-6
    np.testing.assert_array_equal(used, used[::-1])
    assert np.all(taps[2 * r + 1:] == 0) and np.all(used > 0) and used.argmax() == r
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma))
    np.testing.assert_array_equal(used, (g / g.sum()).astype(np.float32))


def test_blur_taps_of_no_blur():
    from lib.utils.augment import blur_taps

    r, taps = blur_taps(0.0)
    assert r == 0 and taps[0] == 1 and not taps[1:].any()


# ---------------------------------------------------------------------------------------------------------------------- the draws
def _config(**train):
    from deepim.config.config import config, reset_config

    reset_config()
    config.TRAIN.AUG_OBSERVED = True
    for k, v in train.items():
        config.TRAIN[k] = v
    return config


def _same(p, q):
    return all(np.array_equal(getattr(p, k), getattr(q, k)) for k in ("on", "radius", "taps", "chain", "seed"))


def test_draws_are_a_function_of_seed_epoch_and_key():
    from deepim.config.config import reset_config
    from lib.utils.augment import ObservedAugmenter

    aug = ObservedAugmenter(_config(AUG_PROB=1.0, AUG_BLUR_PROB=1.0))
    keys = [0, 1, 7, 2 ** 40 + 3]
    p = aug.draw(keys, 0)
    assert len(p) == 4 and p.on.tolist() == [1, 1, 1, 1]
    assert p.on.dtype == np.int32 and p.radius.dtype == np.int32 and p.taps.dtype == np.float32 and p.chain.dtype == np.float32
    assert p.seed.dtype == np.uint32 and p.taps.shape == (4, 15) and p.chain.shape == (4, 7)
    assert _same(p, aug.draw(keys, 0)) and _same(p, ObservedAugmenter(_config(AUG_PROB=1.0, AUG_BLUR_PROB=1.0)).draw(keys, 0))
    # a pair's draw depends on its own key alone, not on its slot or its neighbours
    q = aug.draw([7, 0], 0)
    assert np.array_equal(q.chain[0], p.chain[2]) and np.array_equal(q.chain[1], p.chain[0]) and q.seed[0] == p.seed[2]
    # another epoch, key or seed: other parameters
    for other in (aug.draw(keys, 1), aug.draw([k + 100 for k in keys], 0), ObservedAugmenter(_config(AUG_PROB=1.0, AUG_SEED=5)).draw(keys, 0)):
        for j in range(4):
            assert not np.array_equal(other.chain[j], p.chain[j]) and other.seed[j] != p.seed[j]
    assert len({int(s) for s in p.seed}) == 4 and len({tuple(c) for c in p.chain.tolist()}) == 4
    # inside the configured ranges, taps as blur_taps builds them
    T = aug
    for j in range(4):
        s, k, d, g0, g1, g2, sig = p.chain[j]
        assert T.saturation[0] <= s <= T.saturation[1] and T.contrast[0] <= k <= T.contrast[1] and T.brightness[0] <= d <= T.brightness[1]
        assert all(T.gain[0] <= g <= T.gain[1] for g in (g0, g1, g2)) and T.noise_sigma[0] <= sig <= T.noise_sigma[1]
        assert 2 <= p.radius[j] <= 6 and abs(float(p.taps[j].sum()) - 1) < 1e-6 and not p.taps[j, 2 * p.radius[j] + 1:].any()
    reset_config()


def test_draw_leaves_the_global_generators_alone():
    from deepim.config.config import reset_config
    from lib.utils.augment import ObservedAugmenter

    aug = ObservedAugmenter(_config())
    random.seed(6)
    np.random.seed(3)
    s_py, s_np = random.getstate(), np.random.get_state()
    aug.draw(list(range(16)), 3)
    assert random.getstate() == s_py
    now = np.random.get_state()
    assert now[0] == s_np[0] and np.array_equal(now[1], s_np[1]) and now[2:] == s_np[2:]
    reset_config()


def test_probabilities_and_pinned_ranges():
    from deepim.config.config import reset_config
    from lib.utils.augment import IDENTITY_CHAIN, ObservedAugmenter

    off = ObservedAugmenter(_config(AUG_PROB=0.0)).draw(list(range(64)), 0)
    assert not off.on.any() and not off.radius.any() and np.array_equal(off.chain, np.tile(IDENTITY_CHAIN, (64, 1)))
    some = ObservedAugmenter(_config()).draw(list(range(400)), 0)          # the defaults: 0.8 of the pairs, 0.4 of those blurred
    assert 0.7 < some.on.mean() < 0.9 and 0.25 < (some.radius[some.on == 1] > 0).mean() < 0.55
    assert not some.radius[some.on == 0].any()
    no_blur = ObservedAugmenter(_config(AUG_PROB=1.0, AUG_BLUR_PROB=0.0)).draw(list(range(64)), 0)
    assert no_blur.on.all() and not no_blur.radius.any() and np.all(no_blur.taps[:, 0] == 1) and not no_blur.taps[:, 1:].any()
    pin = ObservedAugmenter(_config(AUG_PROB=1.0, AUG_BLUR_PROB=1.0, AUG_BLUR_SIGMA=[1.0, 1.0], AUG_SATURATION=[0.75, 0.75],
                                    AUG_CONTRAST=[1.1, 1.1], AUG_BRIGHTNESS=[-12.5, -12.5], AUG_GAIN=[1.05, 1.05],
                                    AUG_NOISE_SIGMA=[3.3, 3.3], AUG_QUANTIZE=False))
    p = pin.draw([5, 6, 7], 2)
    want = np.array([0.75, 1.1, -12.5, 1.05, 1.05, 1.05, 3.3], dtype=np.float32)
    from lib.utils.augment import blur_taps

    for j in range(3):
        np.testing.assert_array_equal(p.chain[j], want)
        assert p.radius[j] == 3
        np.testing.assert_array_equal(p.taps[j], blur_taps(1.0)[1])
    assert pin.quantize is False and len({int(s) for s in p.seed}) == 3
    reset_config()


@pytest.mark.parametrize("key,value", [("AUG_BLUR_SIGMA", [2.0, 0.5]), ("AUG_BLUR_SIGMA", [-0.1, 1.0]), ("AUG_BLUR_SIGMA", [0.5, 2.34]),
                                       ("AUG_SATURATION", [1.4, 0.6]), ("AUG_CONTRAST", [1.3, 0.7]), ("AUG_CONTRAST", [-0.2, 1.0]),
                                       ("AUG_BRIGHTNESS", [30.0, -30.0]), ("AUG_GAIN", [1.1, 0.9]), ("AUG_NOISE_SIGMA", [8.0, 0.0]),
                                       ("AUG_NOISE_SIGMA", [-1.0, 8.0]), ("AUG_NOISE_SIGMA", [1.0]), ("AUG_PROB", 1.5),
                                       ("AUG_BLUR_PROB", -0.1)])
def test_bad_ranges_raise_naming_the_key(key, value):
    from deepim.config.config import reset_config
    from lib.utils.augment import ObservedAugmenter

    cfg = _config(**{key: value})
    with pytest.raises(ValueError, match="TRAIN." + key):
        ObservedAugmenter(cfg)
    reset_config()


def test_config_defaults_present_and_off():
    from deepim.config.config import reset_config

    T = reset_config().TRAIN
    assert T.AUG_OBSERVED is False and T.AUG_SEED == 0 and T.AUG_PROB == 0.8 and T.AUG_BLUR_PROB == 0.4
    assert list(T.AUG_BLUR_SIGMA) == [0.5, 2.0] and list(T.AUG_SATURATION) == [0.6, 1.4] and list(T.AUG_CONTRAST) == [0.7, 1.3]
    assert list(T.AUG_BRIGHTNESS) == [-30.0, 30.0] and list(T.AUG_GAIN) == [0.9, 1.1] and list(T.AUG_NOISE_SIGMA) == [0.0, 8.0]
    assert T.AUG_QUANTIZE is True


def test_shipped_yaml_switches_it_on():
    import os

    from conftest import ROOT
    from deepim.config.config import reset_config, update_config
    from lib.utils.augment import ObservedAugmenter

    reset_config()
    cfg = update_config(os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_train_aug.yaml"))
    assert cfg.TRAIN.AUG_OBSERVED is True
    ObservedAugmenter(cfg)
    reset_config()


# ---------------------------------------------------------------------------------------------------------------------- the C entry
def test_entry_argument_errors(hip_lib):
    """the checks run on the host before anything is enqueued: made-up device addresses are never touched"""
    from lib.hip import capi

    assert "dim_augment_observed" in capi.SIGNATURES and hasattr(hip_lib, "dim_augment_observed")
    B, H, W = 2, 8, 16
    nbytes = B * 3 * H * W * 4
    means = np.array([103.939, 116.779, 123.68], dtype=np.float32)
    radius = np.array([0, 7], dtype=np.int32)
    a_in, a_out, dev = 1 << 20, (1 << 20) + nbytes, 1 << 24   # addresses only
    m, r = means.ctypes.data, radius.ctypes.data

    def call(inp=a_in, out=a_out, B=B, H=H, W=W, means=m, on=dev, radius=r, taps=dev, chain=dev, seed=dev):
        return hip_lib.dim_augment_observed(inp, out, B, H, W, means, on, radius, taps, chain, seed, 1, None)

    for kw in ({"inp": None}, {"out": None}, {"means": None}, {"on": None}, {"radius": None}, {"taps": None}, {"chain": None}, {"seed": None}):
        assert call(**kw) == -1 and b"null pointer" in hip_lib.dim_last_error(), kw
    for kw in ({"B": 0}, {"H": 0}, {"W": -4}):
        assert call(**kw) == -1 and b"must be positive" in hip_lib.dim_last_error(), kw
    assert call(W=18) == -1 and b"multiple of 4" in hip_lib.dim_last_error()
    assert call(inp=a_in + 4) == -1 and b"16-byte aligned" in hip_lib.dim_last_error()
    for out in (a_in, a_in + 16, a_in + nbytes - 16, a_in - nbytes + 16):     # the same blob, and overlaps from either side
        assert call(out=out) == -1 and b"alias" in hip_lib.dim_last_error(), out
    for bad in (8, -1, 100):
        rb = np.array([0, bad], dtype=np.int32)
        assert call(radius=rb.ctypes.data) == -1
        msg = hip_lib.dim_last_error()
        assert b"radius" in msg and b"0..7" in msg and str(bad).encode() in msg
