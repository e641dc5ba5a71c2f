"""Photometric augmentation of the observed training image: the host half.

`ObservedAugmenter(config)` turns the TRAIN.AUG_* ranges into the per-pair parameter arrays of dim_augment_observed (csrc/augment.hip;
include/deepim_hip.h lists the kernel's rules).  As with mask_dilate the draws are made here and the kernel is deterministic.

The draws of a pair come from a generator of their own, np.random.RandomState seeded from (TRAIN.AUG_SEED, epoch, key), never from the
global `random` / `np.random` generators: TrainDataLoader._stage replays the reference's global draws in the reference's order, and that
order -- every label, background choice and dilate thickness of a seeded run -- is the same with the augmentation on or off.  `key`
is a stable integer per pair: its index in the pairdb (file loader), batch_id * batch_pairs + slot (SyntheticPairs).

Per pair, always in this order and always all of them (so one component's range does not move another's draw):
  u_on, u_blur = random_sample() twice; blur sigma, saturation, contrast, brightness = uniform(lo, hi) each; gain of blob plane 0, 1,
  2 = uniform(lo, hi) three times; noise sigma = uniform(lo, hi); noise seed = randint(0, 2**32).
on = u_on < AUG_PROB; the pair is blurred when u_blur < AUG_BLUR_PROB.  A range [a, a] pins its component to a.
"""
from __future__ import division

import math

import numpy as np

MAX_RADIUS = 7
N_TAPS = 2 * MAX_RADIUS + 1
CHAIN = ("saturation", "contrast", "brightness", "gain_0", "gain_1", "gain_2", "noise_sigma")   # the columns of `chain`
IDENTITY_CHAIN = np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0], dtype=np.float32)


def blur_radius(sigma):
    """r = min(7, ceil(3 sigma)); sigma 0 = no blur"""
    return min(MAX_RADIUS, int(math.ceil(3.0 * float(sigma))))


def blur_taps(sigma):
    """-> (r, taps float32 (15,)): exp(-x^2 / 2 sigma^2) for x = -r .. r in float64, normalised, cast to float32; entries past 2 r + 1
    are 0.  r = 0 (sigma = 0): the single tap 1, which the kernel does not multiply by."""
    r = blur_radius(sigma)
    taps = np.zeros((N_TAPS,), dtype=np.float32)
    if r == 0:
        taps[0] = 1.0
        return 0, taps
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    taps[:2 * r + 1] = (g / g.sum()).astype(np.float32)
    return r, taps


class AugmentParams(object):
    """the per-pair arrays of one batch on the host: on (B,) int32, radius (B,) int32, taps (B,15) float32, chain (B,7) float32
    (columns: CHAIN), seed (B,) uint32"""

    def __init__(self, B):
        self.on = np.zeros((B,), dtype=np.int32)
        self.radius = np.zeros((B,), dtype=np.int32)
        self.taps = np.zeros((B, N_TAPS), dtype=np.float32)
        self.taps[:, 0] = 1.0
        self.chain = np.tile(IDENTITY_CHAIN, (B, 1))
        self.seed = np.zeros((B,), dtype=np.uint32)

    def __len__(self):
        return self.on.shape[0]

    def to_device(self, device):
        """-> the device tensors of ops.augment_observed (the seed as the int32 with the same bits); radius stays on the host"""
        import torch

        return {"on": torch.from_numpy(self.on).to(device), "taps": torch.from_numpy(self.taps).to(device),
                "chain": torch.from_numpy(self.chain).to(device), "seed": torch.from_numpy(self.seed.view(np.int32)).to(device)}


def _range(train, key, lo_min=None):
    v = train[key]
    try:
        lo, hi = float(v[0]), float(v[1])
        ok = len(v) == 2 and math.isfinite(lo) and math.isfinite(hi)
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok:
        raise ValueError("TRAIN.{}: expected [lo, hi], got {!r}".format(key, v))
    if lo > hi:
        raise ValueError("TRAIN.{}: lo > hi in {!r}".format(key, v))
    if lo_min is not None and lo < lo_min:
        raise ValueError("TRAIN.{}: values below {} in {!r}".format(key, lo_min, v))
    return lo, hi


def _prob(train, key):
    p = float(train[key])
    if not 0.0 <= p <= 1.0:
        raise ValueError("TRAIN.{}: a probability in [0, 1] expected, got {!r}".format(key, train[key]))
    return p


class ObservedAugmenter(object):
    def __init__(self, config):
        T = config.TRAIN
        self.seed = int(T.AUG_SEED)
        self.prob, self.blur_prob = _prob(T, "AUG_PROB"), _prob(T, "AUG_BLUR_PROB")
        self.blur_sigma = _range(T, "AUG_BLUR_SIGMA", lo_min=0.0)
        if math.ceil(3.0 * self.blur_sigma[1]) > MAX_RADIUS:
            raise ValueError("TRAIN.AUG_BLUR_SIGMA: sigma {} needs radius ceil(3 sigma) = {}, the kernel blurs up to radius {}".format(
                self.blur_sigma[1], int(math.ceil(3.0 * self.blur_sigma[1])), MAX_RADIUS))
        self.saturation = _range(T, "AUG_SATURATION")
        self.contrast = _range(T, "AUG_CONTRAST", lo_min=0.0)
        self.brightness = _range(T, "AUG_BRIGHTNESS")
        self.gain = _range(T, "AUG_GAIN", lo_min=0.0)
        self.noise_sigma = _range(T, "AUG_NOISE_SIGMA", lo_min=0.0)
        self.quantize = bool(T.AUG_QUANTIZE)

    def generator(self, epoch, key):
        """the pair's own generator: MT19937 initialised from the words (AUG_SEED, epoch, key low, key high)"""
        key = int(key)
        words = [self.seed & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF]
        return np.random.RandomState(np.array(words, dtype=np.uint32))

    def draw(self, keys, epoch):
        """keys: one stable integer per pair -> AugmentParams of len(keys) pairs"""
        p = AugmentParams(len(keys))
        for j, key in enumerate(keys):
            rs = self.generator(epoch, key)
            u_on, u_blur = rs.random_sample(), rs.random_sample()
            sigma = rs.uniform(*self.blur_sigma)
            chain = [rs.uniform(*self.saturation), rs.uniform(*self.contrast), rs.uniform(*self.brightness)]
            chain += [rs.uniform(*self.gain) for _ in range(3)]
            chain.append(rs.uniform(*self.noise_sigma))
            seed = rs.randint(0, 2 ** 32, dtype=np.uint32)
            if not u_on < self.prob:
                continue   # left alone: on = 0, neutral parameters
            p.on[j] = 1
            if u_blur < self.blur_prob:
                p.radius[j], p.taps[j] = blur_taps(sigma)
            p.chain[j] = np.asarray(chain, dtype=np.float32)
            p.seed[j] = seed
        return p

    def apply(self, image, params, pixel_means_bgr, out=None):
        """image (B,3,H,W) device blob -> its augmented copy (params uploaded here; the file loader ships them with its staging set)"""
        from lib.hip import ops

        d = params.to_device(image.device)
        return ops.augment_observed(image, d["on"], params.radius, d["taps"], d["chain"], d["seed"], pixel_means_bgr, quantize=self.quantize,
                                    out=out)
