"""Numpy float32 restatement of dim_augment_observed, written from the rule list in include/deepim_hip.h (not from the kernel): the
integer hash and the noise, the separable replicate-border blur with sums accumulated in ascending tap order, the colour chain,
clamp, rounding.  Every product and every sum is a float32 operation of its own, as in a library built without fused multiply-add,
so the kernel is compared with np.array_equal."""
import numpy as np

F = np.float32
NOISE_SCALE = F(2.6428997e-05)   # 1 / sqrt((2^32 - 1) / 3): the sum of four 16-bit uniforms has that variance


def mix(x):
    """uint32 array -> uint32 array, wrapping"""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def noise(seed, counter):
    """seed: uint32 scalar, counter: uint32 array -> float32 array, unit variance, within +-3.4642"""
    counter = np.asarray(counter, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h0 = mix(np.uint32(seed) + counter * np.uint32(0x9E3779B9))
    h1 = mix(h0 ^ np.uint32(0x85EBCA6B))
    s = (h0 & np.uint32(0xFFFF)).astype(np.int64) + (h0 >> np.uint32(16)).astype(np.int64) \
        + (h1 & np.uint32(0xFFFF)).astype(np.int64) + (h1 >> np.uint32(16)).astype(np.int64)
    return (s - 131070).astype(F) * NOISE_SCALE


def noise_planes(seed, H, W):
    """(3, H, W) float32: the noise of every pixel of a pair, counter (c * H + y) * W + x"""
    n = np.arange(3 * H * W, dtype=np.uint64).astype(np.uint32).reshape(3, H, W)
    return noise(seed, n)


def blur_axis(v, taps, r, axis):
    """1-D blur of float32 `v` along `axis`: coordinates clamped to the image, acc = 0, then acc = acc + w_t * v[i - r + t] for
    t = 0 .. 2 r"""
    n = v.shape[axis]
    acc = np.zeros_like(v)
    for t in range(2 * r + 1):
        idx = np.clip(np.arange(n) - r + t, 0, n - 1)
        acc = acc + F(taps[t]) * np.take(v, idx, axis=axis)
    return acc


def blur(v, taps, r):
    """v (3, H, W) float32: rows first (along x), then the columns of the row-blurred values; r = 0 leaves v alone"""
    if r == 0:
        return v
    return blur_axis(blur_axis(v, taps, r, axis=2), taps, r, axis=1)


def augment_pair(blob, means_bgr, radius, taps, chain, seed, quantize):
    """blob (3, H, W) float32, mean-subtracted, plane c = BGR channel 2 - c -> the augmented blob of a pair that is on"""
    blob = np.asarray(blob, dtype=F)
    _, H, W = blob.shape
    mean = np.asarray(means_bgr, dtype=F).reshape(3)[::-1].reshape(3, 1, 1)   # of plane c
    v = blur(blob + mean, np.asarray(taps, dtype=F), int(radius))
    s, k, d = F(chain[0]), F(chain[1]), F(chain[2])
    gain = [F(chain[3]), F(chain[4]), F(chain[5])]
    sigma = F(chain[6])
    gray = F(0.299) * v[0] + F(0.587) * v[1] + F(0.114) * v[2]   # plane 0 is red
    nz = noise_planes(seed, H, W) if sigma != 0 else None
    out = np.empty_like(v)
    for c in range(3):
        t = gray + s * (v[c] - gray)
        t = (t - F(128)) * k + F(128) + d
        t = t * gain[c]
        if nz is not None:
            t = t + sigma * nz[c]
        t = np.minimum(np.maximum(t, F(0)), F(255))
        if quantize:
            t = np.rint(t)
        out[c] = t - mean[c]
    assert out.dtype == F
    return out


def augment(blob, means_bgr, on, radius, taps, chain, seed, quantize):
    """blob (B, 3, H, W) and the per-pair arrays of lib/utils/augment.AugmentParams -> the augmented blob; on[b] == 0 copies the pair"""
    blob = np.asarray(blob, dtype=F)
    out = blob.copy()
    for b in range(blob.shape[0]):
        if int(on[b]) != 0:
            out[b] = augment_pair(blob[b], means_bgr, radius[b], taps[b], chain[b], np.uint32(seed[b]), quantize)
    return out
