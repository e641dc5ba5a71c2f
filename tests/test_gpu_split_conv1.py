"""The first layer's three-term kernel (conv1_halo_split_kernel, csrc/conv_first.hip: tile 6 of conv2d_fwd with the three-term switch
on) on the measure of tests/test_gpu_split_gemm.py: per output element, |got - float64| / sum |x w|.

The layer's K is fixed at 392 = 49 taps x 8 channels, where a dropped third-order term product no longer separates from the
accumulator's rounding.  So the EFFECTIVE K is made small: in case i only the four flat taps 4 i .. 4 i + 3 -- packed chunk i, the
two MFMAs 2 i and 2 i + 1 of the kernel's tap-pair loop -- carry non-zero weights (case 12: tap 48 alone; the slot of "tap 49" stays
the packing's zero).  That is 32 products per output, each MFMA's two tap halves in turn, under the bar of the plane GEMM's one-chunk
test: 4 x max(numpy model at K = 32, the f32-pipe kernel conv1_halo_kernel on the same data).  The f32-pipe kernel runs under 4 x its
own model.  A dense case (all 49 taps) holds the three-term kernel within 4 x the f32 pipe's error.

Shape: 3 x 37 x 53 x 8 -> 19 x 27 x 64: partial 16 x 16 blocks on both axes, pixels of the padding in the patches (an output whose
four taps all lie in the padding is exactly zero)."""
import numpy as np
import pytest
import torch

from test_split_terms import BAR_FACTOR, f32_pipe_dot, six_product_dot, unit_error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, W, CIN, COUT, KS, STRIDE, PAD = 3, 37, 53, 8, 64, 7, 2, 3
HO, WO = (H + 2 * PAD - KS) // STRIDE + 1, (W + 2 * PAD - KS) // STRIDE + 1


@pytest.fixture
def arithmetic(hip_lib):
    """sets the arithmetic (three terms / f32 pipe) for the calls of one test; the default (three terms) is back afterwards"""
    from lib.hip import ops

    try:
        yield ops.set_winograd_split
    finally:
        ops.set_winograd_split(True)


def tensors(kind, rng):
    """x (N, H, W, 8) and w (64, 8, 7, 7) of one operand class (test_split_terms.operands: randn, or sign * [1, 2) * 2^(-40 .. 39))"""
    if kind == "randn":
        return rng.standard_normal((N, H, W, CIN)).astype(np.float32), rng.standard_normal((COUT, CIN, KS, KS)).astype(np.float32)

    def spread(shape):
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-40, 40, shape)).astype(np.float32)
    return spread((N, H, W, CIN)), spread((COUT, CIN, KS, KS))


def patches(x, taps):
    """(8 len(taps), N HO WO): the input values under the given flat taps, k = 8 * (position in taps) + channel -- the k order of the
    packed weights (4 taps x 8 channels per chunk) and of the kernels' MFMAs"""
    xp = np.zeros((N, H + 2 * PAD, W + 2 * PAD, CIN), np.float32)
    xp[:, PAD:PAD + H, PAD:PAD + W] = x
    cols = [xp[:, t // KS:t // KS + STRIDE * HO:STRIDE, t % KS:t % KS + STRIDE * WO:STRIDE, :] for t in taps]      # each (N, HO, WO, 8)
    return np.stack(cols, axis=3).reshape(N * HO * WO, 8 * len(taps)).T.copy()


def gpu_conv(x, w, split, set_arith):
    """tile 6, no bias, slope 1: the raw sums, (64, N HO WO), from an output full of NaN"""
    from lib.hip import ops

    set_arith(bool(split))
    wp = ops.conv2d_pack_weight(torch.from_numpy(w).to(DEV))
    out = torch.full((N, HO, WO, COUT), float("nan"), device=DEV)
    y = ops.conv2d_fwd(torch.from_numpy(x).to(DEV), wp, None, COUT, KS, KS, STRIDE, PAD, slope=1.0, tile=6, out=out).cpu().numpy()
    assert y.shape == (N, HO, WO, COUT) and np.isfinite(y).all(), "not every output written / finite"
    return y.reshape(N * HO * WO, COUT).T


@pytest.mark.parametrize("kind", ["randn", "wide"])
def test_one_chunk_of_taps_at_a_time(arithmetic, kind):
    rng = np.random.default_rng(71 if kind == "randn" else 72)
    x, w_all = tensors(kind, rng)
    failed = []
    for i in range(13):
        taps = [t for t in range(4 * i, 4 * i + 4) if t < KS * KS]
        w = np.zeros_like(w_all)
        for t in taps:
            w[:, :, t // KS, t % KS] = w_all[:, :, t // KS, t % KS]
        B = patches(x, taps)                                                       # (8 taps, pixels)
        A = np.stack([w[:, :, t // KS, t % KS] for t in taps], axis=1).reshape(COUT, 8 * len(taps))     # (64, 8 taps): the MFMA's A operand
        if len(taps) < 4:       # the model's k-steps are 16 wide: the zero slots of the last chunk
            A = np.concatenate([A, np.zeros((COUT, 32 - A.shape[1]), np.float32)], axis=1)
            B = np.concatenate([B, np.zeros((32 - B.shape[0], B.shape[1]), np.float32)], axis=0)
        model_split = unit_error(six_product_dot(A, B), A, B).max()
        model_f32 = unit_error(f32_pipe_dot(A, B), A, B).max()
        e_f32 = unit_error(gpu_conv(x, w, 0, arithmetic), A, B).max()
        e_split = unit_error(gpu_conv(x, w, 1, arithmetic), A, B).max()
        bar = BAR_FACTOR * max(model_split, e_f32)
        print("conv1 %-5s chunk %2d: GPU three terms %.3e  GPU f32 pipe %.3e   model: three terms %.3e, f32 %.3e   bar %.3e"
              % (kind, i, e_split, e_f32, model_split, model_f32, bar))
        if not e_f32 <= BAR_FACTOR * model_f32:
            failed.append(("f32 pipe", i, e_f32, BAR_FACTOR * model_f32))
        if not e_split <= bar:
            failed.append(("three terms", i, e_split, bar))
    assert not failed, failed


def test_dense_within_4x_f32_pipe(arithmetic):
    x, w = tensors("randn", np.random.default_rng(73))
    taps = list(range(KS * KS))
    B = patches(x, taps)
    A = np.stack([w[:, :, t // KS, t % KS] for t in taps], axis=1).reshape(COUT, 8 * len(taps))
    e_f32 = unit_error(gpu_conv(x, w, 0, arithmetic), A, B).max()
    e_split = unit_error(gpu_conv(x, w, 1, arithmetic), A, B).max()
    model_f32 = unit_error(f32_pipe_dot(A, B), A, B).max()
    print("conv1 dense K=392: GPU three terms %.3e  GPU f32 pipe %.3e  ratio %.2f   model f32 %.3e" % (e_split, e_f32, e_split / e_f32, model_f32))
    assert e_f32 <= BAR_FACTOR * model_f32, (e_f32, model_f32)
    assert e_split <= BAR_FACTOR * e_f32, (e_split, e_f32)
