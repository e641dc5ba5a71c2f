"""The plane GEMM of the Winograd layers called directly (dim_winograd_plane_gemm: the launch plan and kernels of csrc/wino_gemm.hip
and csrc/wino_gemm_split.hip, no transforms around them) against a float64 product of the same f32 operands, PER OUTPUT ELEMENT in
units of that element's sum_k |x_k y_k|.

Why direct: the three-term kernel claims f32 accuracy from six bf16 term products per multiply.  A kernel that lost one of the three
third-order products (h l', m m', l h') in one k-step, or paired the terms wrongly, is off by 2^-16 of a product: 1e-6 .. 3e-6 of
max|y| at K = 256, inside every layer-level bar and inside the Winograd transforms' own f32 error.  At K = 32 (one chunk, two
k-steps) and on this measure the intact arithmetic sits near 1e-7 and one dropped product 5 .. 15 times higher.

The bar of a three-term run is 4 x max(the numpy model of the kernel's sum on the same data, this GPU's f32-pipe run of the same call);
tests/test_split_terms.py (no GPU) holds the model -- six_product_dot, imported here -- and the negative controls which show that this
bar catches every single product dropped from a single k-step, for the operand classes, K and bar used here.  The factor 4 covers the
matrix unit's undocumented summation order inside an MFMA.  The f32 pipe (wino_gemm_kernel, tiles 3 .. 7) runs the same cases under
4 x its own model (f32_pipe_dot).

Operand magnitudes stay inside 2^+-40: every term and every term product is then a normal number.  Subnormal bf16 terms (operands
below about 2^-100) are out of scope: the split loses them, as bf16 does.

Measured on an MI355X (worst element, units of sum |x y|): see DESIGN.md, "The three-term arithmetic pinned on the GPU"."""
import numpy as np
import pytest
import torch

from test_split_terms import BAR_FACTOR, OPERAND_CLASSES, f32_pipe_dot, operands, six_product_dot, unit_error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPLIT_TILES = (4, 5, 7)        # wino_gemm_split_kernel<128, 4>, <128, 8>, <96, 4>
F32_TILES = (3, 4, 5, 6, 7)    # wino_gemm_kernel: 64 x 64, 128 x 128, 128 x 256, 160 x 128, 96 x 128 (3 and 6 have no three-term twin)
MODEL_PLANES = 16              # the models run on the first 16 planes of a problem: a maximum over fewer elements, never a wider bar


@pytest.fixture
def arithmetic(hip_lib):
    """sets the arithmetic of the plane GEMMs for the calls of one test; the default (three terms) is back afterwards"""
    from lib.hip import ops

    try:
        yield ops.set_winograd_split
    finally:
        ops.set_winograd_split(True)


def special_operands(kind, rng, P, M, K, N):
    if kind == "same_sign":   # nothing cancels: the sum grows to K times a product, the accumulator's rounding is all there is
        return np.abs(rng.standard_normal((P, M, K))).astype(np.float32), np.abs(rng.standard_normal((P, K, N))).astype(np.float32)
    assert kind == "cancel", kind
    # every (x, y) comes with (x, -y) somewhere else in the run: the exact result is 0, the measure is the error against sum |x y| alone
    x = rng.standard_normal((P, M, K // 2)).astype(np.float32)
    y = rng.standard_normal((P, K // 2, N)).astype(np.float32)
    x, y = np.concatenate([x, x], axis=2), np.concatenate([y, -y], axis=1)
    for p in range(P):
        perm = rng.permutation(K)
        x[p], y[p] = x[p][:, perm], y[p][perm, :]
    return x, y


def problem(kind, T, K, Cout, P, seed):
    """operands, float64 reference and the two models' worst elements of one problem: computed once per test, read-only"""
    rng = np.random.default_rng(seed)
    x, y = (operands if kind in OPERAND_CLASSES else special_operands)(kind, rng, P, T, K, Cout)      # x (P, T, K), y (P, K, Cout)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    exact, unit = np.matmul(x64, y64), np.matmul(np.abs(x64), np.abs(y64))
    mp = min(P, MODEL_PLANES)
    model_split = unit_error(six_product_dot(x[:mp], y[:mp]), x[:mp], y[:mp]).max()
    model_f32 = unit_error(f32_pipe_dot(x[:mp], y[:mp]), x[:mp], y[:mp]).max()
    for a in (x, y, exact, unit):
        a.setflags(write=False)
    return x, y, exact, unit, model_split, model_f32


def run(prob, tile, split, set_arith):
    """one launch into an M full of NaN: (per-element error (P, T, Cout), raw M); asserts the kernel family that ran and finiteness"""
    from lib.hip import ops

    x, y, exact, unit = prob[:4]
    P, T, K = x.shape
    Cout = y.shape[2]
    set_arith(bool(split))
    V = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(DEV)
    U = torch.tensor(y, device=DEV)
    M = torch.full((T, P, Cout), float("nan"), device=DEV)
    M, used = ops.winograd_plane_gemm(V, U, T, K, Cout, P, tile, out=M)
    assert used == (1 if split and tile in SPLIT_TILES else 0), (tile, split, used)
    m = M.cpu().numpy()
    assert m.shape == (T, P, Cout) and np.isfinite(m).all(), (tile, split, "not every element of M written / finite")
    return np.abs(m.transpose(1, 0, 2).astype(np.float64) - exact) / unit, m


def check(prob, split_tiles, f32_tiles, set_arith, what, twice=False):
    """the f32 pipe on f32_tiles under 4 x its model, then the three-term kernel on split_tiles under 4 x max(its model, the f32 pipe's
    run of the same call); twice: the same call again, bit-identical.  Returns {(tile, split): worst element}."""
    worst = {}
    for split, tiles in ((0, f32_tiles), (1, split_tiles)):
        for tile in tiles:
            e, m = run(prob, tile, split, set_arith)
            worst[tile, split] = e.max()
            bar = BAR_FACTOR * (max(prob[4], worst[tile, 0]) if split else prob[5])
            print("%-22s tile %d %-10s GPU %.3e   model: three terms %.3e, f32 %.3e%s   bar %.3e"
                  % (what, tile, "three terms" if split else "f32 pipe", e.max(), prob[4], prob[5],
                     "   GPU f32 pipe %.3e" % worst[tile, 0] if split else "", bar))
            assert e.max() <= bar, (what, tile, "three terms" if split else "f32 pipe", e.max(), bar, np.unravel_index(e.argmax(), e.shape))
            if twice:   # a shared tile is two summands on a zero: the atomics' order does not change the sum
                np.testing.assert_array_equal(run(prob, tile, split, set_arith)[1], m)
    return worst


# ---- term sensitivity: K = 32 = one chunk.  Cout = 256: eight 32-column tiles of U3, both column tiles of tile 5; T = 200: a partial
# last row tile for BM = 128 and 96 (and 64, 160); P = 16
@pytest.mark.parametrize("kind", OPERAND_CLASSES)
def test_one_chunk(arithmetic, kind):
    prob = problem(kind, T=200, K=32, Cout=256, P=16, seed=11 + OPERAND_CLASSES.index(kind))
    check(prob, SPLIT_TILES, F32_TILES, arithmetic, "K=32 " + kind)


# ---- layout reach: 36 and 81 planes, two chunks, every three-term kernel once.  The last case has more items than resident workgroups:
# tile 4 = 128 x 128, so ceil(500 / 128) = 4 row tiles x 2 column tiles x 81 planes = 648 items of 2 chunks = 1296 chunks.  A 4-wave
# three-term workgroup holds 56 KB of LDS and one wave per SIMD at waves_per_eu(2, 2): two per CU, 512 slots on 256 CUs (the f32 pipe's
# 8-wave 128 x 128 workgroup: 52 KB, also two per CU).  648 > 512, so G = 512 ranges of 2 or 3 chunks (1296 = 512 x 2 + 272): the
# first 272 ranges are 3 chunks long, every second boundary among them falls inside an item, and the shared-tile atomics run.
LAYOUT = [("rows", dict(T=200, K=64, Cout=256, P=36), 5),
          ("wide", dict(T=200, K=64, Cout=256, P=81), 7),
          ("randn", dict(T=500, K=64, Cout=256, P=81), 4)]


@pytest.mark.parametrize("case", LAYOUT, ids=["P36-tile5", "P81-tile7", "P81-T500-tile4-cut-items"])
def test_layout_reach_and_bit_identical(arithmetic, case):
    kind, shape, tile = case
    prob = problem(kind, seed=31 + tile, **shape)
    check(prob, (tile,), (tile,), arithmetic, "K=64 P=%d %s" % (shape["P"], kind), twice=True)


# ---- accumulation: long sums.  A dropped term no longer separates from the accumulator's rounding here (checked on the model), so the
# bar of the three-term kernel is the f32 pipe's own error on the same data, and the f32 pipe's is its model's
ACCUMULATION = [("same_sign", dict(T=128, K=1024, Cout=128, P=16), 4),
                ("cancel", dict(T=128, K=256, Cout=128, P=16), 4)]


@pytest.mark.parametrize("case", ACCUMULATION, ids=["same-sign-K1024", "exact-cancellation-K256"])
def test_accumulation_within_4x_f32_pipe(arithmetic, case):
    kind, shape, tile = case
    prob = problem(kind, seed=51, **shape)
    if kind == "cancel":
        assert np.abs(prob[2]).max() <= 1e-12 * prob[3].min()       # the float64 reference is 0 up to its own rounding
    e_f32, e_split = run(prob, tile, 0, arithmetic)[0].max(), run(prob, tile, 1, arithmetic)[0].max()
    print("K=%d %-10s tile %d: GPU three terms %.3e  GPU f32 pipe %.3e  ratio %.2f   model: three terms %.3e, f32 %.3e"
          % (shape["K"], kind, tile, e_split, e_f32, e_split / e_f32, prob[4], prob[5]))
    assert e_f32 <= BAR_FACTOR * prob[5], (kind, e_f32, prob[5])
    assert e_split <= BAR_FACTOR * e_f32, (kind, e_split, e_f32)


def test_argument_errors(hip_lib):
    """K % 32, Cout % 64, null and host pointers: DIM_ERR_ARG (-1), nothing enqueued"""
    import ctypes

    used = ctypes.c_int(-7)
    n = hip_lib.dim_winograd_plane_gemm_weight_floats(32, 64, 16)
    V = torch.zeros((8, 16, 32), device=DEV)
    U = torch.zeros((n,), device=DEV)
    M = torch.full((8, 16, 64), 3.0, device=DEV)
    host = np.zeros(n, np.float32)
    call = lambda v, u, m, K=32, Cout=64, us=ctypes.byref(used): hip_lib.dim_winograd_plane_gemm(v, u, m, 8, K, Cout, 16, 3, us, None)
    assert call(V.data_ptr(), U.data_ptr(), M.data_ptr(), K=48) == -1
    assert call(V.data_ptr(), U.data_ptr(), M.data_ptr(), Cout=96) == -1
    assert call(None, U.data_ptr(), M.data_ptr()) == -1 and call(V.data_ptr(), None, M.data_ptr()) == -1
    assert call(V.data_ptr(), U.data_ptr(), None) == -1 and call(V.data_ptr(), U.data_ptr(), M.data_ptr(), us=None) == -1
    assert call(V.data_ptr(), host.ctypes.data, M.data_ptr()) == -1 and call(host.ctypes.data, U.data_ptr(), M.data_ptr()) == -1
    assert hip_lib.dim_winograd_plane_gemm_split_weights(host.ctypes.data, 32, 64, 16, None) == -1
    assert hip_lib.dim_winograd_plane_gemm_split_weights(None, 32, 64, 16, None) == -1
    assert hip_lib.dim_winograd_plane_gemm_split_weights(U.data_ptr(), 40, 64, 16, None) == -1
    torch.cuda.synchronize()
    assert used.value == -7 and bool((M == 3.0).all())
    assert call(V.data_ptr(), U.data_ptr(), M.data_ptr()) == 0 and used.value == 0     # tile 3: the f32 pipe whatever the switch
    torch.cuda.synchronize()
    assert bool((M == 0.0).all())
