"""The arithmetic of csrc/wino_gemm_split.hip restated in numpy (no GPU): an f32 number as three bf16 terms, a product as the six
largest term products.  Checks the bounds the kernel's header states, on random and on adversarial operands, and -- the negative
controls at the end -- that the per-element bar of tests/test_gpu_split_gemm.py catches every single term product left out of a single
k-step.  That file imports the model (six_product_dot, f32_pipe_dot), the operand classes and the error measure from here."""
import numpy as np


def bf16_rne(x):
    """float32 -> nearest bfloat16 (ties to even), returned as float32: what v_cvt_pk_bf16_f32 does for finite inputs"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) << 16).astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r1 = x - h            # exact in f32
    m = bf16_rne(r1)
    r2 = r1 - m           # exact in f32
    return h, m, bf16_rne(r2)


def rand_operands(rng, n):
    mant = rng.uniform(1.0, 2.0, n)
    expo = rng.integers(-20, 20, n)
    sign = rng.choice([-1.0, 1.0], n)
    return (sign * mant * 2.0 ** expo).astype(np.float32)


def test_three_terms_rebuild_the_number():
    rng = np.random.default_rng(0)
    x = np.concatenate([rand_operands(rng, 200000), np.float32([0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 3.0e38, 1.0e-30,
                                                                   np.pi, -np.e, 255.0 / 256.0, 1.0 + 2.0 ** -8 + 2.0 ** -16])])
    h, m, l = split3(x)
    x64 = x.astype(np.float64)
    # the subtractions are exact: r1, r2 computed in f32 equal the f64 differences
    assert np.array_equal((x - h).astype(np.float64), x64 - h.astype(np.float64))
    assert np.array_equal(((x - h) - m).astype(np.float64), x64 - h.astype(np.float64) - m.astype(np.float64))
    rest = np.abs(x64 - (h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)))
    assert np.all(rest <= 2.0 ** -27 * np.abs(x64))
    # most f32 numbers are rebuilt exactly (24 significant bits fit in 3 x 8 plus the signs)
    assert (rest == 0).mean() > 0.9
    # term sizes: |m| <= 2^-8 |h|-ish, |l| <= 2^-16
    assert np.all(np.abs(m) <= 2.0 ** -8 * np.abs(x) * (1 + 2.0 ** -7)) and np.all(np.abs(l) <= 2.0 ** -17 * np.abs(x) * (1 + 2.0 ** -6))


def test_six_products_are_a_product_to_f32_accuracy():
    rng = np.random.default_rng(1)
    x, y = rand_operands(rng, 300000), rand_operands(rng, 300000)
    xs = [t.astype(np.float64) for t in split3(x)]
    ys = [t.astype(np.float64) for t in split3(y)]
    six = xs[0] * ys[0] + (xs[0] * ys[1] + xs[1] * ys[0]) + (xs[0] * ys[2] + xs[1] * ys[1] + xs[2] * ys[0])
    exact = x.astype(np.float64) * y.astype(np.float64)
    err = np.abs(six - exact) / np.abs(exact)
    assert err.max() <= 3.5 * 2.0 ** -26, err.max()       # the dropped terms m l' + l m' + l l' and the two rests
    assert err.max() < 2.0 ** -24                         # below half an ulp of the f32 product itself
    # every term product is exact in f32 (8 x 8 significant bits): the matrix pipe adds exact numbers
    for a in xs:
        for b in ys:
            p = a * b
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p) or np.all(np.abs(p[p.astype(np.float32) != p]) < 1e-37)


# ---------------------------------------------------------------------------------------------------------------- the kernel's sum
# (A's term, B's term) of the six MFMAs of a k-step of 16, in issue order, for the two k-steps of a chunk of 32 (0 = h, 1 = m, 2 = l):
# kTA / kTB of csrc/wino_gemm_split.hip.  A = the first operand (V, the transformed input), B = the second (U, the weights).
TERM_ORDER = (((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)),
              ((2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)))
SIX = TERM_ORDER[0]
OPERAND_CLASSES = ("randn", "wide", "rows")


def six_product_dot(x, y, drop=None, step=None, order=TERM_ORDER):
    """x (..., M, K) . y (..., K, N) as wino_gemm_split_kernel sums it: per k-step of 16 six term products in the kernel's issue order,
    each a 16-term sum of exact products (float64 here: the matrix unit's own order inside an MFMA is not modelled), added to an f32
    accumulator one after the other.  drop = (A's term, B's term) leaves that product out of k-step `step` (None: of every k-step):
    the defect the bar has to catch.  order: other term pairs per k-step parity (a mispaired kTA / kTB)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    K = x.shape[-1]
    assert K % 16 == 0 and y.shape[-2] == K
    xs = [t.astype(np.float64) for t in split3(x)]
    ys = [t.astype(np.float64) for t in split3(y)]
    acc = np.zeros(np.broadcast_shapes(x.shape[:-2], y.shape[:-2]) + (x.shape[-2], y.shape[-1]), np.float32)
    for s in range(K // 16):
        k = slice(16 * s, 16 * s + 16)
        for ta, tb in order[s & 1]:
            if drop is not None and (ta, tb) == tuple(drop) and (step is None or step == s):
                continue
            acc = (acc.astype(np.float64) + np.matmul(xs[ta][..., :, k], ys[tb][..., k, :])).astype(np.float32)
    return acc


def f32_pipe_dot(x, y):
    """the same product as wino_gemm_kernel sums it on the f32 pipe: v_mfma_f32_32x32x2_f32 adds the two exact products k, k + 4 of a
    group of 8 to the f32 accumulator (the two lane halves hold k = 8 g + j and 8 g + 4 + j)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    K = x.shape[-1]
    assert K % 8 == 0 and y.shape[-2] == K
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    acc = np.zeros(np.broadcast_shapes(x.shape[:-2], y.shape[:-2]) + (x.shape[-2], y.shape[-1]), np.float32)
    for g in range(K // 8):
        for j in range(4):
            k = [8 * g + j, 8 * g + 4 + j]
            acc = (acc.astype(np.float64) + np.matmul(x64[..., :, k], y64[..., k, :])).astype(np.float32)
    return acc


def unit_error(got, x, y):
    """per output element |got - exact| / sum_k |x_k y_k|, exact = the float64 product of the same f32 operands: the unit in which a
    lost term product shows whatever the element's size and however much of it cancels"""
    x64, y64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    exact = np.matmul(x64, y64)
    unit = np.matmul(np.abs(x64), np.abs(y64))
    diff = np.abs(np.asarray(got).astype(np.float64) - exact)
    # an element whose every product is zero (a border pixel of a convolution) has to be exactly zero
    return np.where(unit > 0, diff / np.where(unit > 0, unit, 1.0), np.where(diff == 0, 0.0, np.inf))


def operands(kind, rng, P, M, K, N):
    """x (P, M, K), y (P, K, N) of one operand class.  randn: standard normal.  wide: sign * [1, 2) * 2^e with e uniform in -40 .. 39
    per element, on both operands.  rows: the same spread, one e per row of x and per column of y.  Magnitudes stay inside 2^+-40, so
    every term (>= 2^-40-24) and every term product is a normal bf16 / f32 number: subnormal terms are out of scope."""
    if kind == "randn":
        return rng.standard_normal((P, M, K)).astype(np.float32), rng.standard_normal((P, K, N)).astype(np.float32)

    def spread(shape, eshape):
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-40, 40, eshape)).astype(np.float32)
    if kind == "wide":
        return spread((P, M, K), (P, M, K)), spread((P, K, N), (P, K, N))
    assert kind == "rows", kind
    return spread((P, M, K), (P, M, 1)), spread((P, K, N), (P, 1, N))


def test_dot_products_match_f32_accumulation():
    """K = 1024 dot products: six-product sums accumulated in f32 against f64 -- the error is that of an f32 accumulation, the same as
    with exact f32 products (what v_mfma_f32_32x32x2_f32 does)"""
    rng = np.random.default_rng(2)
    K, n = 1024, 2000
    x = rng.standard_normal((n, 1, K)).astype(np.float32)
    y = rng.standard_normal((n, K, 1)).astype(np.float32)
    exact = np.matmul(x.astype(np.float64), y.astype(np.float64))
    scale = np.sqrt(K)
    e6 = np.abs(six_product_dot(x, y) - exact).max() / scale
    ef = np.abs(f32_pipe_dot(x, y) - exact).max() / scale
    assert e6 < 4e-6 and e6 < 4 * ef + 1e-7, (e6, ef)


# ---------------------------------------------------------------------------------------------------------------- negative controls
BAR_FACTOR = 4.0    # the bar of the GPU tests: 4 x the intact model's own worst element (there also: x the f32 pipe's, if larger)


def test_model_catches_every_dropped_product_at_one_chunk():
    """K = 32 (one chunk = two k-steps), 6144 outputs per operand class.  The intact model is within the bar by construction; with any
    one of the six term products left out of any one k-step the worst element is at least 2 x over it and at least 20 % of the elements
    are over it -- also for the third-order products h l', m m', l h', which cost 2^-16 of a product and pass every layer-level bar."""
    for ci, kind in enumerate(OPERAND_CLASSES):
        x, y = operands(kind, np.random.default_rng(100 + ci), 4, 48, 32, 32)
        intact = unit_error(six_product_dot(x, y), x, y)
        bar = BAR_FACTOR * intact.max()
        assert intact.size >= 4096 and intact.max() <= bar and intact.max() < 2.0 ** -22, (kind, intact.max())
        for drop in SIX:
            for step in (0, 1):
                e = unit_error(six_product_dot(x, y, drop=drop, step=step), x, y)
                worst, share = e.max() / bar, (e > bar).mean()
                print("%-5s drop %s step %d: worst %8.1f x bar, %4.1f %% of the elements over (bar %.2e)" % (kind, drop, step, worst, 100 * share, bar))
                assert worst >= 2.0, (kind, drop, step, worst)
                assert share >= 0.2, (kind, drop, step, share)


def test_model_catches_a_mispaired_k_step():
    """k-step 1 issued with A's terms of step 1 against B's terms of step 0 (kTA[1] with kTB[0]): (m, l'), (m, m'), (h, h') twice --
    two products lost, one doubled"""
    bad = (TERM_ORDER[0], tuple((a, b) for (a, _), (_, b) in zip(TERM_ORDER[1], TERM_ORDER[0])))
    assert set(bad[1]) != set(SIX)
    for ci, kind in enumerate(OPERAND_CLASSES):
        x, y = operands(kind, np.random.default_rng(200 + ci), 4, 48, 32, 32)
        bar = BAR_FACTOR * unit_error(six_product_dot(x, y), x, y).max()
        e = unit_error(six_product_dot(x, y, order=bad), x, y)
        assert e.max() >= 2.0 * bar and (e > bar).mean() >= 0.2, (kind, e.max() / bar, (e > bar).mean())


def test_both_k_step_orders_hold_the_same_six_products():
    assert all(sorted(o) == sorted(SIX) and o[-1] == (0, 0) for o in TERM_ORDER)
    assert sorted(SIX) == sorted((a, b) for a in range(3) for b in range(3) if a + b <= 2)
