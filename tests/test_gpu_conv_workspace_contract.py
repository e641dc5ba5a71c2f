"""The workspace, packed-buffer and output-window contract of the convolution, FC and gradient entry points (include/deepim_hip.h,
"Caller-owned buffers of the convolution stack"), on guarded buffers (tests/guard_arena.py):

  a. a call writes nothing outside the declared size of its workspace, and nothing outside its output (window);
  b. every result is finite and within the bar the entry's existing f64 test asserts (named at each row);
  c. the result does not depend on what the workspace held: zero, NaN and +inf words and what another shape's call left behind give
     the same bits -- after the precondition, asserted first, that two calls on a zeroed workspace give the same bits;
  d. channels outside an output's window keep their sentinel bit for bit;
  e. a row that is meant to reach a branch asserts with the library's host-side queries that it does.

Every workspace has exactly the size its dim_*_workspace_floats function reports and starts 256-byte aligned; every guard is >= 1 MiB.
Packers: two images packed into NaN- and zero-prefilled buffers of exactly dim_*_packed_weight_floats are bit-identical (every word is
written), and a forward through the image packed over NaN meets the f64 bar.

No row is known to miss the precondition of c.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_arena as ga

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, bf16 = torch.float32, torch.bfloat16
FILLS = (("zero", ga.ZERO_WORD), ("zero again", ga.ZERO_WORD), ("nan", ga.NAN_WORD), ("inf", ga.INF_WORD), ("stale", None))


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


@pytest.fixture(params=[1, 0], ids=["bf16x3", "f32pipe"])
def wino_split(request, ops):
    """both arithmetics of the plane GEMMs and of the first layer's tile 6: three bf16 terms (the default), and the f32 matrix pipe"""
    ops.set_winograd_split(bool(request.param))
    yield request.param
    ops.set_winograd_split(True)


class Row(object):
    """need: workspace floats (0: the entry takes none); call(ws) -> [ChannelWindow] outputs; verify([inside arrays], what); branch():
    the assertion of e"""

    def __init__(self, need, call, verify, branch=None, inspect=None):
        """inspect(workspace after the call on the NaN fill): what a row can say about its branch from the words the call wrote"""
        self.need, self.call, self.verify, self.branch, self.inspect = int(need), call, verify, branch, inspect


def contract(row, stale_row=None, what=""):
    """a .. e for one row; stale_row: the same entry at another shape, whose workspace contents are the last fill"""
    if row.branch:
        row.branch()
    if row.need == 0:        # no workspace: the guarded outputs, twice
        fills = FILLS[:2]
    else:
        assert stale_row is not None and stale_row.need > 0, what
        fills = FILLS
    results = []
    for name, word in fills:
        ws = None
        if row.need:
            ws = ga.GuardArena(row.need, device=DEV, fill=ga.ZERO_WORD if word is None else word)
            if word is None:
                left = ga.GuardArena(stale_row.need, device=DEV, fill=ga.ZERO_WORD)
                for o in stale_row.call(left.view()):
                    o.check("{}: output of the call that leaves the stale workspace".format(what))
                left.check("{}: workspace of the call that leaves the stale workspace".format(what))
                assert bool((left.view() != 0).any()), "the stale workspace is all zero"
                ws.fill_from(left.view())
        outs = row.call(ws.view() if ws is not None else None)
        if ws is not None:
            ws.check("{} [{} workspace of {} floats]".format(what, name, row.need))                       # a
            if name == "nan":
                # the call went through this buffer (a wrapper that found it too small would have allocated its own, and every
                # check above would pass on an arena nobody used)
                assert not bool(torch.isnan(ws.view()).all()), "{}: the workspace in the arena was not used".format(what)
                if row.inspect:
                    row.inspect(ws.view())
        for i, o in enumerate(outs):
            o.check("{} [{} workspace] output {}".format(what, name, i))                                  # a, d
        got = [o.inside() for o in outs]
        for i, g in enumerate(got):
            assert np.isfinite(g).all(), "{} [{} workspace] output {}: {} non-finite values".format(what, name, i, int((~np.isfinite(g)).sum()))
        row.verify(got, "{} [{} workspace]".format(what, name))                                          # b
        results.append((name, got))
    (_, first), (_, again) = results[:2]
    for a, b in zip(first, again):
        assert np.array_equal(a, b), "{}: two calls on a zeroed workspace differ (the precondition of c)".format(what)
    for name, got in results[2:]:
        for i, (a, b) in enumerate(zip(first, got)):
            diff = int((a != b).sum())
            assert diff == 0, "{}: output {} depends on the workspace's contents: {} of {} values differ between the zero and the {} fill (max {:.3e})".format(
                what, i, diff, a.size, name, float(np.abs(a.astype(np.float64) - b).max()))                # c


def test_the_driver_sees_what_it_is_there_to_see(ops):
    """negative controls of contract() on stand-in entries made of torch operations: one word written behind the workspace, a result
    that takes a word from the workspace, a result that differs from call to call, and a write into the channel next to the window
    each fail with the message of their assertion; the well-behaved stand-in passes"""
    n, calls = 1000, [0]
    x = torch.arange(24, dtype=f32).reshape(2, 3, 4)

    def stand_in(overrun=False, reads=False, drifts=False, spills=False):
        def call(ws):
            calls[0] += 1
            y = ga.ChannelWindow((2, 3, 8), 2, 4, device=DEV)
            # reads: word 5 is used before anything is written (0 on a zeroed workspace, 1 on NaN, 2 on +inf or on what is left behind)
            seen = torch.nan_to_num(ws[5], nan=1.0, posinf=2.0).clamp(0.0, 2.0) if reads else 0.0
            ws.copy_(dev(torch.arange(n, dtype=f32)))
            y.tensor[..., 2:6] = dev(x) + 1e-3 * seen + (1e-3 * calls[0] if drifts else 0.0)
            if overrun:
                torch.as_strided(ws, (n + 1,), (1,))[n] = 0.0      # one word behind the payload: the first word of the arena's guard
            if spills:
                y.tensor[1, 2, 6] = 0.0
            return [y]

        return Row(n, call, lambda got, what: np.testing.assert_allclose(got[0], x.numpy(), atol=0.1))

    good = stand_in()
    contract(good, good, what="well-behaved stand-in")
    with pytest.raises(AssertionError, match="behind the payload: words 1000 .. 1000 "):
        contract(stand_in(overrun=True), good, what="overrun")
    with pytest.raises(AssertionError, match="depends on the workspace's contents"):
        contract(stand_in(reads=True), good, what="reads before it writes")
    with pytest.raises(AssertionError, match="two calls on a zeroed workspace differ"):
        contract(stand_in(drifts=True), good, what="drifts")
    with pytest.raises(AssertionError, match="channel 6 of row 5 "):
        contract(stand_in(spills=True), good, what="spills")


# ---------------------------------------------------------------------------------------------------------------- bars
def max_bar(rel, abs_):
    """|got - ref| <= rel * max |ref| + abs_"""
    def check(got, ref, what):
        err, bar = float(np.abs(got - ref).max()), rel * float(np.abs(ref).max()) + abs_
        print("%s: max err %.3e, bar %.3e" % (what, err, bar))
        assert got.shape == ref.shape and err <= bar, (what, err, bar)
    return check


def elem_bar(rtol, atol):
    def check(got, ref, what):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=str(what))
    return check


F32_BAR = max_bar(1e-4, 2e-5)       # test_gpu_ops.py: the Winograd / auto-plan / three-term paths; test_gpu_bf16.py: the "exact" forward bar
CONV_BAR = elem_bar(1e-4, 2e-5)     # test_gpu_ops.py::test_conv2d_vs_torch_cpu (direct f32 forward, first layer)


def r16(t):
    return t.float().bfloat16().double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def dev(t):
    return t.to(DEV)


def tail_plan(ops, M, Cout, Cin, k, tile):
    tb, ts = ctypes.c_int(0), ctypes.c_int(1)
    ops.check(ops.lib().dim_conv2d_tail_plan(M, Cout, Cin, k, k, tile, ctypes.byref(tb), ctypes.byref(ts)))
    return tb.value, ts.value


# ---------------------------------------------------------------------------------------------------------------- direct forward
@functools.lru_cache(maxsize=None)
def conv_problem(shape, rounded=False):
    """x NHWC, w, b and the f64 reference NHWC of y = LeakyReLU_0.1(conv + b); rounded: operands rounded to bf16 first (the exact bar)"""
    N, H, W, Cin, Cout, k, s, p = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn((Cout,), generator=g) * 0.1
    xr, wr = (r16(x), r16(w)) if rounded else (x.double(), w.double())
    ref = nhwc(F.leaky_relu(F.conv2d(xr, wr, b.double(), stride=s, padding=p), 0.1)).numpy()
    ref.setflags(write=False)
    return nhwc(x), w, b, ref


def direct_fwd(ops, shape, tile, splits, two_phase=False, as_bf16=False, bar=CONV_BAR, branch=None):
    N, H, W, Cin, Cout, k, s, p = shape
    x, w, b, ref = conv_problem(shape, as_bf16)
    Ho, Wo = out_hw(H, W, k, s, p)
    need = ops.lib().dim_conv2d_workspace_floats(N, H, W, Cin, Cout, k, k, s, p, splits)
    assert (need > 0) == (splits != 1)

    def call(ws):
        y = ga.dense((N, Ho, Wo, Cout), device=DEV)
        wp = ops.conv2d_pack_weight(dev(w), as_bf16=as_bf16)
        ops.conv2d_fwd(dev(x), wp, dev(b), Cout, k, k, s, p, slope=0.1, splits=splits, tile=tile, out=y.tensor, workspace=ws,
                       events=[] if two_phase else None)   # events: dim_conv2d_fwd_partial + dim_splitk_reduce as two calls
        return [y]

    return Row(need, call, lambda got, what: bar(got[0], ref, what), branch)


@pytest.mark.parametrize("tile", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(1, 9, 11, 32, 64, 3, 1, 0), (1, 23, 31, 64, 128, 5, 2, 2)], ids=["9x11_k3", "23x31_k5s2"])
def test_direct_fwd_tiles(ops, shape, tile):
    """dim_conv2d_fwd, one launch, no workspace: the output's guards.  The 128 x 128 tiles (1, 4) need Cout % 128 == 0: on the 64-filter
    shape the entry refuses them before anything is enqueued, and the output keeps its sentinel"""
    from lib.hip.capi import DeepIMHipError

    if tile in (1, 4) and shape[4] % 128:
        N, H, W, Cin, Cout, k, s, p = shape
        x, w, b, _ = conv_problem(shape)
        y = ga.ChannelWindow((N,) + out_hw(H, W, k, s, p) + (Cout,), 0, 0, device=DEV)
        with pytest.raises(DeepIMHipError):
            ops.conv2d_fwd(dev(x), ops.conv2d_pack_weight(dev(w)), dev(b), Cout, k, k, s, p, slope=0.1, tile=tile, out=y.tensor)
        y.check("refused tile {} leaves the output alone".format(tile))
        return
    contract(direct_fwd(ops, shape, tile, 1), what="conv2d_fwd {} tile {}".format(shape, tile))


@pytest.mark.parametrize("two_phase", [False, True], ids=["fwd", "partial+reduce"])
def test_direct_fwd_split_k(ops, two_phase):
    """splits = 3 through workspace[3][M][Cout], as one call and as dim_conv2d_fwd_partial + dim_splitk_reduce"""
    shape, other = (2, 15, 20, 512, 512, 3, 1, 1), (1, 7, 9, 512, 512, 3, 1, 1)
    assert ops.lib().dim_conv2d_workspace_floats(2, 15, 20, 512, 512, 3, 3, 1, 1, 3) == 3 * 600 * 512
    contract(direct_fwd(ops, shape, 3, 3, two_phase), direct_fwd(ops, other, 3, 3, two_phase), what="conv2d_fwd split-K {}".format(shape))


def test_direct_fwd_auto_plan_tail(ops):
    """splits = 0: whole tiles per CU + a split-K tail through dim_conv2d_workspace_floats(..., 0).  The smallest shape with a tail on a
    256-CU device is 257 row tiles of the 64 x 64 kernel (1 x 64 x 257 pixels); where the device's CU count gives that shape no tail, the
    shape of test_gpu_ops.py::test_conv_auto_split_tail_vs_f64 is used.  Bar: that test's"""
    for shape in ((1, 64, 257, 32, 64, 3, 1, 1), (6, 96, 128, 32, 64, 3, 1, 1)):
        N, H, W, Cin, Cout, k, s, p = shape
        tb, ts = tail_plan(ops, N * H * W, Cout, Cin, k, 3)
        if ts >= 2 and tb > 0:
            break
    print("auto plan: shape {}, tail begins at tile {}, {} splits".format(shape, tb, ts))

    def branch():
        assert ts >= 2 and tb > 0, (shape, tb, ts)
        assert ops.conv_auto_plan(N * H * W, Cout, k * k * Cin // 32, Cin) == (3, 0)     # the default plan of this layer is "auto" on tile 3

    other = (1, 64, 300, 32, 64, 3, 1, 1)
    contract(direct_fwd(ops, shape, 3, 0, bar=F32_BAR, branch=branch), direct_fwd(ops, other, 3, 0, bar=F32_BAR),
             what="conv2d_fwd auto {}".format(shape))


@pytest.mark.parametrize("shape,tile", [((1, 37, 53), 2), ((1, 37, 53), 3), ((1, 37, 53), 6), ((3, 22, 18), 6)],
                         ids=["37x53_t2", "37x53_t3", "37x53_t6", "22x18_t6"])
def test_first_layer(ops, wino_split, shape, tile):
    """Cin 8, 7x7 / stride 2 / pad 3, 64 filters on the gathered-tap tiles and the LDS-halo kernel (tile 6), f32 and three-term pipe"""
    full = shape + (8, 64, 7, 2, 3)
    contract(direct_fwd(ops, full, tile, 1), what="first layer {} tile {} split {}".format(shape, tile, wino_split))


@pytest.mark.parametrize("tile", [3, 7, 9])
@pytest.mark.parametrize("shape", [(3, 9, 11, 96, 128, 3, 2, 1), (1, 16, 16, 32, 128, 3, 1, 1)], ids=["9x11_s2", "16x16_s1"])
def test_bf16_fwd_tiles(ops, shape, tile):
    """dim_conv2d_fwd_bf16 on the gathered-tap, LDS-halo and patch kernels; bar: the exact one of test_gpu_bf16.py::test_conv_fwd_bf16"""
    contract(direct_fwd(ops, shape, tile, 1, as_bf16=True, bar=F32_BAR), what="conv2d_fwd_bf16 {} tile {}".format(shape, tile))


# ---------------------------------------------------------------------------------------------------------------- Winograd forwards
WINO = {   # kind: (kernel, stride, pad, planes, output tile edge)
    "s1m2": (3, 1, 1, 16, 2), "s1m4": (3, 1, 1, 36, 4), "s2": (3, 2, 1, 81, 4), "5x5": (5, 2, 2, 36, 4)}


@functools.lru_cache(maxsize=None)
def wino_problem(kind, shape):
    k, s, p = WINO[kind][:3]
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape) + 29 + k + s)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) * (1.0 / np.sqrt(k * k * Cin))
    b = torch.randn((Cout,), generator=g) * 0.1
    ref = nhwc(F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p), 0.1)).numpy()
    ref.setflags(write=False)
    return nhwc(x), w, b, ref


def wino_rows_and_items(kind, shape, tile):
    """GEMM rows T and (tile, plane) items of the plane GEMMs of one un-sliced run"""
    k, s, p, planes, m = WINO[kind]
    N, H, W, Cin, Cout = shape
    Ho, Wo = out_hw(H, W, k, s, p)
    T = N * (-(-Ho // m)) * (-(-Wo // m))
    BM, BN = {3: (64, 64), 4: (128, 128)}[tile]
    return T, -(-T // BM) * (Cout // BN) * planes


def wino_fwd(ops, kind, shape, tile, branch=None):
    """the three forward Winograd entries into channels [32, 32 + Cout) of a (Cout + 64)-wide output, from an input with 32 pad channels"""
    N, H, W, Cin, Cout = shape
    x, w, b, ref = wino_problem(kind, shape)
    L = ops.lib()
    if kind in ("s1m2", "s1m4"):
        m = WINO[kind][4]
        need = L.dim_winograd_workspace_floats(N, H, W, Cin, Cout, m)
        pack, fwd = (lambda wd: ops.winograd_pack_weight(wd, m=m)), functools.partial(ops.conv2d_fwd_winograd, m=m)
    elif kind == "s2":
        need, pack, fwd = L.dim_winograd3x3s2_workspace_floats(N, H, W, Cin, Cout), ops.winograd3x3s2_pack_weight, ops.conv2d_fwd_winograd3x3s2
    else:
        need, pack, fwd = L.dim_winograd5x5s2_workspace_floats(N, H, W, Cin, Cout), ops.winograd5x5s2_pack_weight, ops.conv2d_fwd_winograd5x5s2

    def call(ws):
        assert ws.numel() == need
        xd = torch.zeros((N, H, W, Cin + 32), device=DEV)
        xd[..., :Cin] = dev(x)
        y = ga.ChannelWindow(ref.shape[:3] + (Cout + 64,), 32, Cout, device=DEV)
        fwd(xd, Cin, pack(dev(w)), dev(b), Cout, slope=0.1, tile=tile, out=y.tensor, out_coff=32, workspace=ws)
        return [y]

    return Row(need, call, lambda got, what: F32_BAR(got[0], ref, what), branch)


WINO_SMALL = [("s1m2", (1, 3, 5, 32, 64)), ("s1m2", (2, 7, 9, 32, 64)), ("s1m4", (1, 3, 5, 32, 64)), ("s1m4", (2, 7, 9, 32, 64)),
              ("s2", (1, 29, 37, 32, 64)), ("5x5", (1, 6, 9, 32, 128))]
WINO_OTHER = {"s1m2": (1, 6, 4, 32, 64), "s1m4": (1, 6, 4, 32, 64), "s2": (1, 12, 9, 32, 64), "5x5": (1, 9, 5, 32, 128)}


@pytest.mark.parametrize("kind,shape", WINO_SMALL, ids=["{}-{}".format(k, "x".join(map(str, s))) for k, s in WINO_SMALL])
def test_winograd_fwd(ops, wino_split, kind, shape):
    """3x3 / stride 1 (m = 2, 4), 3x3 / stride 2 and 5x5 / stride 2 on the 64 x 64 GEMM tile"""
    contract(wino_fwd(ops, kind, shape, 3), wino_fwd(ops, kind, WINO_OTHER[kind], 3), what="winograd {} {}".format(kind, shape))


# T = 162 GEMM rows each (two row tiles of 128, the second partly empty), Cout 128 on the 128 x 128 tile: 2 x planes items of K / 32
# chunks; K = 128 everywhere (four chunks per item; the planner's query wants K % 128 == 0): Cin 128 on the 3x3 paths, 4 Cin on 5x5
WINO_SHARED = [("s1m2", (2, 18, 18, 128, 128)), ("s1m4", (2, 36, 36, 128, 128)), ("s2", (2, 68, 68, 128, 128)), ("5x5", (2, 68, 68, 32, 128))]


@pytest.mark.parametrize("kind,shape", WINO_SHARED, ids=[k for k, _ in WINO_SHARED])
def test_winograd_fwd_shared_tiles(ops, wino_split, monkeypatch, kind, shape):
    """DIM_WINO_MAX_G=7: 7 stream-K ranges over 2 x planes items, so a range is several items long, range boundaries fall inside items
    and the M tile of such an item is shared by two workgroups (zeroed by the input transform's spare blocks, summed with atomics).
    G comes from the library: the 5x5 layer's item map, and for the 3x3 layers the planner of the plane GEMMs (wino_gemm_plan, which
    every plane count runs) asked through dim_wino_item_map_plan at this T, K, Cout and tile.  That query counts items for 36 planes;
    the item count of the 16- and 81-plane layers is row tiles x column tiles x planes, computed here.  Where no block is skipped the
    chunk list is items x K / 32 long and range w starts at chunk w per + min(w, rem) (wg_first_chunk): a start that is no multiple
    of K / 32 lies inside an item"""
    monkeypatch.setenv("DIM_WINO_MAX_G", "7")
    tile = 4
    T, items = wino_rows_and_items(kind, shape, tile)
    N, H, W, Cin, Cout = shape

    def branch():
        assert T == 162 and items == 2 * WINO[kind][3] > 7
        if kind == "5x5":
            hdr, _ = ops.wino_item_map_create(N, H, W, Cin, Cout, tile).query()
            print(kind, hdr)
            assert (hdr["T"], hdr["G"], hdr["items"], hdr["nch"]) == (162, 7, items, 4), hdr
            assert hdr["per"] > hdr["nch"]                                    # ranges longer than any item
            return
        hdr, _ = ops.wino_item_map_plan(T, Cin, Cout, tile, G=0, skip5=False)
        print(kind, hdr)
        assert (hdr["T"], hdr["G"], hdr["nch"]) == (162, 7, 4), hdr
        if kind == "s1m4":
            assert hdr["items"] == items
        per, rem = divmod(items * hdr["nch"], hdr["G"])
        starts = [w * per + min(w, rem) for w in range(1, hdr["G"])]
        inside = [c for c in starts if c % hdr["nch"]]
        print(kind, "range starts", starts, "inside an item:", inside)
        assert per > hdr["nch"] and len(inside) >= 3

    other = {"s1m2": (1, 9, 9, 128, 128), "s1m4": (1, 18, 18, 128, 128), "s2": (1, 34, 34, 128, 128), "5x5": (1, 34, 34, 32, 128)}[kind]
    contract(wino_fwd(ops, kind, shape, tile, branch), wino_fwd(ops, kind, other, tile), what="winograd {} {} MAX_G 7".format(kind, shape))


@pytest.mark.parametrize("kind,shape", [("s1m4", (3, 7, 9, 32, 64)), ("s1m2", (3, 7, 9, 32, 64)), ("s2", (3, 29, 37, 32, 64)), ("5x5", (3, 6, 9, 32, 128))],
                         ids=["s1m4", "s1m2", "s2", "5x5"])
def test_winograd_fwd_second_slice_reuses_the_workspace(ops, wino_split, monkeypatch, kind, shape):
    """DIM_WINO_MAX_SLICE=2: 3 images run as 2 + 1 through one workspace sized for the whole batch; the second slice finds the first
    one's V and M there (and, on the stale fill, another shape's)"""
    monkeypatch.setenv("DIM_WINO_MAX_SLICE", "2")
    assert shape[0] > 2                                             # the branch: more images than a slice holds
    contract(wino_fwd(ops, kind, shape, 3), wino_fwd(ops, kind, WINO_OTHER[kind], 3), what="winograd {} {} MAX_SLICE 2".format(kind, shape))


# ---------------------------------------------------------------------------------------------------------------- Winograd gradients
@functools.lru_cache(maxsize=None)
def dgrad_problem(shape, k, s, p, rounded=False):
    """w (Cout,Cin,k,k), dy NHWC and the f64 input gradient NHWC of conv(x, w, stride s, pad p)"""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape) + 13 + k)
    w = torch.randn((Cout, Cin, k, k), generator=g) * (1.0 / np.sqrt(k * k * Cout))
    Ho, Wo = out_hw(H, W, k, s, p)
    dy = torch.randn((N, Cout, Ho, Wo), generator=g)
    wr, dyr = (r16(w), r16(dy)) if rounded else (w.double(), dy.double())
    ref = nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), wr, dyr, stride=s, padding=p)).numpy()
    ref.setflags(write=False)
    return w, nhwc(dy), ref


def wino5_dgrad(ops, shape):
    N, H, W, Cin, Cout = shape
    w, dy, ref = dgrad_problem(shape, 5, 2, 2)
    need = ops.lib().dim_winograd5x5s2_workspace_floats(N, H, W, Cin, Cout)

    def call(ws):
        dyd = torch.zeros(dy.shape[:3] + (Cout + 32,), device=DEV)
        dyd[..., :Cout] = dev(dy)
        dx = ga.ChannelWindow((N, H, W, Cin + 8), 0, Cin, device=DEV)
        ops.conv2d_dgrad_winograd5x5s2(dyd, Cout, ops.winograd5x5s2_dgrad_pack_weight(dev(w)), dx.tensor, Cin, workspace=ws)
        return [dx]

    return Row(need, call, lambda got, what: F32_BAR(got[0], ref, what))


@pytest.mark.parametrize("shape", [(1, 7, 10, 16, 32), (1, 15, 21, 32, 64)], ids=["7x10", "15x21"])
def test_winograd5x5s2_dgrad(ops, wino_split, shape):
    """dim_conv2d_dgrad_winograd5x5s2 into channels [0, Cin) of a (Cin + 8)-wide dx; bar: test_conv5x5s2_winograd_dgrad_vs_f64's"""
    contract(wino5_dgrad(ops, shape), wino5_dgrad(ops, (1, 9, 6, shape[3], shape[4])), what="winograd5x5s2 dgrad {}".format(shape))


def wino3_dgrad(ops, shape, m):
    """the 3x3 / stride-1 input gradient as deepim/core/module.py runs it: the forward entry on dy with dim_winograd_dgrad_pack_weight's
    weights, no bias, slope 1, Cout input and Cin output channels"""
    N, H, W, Cin, Cout = shape
    w, dy, ref = dgrad_problem(shape, 3, 1, 1)
    need = ops.lib().dim_winograd_workspace_floats(N, H, W, Cout, Cin, m)

    def call(ws):
        dx = ga.dense((N, H, W, Cin), device=DEV)
        ops.conv2d_fwd_winograd(dev(dy), Cout, ops.winograd_dgrad_pack_weight(dev(w), m=m), None, Cin, slope=1.0, tile=3, out=dx.tensor,
                                workspace=ws, m=m)
        return [dx]

    return Row(need, call, lambda got, what: F32_BAR(got[0], ref, what))


@pytest.mark.parametrize("m", [2, 4])
def test_winograd3x3_dgrad_through_the_forward_entry(ops, wino_split, m):
    shape = (2, 7, 9, 64, 32)
    contract(wino3_dgrad(ops, shape, m), wino3_dgrad(ops, (1, 6, 4, 64, 32), m), what="winograd 3x3 dgrad m {} {}".format(m, shape))


@functools.lru_cache(maxsize=None)
def wino_wgrad_problem(shape):
    N, H, W, Cin, Cout, S = shape
    k, pad = (3, 1) if S == 1 else (5, 2)
    g = torch.Generator().manual_seed(sum(shape) + 17)
    x = torch.randn((N, Cin, H, W), generator=g)
    Ho, Wo = out_hw(H, W, k, S, pad)
    dy = torch.randn((N, Cout, Ho, Wo), generator=g) / np.sqrt(N * Ho * Wo)
    ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, k, k), dy.double(), stride=S, padding=pad).numpy()
    ref.setflags(write=False)
    return nhwc(x), nhwc(dy), ref


def wino_wgrad(ops, shape, splits, accumulate):
    """accumulate: dw starts as float32(ref) and the call adds 0.5 times the gradient: 1.5 ref within twice the bar, the accumulate step
    of test_gpu_ops.py::test_conv_winograd_wgrad_vs_f64 (whose bar, 1e-4 max|ref| + 2e-6, this row uses)"""
    N, H, W, Cin, Cout, S = shape
    x, dy, ref = wino_wgrad_problem(shape)
    need = ops.lib().dim_conv2d_wgrad_winograd_workspace_floats(N, H, W, Cin, Cout, S, splits)
    tol = 1e-4 * np.abs(ref).max() + 2e-6

    def call(ws):
        xd = torch.zeros((N, H, W, Cin + 32), device=DEV)
        xd[..., :Cin] = dev(x)
        dyd = torch.zeros(dy.shape[:3] + (Cout + 64,), device=DEV)
        dyd[..., :Cout] = dev(dy)
        dw = ga.dense(ref.shape, device=DEV)
        if accumulate:
            dw.tensor.copy_(torch.from_numpy(ref.astype(np.float32)))
            ops.conv2d_wgrad_winograd(xd, Cin, dyd, Cout, dw.tensor, S=S, splits=splits, workspace=ws, scale=0.5, accumulate=True)
        else:
            ops.conv2d_wgrad_winograd(xd, Cin, dyd, Cout, dw.tensor, S=S, splits=splits, workspace=ws)
        return [dw]

    def verify(got, what):
        err = np.abs(got[0] - (1.5 if accumulate else 1.0) * ref).max()
        print("%s: max err %.3e, bar %.3e" % (what, err, (2 if accumulate else 1) * tol))
        assert err <= (2 if accumulate else 1) * tol, (what, err, tol)

    return Row(need, call, verify)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("shape", [(1, 15, 21, 64, 64, 1), (2, 30, 40, 32, 64, 2)], ids=["S1", "S2"])
def test_winograd_wgrad(ops, shape, splits, accumulate):
    other = (1, 9, 13) + shape[3:]
    contract(wino_wgrad(ops, shape, splits, accumulate), wino_wgrad(ops, other, splits, accumulate),
             what="winograd wgrad {} splits {} accumulate {}".format(shape, splits, accumulate))


# ---------------------------------------------------------------------------------------------------------------- direct weight gradients
@functools.lru_cache(maxsize=None)
def wgrad_problem(shape, rounded):
    N, H, W, Cin, Cout, k, s, p = shape
    g = torch.Generator().manual_seed(sum(shape) + 3)
    x = torch.randn((N, Cin, H, W), generator=g)
    Ho, Wo = out_hw(H, W, k, s, p)
    dy = torch.randn((N, Cout, Ho, Wo), generator=g)
    xr, dyr = (r16(x), r16(dy)) if rounded else (x.double(), dy.double())
    ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, k, k), dyr, stride=s, padding=p)
    return nhwc(x), nhwc(dy), ref


def packed_floats(Cin, Cout, k):
    """the packed f32 weights dim_conv2d_wgrad writes: chunks of 32 x Cout (behind them a first-layer buffer holds the three-term image)"""
    return (-(-k * k // 4) if Cin == 8 else k * k * (Cin // 32)) * 32 * Cout


def packed_reference(w):
    """the packed layout restated with torch indexing, independent of the library's packer: [chunk][Cout][32], a chunk = (32-channel
    slice, kh, kw) for Cin % 32 == 0 (as tests/test_gpu_bf16.py restates it); for Cin 8 a chunk = 4 taps x 8 channels, the taps flat
    over kh x kw and the last chunk padded with zero taps"""
    cout, cin, kh, kw = w.shape
    if cin == 8:
        taps = -(-kh * kw // 4) * 4
        wt = torch.zeros((cout, taps, 8), dtype=w.dtype)
        wt[:, :kh * kw] = w.reshape(cout, 8, kh * kw).permute(0, 2, 1)
        return wt.reshape(cout, taps // 4, 32).permute(1, 0, 2).reshape(-1)
    return w.reshape(cout, cin // 32, 32, kh * kw).permute(1, 3, 0, 2).reshape(-1)


def direct_wgrad(ops, shape, splits, as_bf16, oihw, slabs=None):
    """dim_conv2d_wgrad[_bf16] (packed layout, dz = channels [4, 4 + Cout) of a wider row) and dim_conv2d_wgrad_oihw, whose workspace is
    workspace_floats(splits + 1) also for one split.  Bars: f32 3e-5 max|dW| + 1e-5 (test_gpu_backward.py), bf16 the exact bar 1e-4
    max|dW| + 1e-5 on bf16-rounded operands (test_gpu_bf16.py).
    slabs: how many leading slabs of the workspace the call is meant to use -- after the call on the NaN fill exactly those hold
    numbers in every word and every other word is still NaN: the library's own account of its split count (clamped or not) and of
    whether dim_conv2d_wgrad_oihw took the slab behind the last one for its lane-parallel sum"""
    N, H, W, Cin, Cout, k, s, p = shape
    x, dy, ref = wgrad_problem(shape, as_bf16)
    L = ops.lib()
    need = L.dim_conv2d_wgrad_workspace_floats(Cout, Cin, k, k, splits + 1 if oihw else splits)
    assert need == (packed_floats(Cin, Cout, k) * (splits + 1 if oihw else splits if splits > 1 else 0))
    scale = ref.abs().max().item()
    tol = (1e-4 if as_bf16 else 3e-5) * scale + 1e-5
    n = packed_floats(Cin, Cout, k)

    def call(ws):
        dz = torch.full(dy.shape[:3] + (Cout + 8,), float("nan"), device=DEV)
        dz[..., 4:4 + Cout] = dev(dy)
        if oihw:
            dw = ga.dense((Cout, Cin, k, k), device=DEV)
            ops.conv2d_wgrad_oihw(dev(x), Cin, dz, Cout, k, k, s, p, dw.tensor, splits=splits, dz_coff=4, workspace=ws, bf16_mfma=as_bf16)
        else:
            dw = ga.dense((n,), device=DEV)
            ops.conv2d_wgrad(dev(x), Cin, dz, Cout, k, k, s, p, dw.tensor, splits=splits, dz_coff=4, workspace=ws, bf16_mfma=as_bf16)
        return [dw]

    def verify(got, what):
        want = ref.numpy() if oihw else packed_reference(ref).numpy()
        assert want.size == got[0].size
        err = np.abs(got[0] - want).max()
        print("%s: max err %.3e, bar %.3e" % (what, err, tol))
        assert err <= tol, (what, err, tol)

    def inspect(ws):
        rows = ws.view(-1, n)
        numbers = ~torch.isnan(rows)
        full, untouched = numbers.all(1).cpu().numpy(), (~numbers.any(1)).cpu().numpy()
        print("wgrad {} splits {}: slabs written {}".format(shape, splits, np.nonzero(full)[0].tolist()))
        assert full[:slabs].all() and untouched[slabs:].all(), (slabs, full.tolist(), untouched.tolist())

    return Row(need, call, verify, inspect=inspect if (slabs and need) else None)


WG_SHAPE = (3, 13, 9, 32, 64, 3, 1, 1)


@pytest.mark.parametrize("oihw", [False, True], ids=["packed", "oihw"])
@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("splits", [1, 2, 100])
def test_direct_wgrad(ops, splits, as_bf16, oihw):
    """351 pixels = 11 steps of 32: 100 splits are clamped to 11 (slabs of one step), inside a workspace sized for 100 (+ 1): the
    workspace shows 11 slabs written (1 and 2 for the other counts; the slab behind them is not touched with so few)"""
    other = (1, 6, 7) + WG_SHAPE[3:]
    contract(direct_wgrad(ops, WG_SHAPE, splits, as_bf16, oihw, slabs=min(splits, 11)), direct_wgrad(ops, other, max(splits, 2), as_bf16, oihw),
             what="wgrad {} splits {} bf16 {} oihw {}".format(WG_SHAPE, splits, as_bf16, oihw))


@pytest.mark.parametrize("oihw", [False, True], ids=["packed", "oihw"])
@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
def test_direct_wgrad_first_layer(ops, as_bf16, oihw):
    """Cin 8, 7x7 / stride 2 / pad 3, 4 splits: slabs of 13 chunks x 32 x 64 floats"""
    shape, other = (2, 33, 41, 8, 64, 7, 2, 3), (1, 20, 17, 8, 64, 7, 2, 3)
    contract(direct_wgrad(ops, shape, 4, as_bf16, oihw, slabs=4), direct_wgrad(ops, other, 4, as_bf16, oihw),
             what="wgrad first layer splits 4 bf16 {} oihw {}".format(as_bf16, oihw))


@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
def test_direct_wgrad_oihw_many_small_slabs(ops, as_bf16):
    """2048 pixels = 64 steps in 64 splits: with >= 64 slabs of fewer than 2^18 floats dim_conv2d_wgrad_oihw sums them with the
    lane-parallel reduce into the slab behind the last one -- the 65th of workspace_floats(splits + 1), which the workspace shows
    written -- and converts that"""
    shape, other = (2, 32, 32, 32, 64, 3, 1, 1), (1, 40, 52, 32, 64, 3, 1, 1)
    assert packed_floats(32, 64, 3) // 4 < 65536
    contract(direct_wgrad(ops, shape, 64, as_bf16, True, slabs=65), direct_wgrad(ops, other, 64, as_bf16, True),
             what="wgrad_oihw 64 slabs bf16 {}".format(as_bf16))


@pytest.mark.parametrize("shape", [WG_SHAPE, (2, 36, 44, 64, 128, 3, 1, 1)], ids=["gathered", "patch"])
@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
def test_direct_wgrad_refuses_accumulate_with_splits(ops, as_bf16, shape):
    """accumulate with more than one split is refused (the slab sum would replace dw, not add to it) before anything is enqueued: the
    workspace keeps every NaN word and dw its sentinel.  One split may accumulate (not in the bf16 patch form)"""
    from lib.hip.capi import DeepIMHipError

    N, H, W, Cin, Cout, k, s, p = shape
    x, dy, ref = wgrad_problem(shape, as_bf16)
    n = packed_floats(Cin, Cout, k)
    ws = ga.GuardArena(ops.lib().dim_conv2d_wgrad_workspace_floats(Cout, Cin, k, k, 2), device=DEV)
    dw = ga.ChannelWindow((n,), 0, 0, device=DEV)
    with pytest.raises(DeepIMHipError, match="accumulate"):
        ops.conv2d_wgrad(dev(x), Cin, dev(dy), Cout, k, k, s, p, dw.tensor, splits=2, workspace=ws.view(), accumulate=True, bf16_mfma=as_bf16)
    ws.check("refused wgrad")
    dw.check("refused wgrad")
    assert bool(torch.isnan(ws.view()).all())
    if as_bf16 and Cout % 128 == 0:
        return
    acc = ga.dense((n,), device=DEV)
    acc.tensor.copy_(packed_reference(ref).float())
    ops.conv2d_wgrad(dev(x), Cin, dev(dy), Cout, k, k, s, p, acc.tensor, splits=1, accumulate=True, bf16_mfma=as_bf16)
    acc.check("accumulating wgrad")
    tol = (1e-4 if as_bf16 else 3e-5) * ref.abs().max().item() + 1e-5
    assert np.abs(acc.inside() - 2 * packed_reference(ref).numpy()).max() <= 2 * tol


@pytest.mark.parametrize("oihw", [False, True], ids=["packed", "oihw"])
def test_direct_wgrad_bf16_patch_form(ops, oihw):
    """3x3 / stride 1, 3168 pixels, Cout % 128 == 0: the bf16 patch form (8 x 8 pixel blocks: 2 x 5 x 6 = 60 blocks in 7 splits of 9, 9, ...).
    The branch: dim_conv2d_wgrad_bf16_splits plans this shape by the patch form's rule (2 tiles, 60 blocks, 2 workgroups per CU: 15
    splits on 256 CUs; the gathered form's rule would give 24), and the workspace shows 7 slabs written"""
    shape, other = (2, 36, 44, 64, 128, 3, 1, 1), (1, 36, 40, 64, 128, 3, 1, 1)
    assert ops.lib().dim_conv2d_wgrad_bf16_splits(2, 36, 44, 64, 128, 3, 3, 1, 1, 256) == 15
    contract(direct_wgrad(ops, shape, 7, True, oihw, slabs=7), direct_wgrad(ops, other, 7, True, oihw), what="wgrad patch form splits 7 oihw {}".format(oihw))


# ---------------------------------------------------------------------------------------------------------------- bf16 input gradients
def test_dgrad_bf16_splitk(ops):
    """dim_conv2d_dgrad_bf16_splitk, 2 K ranges through 2 copies of dx, into channels [0, 128) of a 192-wide dx; bar: the exact one of
    test_gpu_bf16.py::test_dgrad_wgrad_bf16"""
    def row(shape):
        N, H, W, Cin, Cout = shape
        w, dy, ref = dgrad_problem(shape, 3, 2, 1, rounded=True)
        cs = ops.pad64(Cin) + 64
        need = ops.lib().dim_conv2d_dgrad_splitk_workspace_floats(N, H, W, cs, 2)
        bar = max_bar(1e-4, 1e-5)

        def call(ws):
            dx = ga.ChannelWindow((N, H, W, cs), 0, ops.pad64(Cin), device=DEV)
            wd = ops.conv2d_dgrad_pack_weight(dev(w), 2, 1, as_bf16=True)
            ops.conv2d_dgrad(dev(dy), Cout, wd, dx.tensor, Cin, 3, 3, 2, 1, accumulate=False, tile=3, splits=2, workspace=ws)
            return [dx]

        return Row(need, call, lambda got, what: bar(got[0][..., :Cin], ref, what))

    contract(row((2, 9, 11, 128, 64)), row((1, 5, 6, 128, 64)), what="dgrad_bf16_splitk")


def test_dgrad_bf16_lrelu(ops):
    """dim_conv2d_dgrad_bf16_lrelu: dz and db; bars of test_gpu_bf16.py::test_dgrad_with_lrelu_and_bias_gradient_folded_in"""
    def row(shape):
        N, H, W, Cin, Cout = shape
        w, dy, dx_ref = dgrad_problem(shape, 3, 1, 1, rounded=True)
        g = torch.Generator().manual_seed(sum(shape))
        y_act = torch.randn((N, H, W, Cin), generator=g)
        y_act[0, :2, :3, :] = 0.0
        dz_ref = dx_ref * np.where(y_act.double().numpy() > 0, 1.0, 0.1)
        db_ref = dz_ref.sum((0, 1, 2))
        need = ops.lib().dim_conv2d_dgrad_lrelu_workspace_floats(N, H, W, Cin, 1)
        dz_bar, db_bar = max_bar(1e-4, 1e-5), max_bar(1e-4, 1e-3)

        def call(ws):
            dz, db = ga.dense((N, H, W, Cin), device=DEV), ga.dense((Cin,), device=DEV)
            wd = ops.conv2d_dgrad_pack_weight(dev(w), 1, 1, as_bf16=True)
            ops.conv2d_dgrad_lrelu(dev(dy), Cout, wd, dz.tensor, dev(y_act), Cin, 3, 3, 1, 1, db.tensor, workspace=ws)
            return [dz, db]

        def verify(got, what):
            dz_bar(got[0], dz_ref, what + " dz")
            db_bar(got[1], db_ref, what + " db")

        return Row(need, call, verify)

    contract(row((1, 37, 53, 128, 128)), row((1, 20, 17, 128, 128)), what="dgrad_bf16_lrelu")


# ---------------------------------------------------------------------------------------------------------------- column sums
COLSUM_M = (1, 63, 512, 513, 4097)


def colsum_data(M, cols, seed):
    """multiples of 1/8 in [-1, 1]: every partial sum of up to 4097 of them (and of their halves) is exact in float32, so the f64 column
    sum is the expected value bit for bit in any summation order, and a row block that is dropped, counted twice or left over from
    another call moves a sum by at least 1/16"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, cols), generator=g).float() / 8


def bias_grad_row(ops, M, C, coff):
    cs = C + 8
    dz = colsum_data(M, cs, 7 * M + C + coff)
    ref = dz[:, coff:coff + C].double().sum(0).numpy()
    need = ops.lib().dim_bias_grad_workspace_floats(M, C)
    bar = elem_bar(1e-4, 1e-4)          # test_gpu_backward.py::test_dgrad_wgrad_bias_vs_autograd

    def call(ws):
        db = ga.dense((C,), device=DEV)
        ops.bias_grad(dev(dz).view(1, 1, M, cs), C, db.tensor, dz_coff=coff, workspace=ws)
        return [db]

    return Row(need, call, lambda got, what: bar(got[0], ref, what))


def lrelu_bias_grad_row(ops, M, C, coff):
    """slope 0.5 keeps every product exact; dy is read and written in place inside its window of a wider row"""
    cs = C + 8
    dy, y = colsum_data(M, cs, 11 * M + C + coff), colsum_data(M, cs, 13 * M + C + coff + 1)
    ref_dy = (dy[:, coff:coff + C] * torch.where(y[:, 4:4 + C] > 0, 1.0, 0.5)).double()
    ref_db = ref_dy.sum(0).numpy()
    need = ops.lib().dim_lrelu_bwd_bias_grad_workspace_floats(M, C)
    dy_bar, db_bar = elem_bar(1e-6, 0), elem_bar(2e-5, 2e-4)   # test_gpu_backward.py::test_lrelu_bwd_bias_grad_fused

    def call(ws):
        db = ga.dense((C,), device=DEV)
        d = ga.ChannelWindow((1, 1, M, cs), coff, C, device=DEV)
        d.tensor[..., coff:coff + C] = dev(dy[:, coff:coff + C])
        ops.lrelu_bwd_bias_grad(dev(y).view(1, 1, M, cs), d.tensor, C, db.tensor, slope=0.5, y_coff=4, dy_coff=coff, workspace=ws)
        return [db, d]

    def verify(got, what):
        db_bar(got[0], ref_db, what + " db")
        dy_bar(got[1].reshape(M, C), ref_dy.numpy(), what + " dy")

    return Row(need, call, verify)


@pytest.mark.parametrize("coff", [0, 4])
@pytest.mark.parametrize("C", [4, 64, 68, 132])
@pytest.mark.parametrize("entry", ["bias_grad", "lrelu_bwd_bias_grad"])
def test_column_sums(ops, entry, C, coff):
    """dim_bias_grad / dim_lrelu_bwd_bias_grad on 1 .. 4097 rows (below, at and above one row block of 512 / 64) of a window of a wider
    row, through a workspace of exactly the reported size: deepim/core/module.py sizes its bias workspace by these functions alone"""
    make = bias_grad_row if entry == "bias_grad" else lrelu_bias_grad_row
    for M in COLSUM_M:
        contract(make(ops, M, C, coff), make(ops, 700, C, coff), what="{} M {} C {} coff {}".format(entry, M, C, coff))


# ---------------------------------------------------------------------------------------------------------------- FC
@functools.lru_cache(maxsize=None)
def fc_weights(C, H, W, Out):
    g = torch.Generator().manual_seed(C + H + W + Out)
    w = torch.randn((Out, C * H * W), generator=g) * 0.01
    b = torch.randn((Out,), generator=g) * 0.1
    return w, b


@functools.lru_cache(maxsize=None)
def fc_problem(B, C, H, W, Out):
    w, b = fc_weights(C, H, W, Out)
    g = torch.Generator().manual_seed(40 + B)
    feat = torch.randn((B, C, H, W), generator=g)
    ref = F.leaky_relu(feat.double().reshape(B, -1) @ w.double().t() + b.double(), 0.1).numpy()
    return nhwc(feat), ref


def fc_row(ops, B, C, H, W, Out, packed):
    x, ref = fc_problem(B, C, H, W, Out)
    _, b = fc_weights(C, H, W, Out)
    need = ops.lib().dim_fc_fwd_workspace_floats(C, H, W, Out)
    bar = elem_bar(1e-4, 5e-5)          # test_gpu_ops.py::test_fc_stream_vs_f64_and_conv_path

    def call(ws):
        y = ga.dense((B, Out), device=DEV)
        ops.fc_fwd(dev(x), packed, dev(b), Out, slope=0.1, out=y.tensor, workspace=ws)
        return [y]

    return Row(need, call, lambda got, what: bar(got[0], ref, what))


@pytest.mark.parametrize("geom", [(64, 1, 1, 256), (256, 8, 10, 1024)], ids=["64x1x1_256", "256x8x10_1024"])
def test_fc_fwd(ops, geom):
    """dim_fc_fwd with 1, 3, 16 and 17 rows (one pass of 32 rows, partly filled); the stale workspace comes from another batch"""
    C, H, W, Out = geom
    packed = ops.fc_pack_weight(dev(fc_weights(*geom)[0]), C, H, W)
    for B in (1, 3, 16, 17):
        contract(fc_row(ops, B, C, H, W, Out, packed), fc_row(ops, 5, C, H, W, Out, packed), what="fc_fwd B {} {}".format(B, geom))


def test_fc_fwd_refuses_an_output_count_it_has_no_kernel_for(ops):
    """Out = 48 (not a multiple of 256) is refused before anything is enqueued: workspace and output keep their fills"""
    from lib.hip.capi import DeepIMHipError

    C, H, W, Out, B = 64, 1, 1, 48, 3
    ws, y = ga.GuardArena(max(ops.lib().dim_fc_fwd_workspace_floats(C, H, W, Out), 64), device=DEV), ga.ChannelWindow((B, Out), 0, 0, device=DEV)
    with pytest.raises(DeepIMHipError):
        ops.fc_fwd(torch.zeros((B, H, W, C), device=DEV), torch.zeros((Out * C,), device=DEV), torch.zeros((Out,), device=DEV), Out, out=y.tensor,
                   workspace=ws.view())
    ws.check("refused fc_fwd")
    y.check("refused fc_fwd")
    assert bool(torch.isnan(ws.view()).all())


@pytest.mark.parametrize("shape", [(3, 48, 64, 1, 1), (17, 256, 64, 8, 10)], ids=["3x48", "17x256"])
def test_fc_wgrad_nhwc(ops, shape):
    """dim_fc_wgrad_nhwc takes no workspace: its output's guards; bar of test_gpu_ops.py's test of the entry"""
    B, Out, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((B, C, H, W), generator=g)
    dz = torch.randn((B, Out), generator=g)
    ref = (dz.double().t() @ x.double().reshape(B, -1)).numpy()
    bar = max_bar(1e-5, 1e-6)

    def call(ws):
        dW = ga.dense((Out, C * H * W), device=DEV)
        ops.fc_wgrad_nhwc(dev(dz), dev(nhwc(x)), dW.tensor)
        return [dW]

    contract(Row(0, call, lambda got, what: bar(got[0], ref, what)), what="fc_wgrad_nhwc {}".format(shape))


# ---------------------------------------------------------------------------------------------------------------- heads
@pytest.mark.parametrize("shape", [(2, 30, 40, 6, 8, 2), (2, 9, 11, 770, 800, 2)], ids=["cin6", "cin770"])
def test_conv_small_cout(ops, shape):
    """dim_conv_small_cout_fwd into channels [4, 4 + Cout) of an 8-wide output and dim_conv_small_cout_bwd (dx into [0, Cin) of the
    concat-gradient row, through its workspace); bars of test_gpu_decoder.py / test_gpu_backward.py::test_conv_small_cout_backward"""
    def rows(shp):
        N, H, W, Cin, cs, Cout = shp
        g = torch.Generator().manual_seed(sum(shp))
        x = torch.randn((N, Cin, H, W), generator=g, dtype=torch.float64, requires_grad=True)
        w = (torch.randn((Cout, Cin, 3, 3), generator=g, dtype=torch.float64) / np.sqrt(9 * Cin)).requires_grad_()
        b = (torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
        y = F.conv2d(x, w, b, padding=1)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        y_ref = nhwc(y.detach()).numpy()
        xb = torch.zeros((N, H, W, cs))
        xb[..., :Cin] = nhwc(x.detach().float())
        fwd_bar = elem_bar(1e-4, 2e-5)

        xf = torch.zeros((N, H, W, max(cs, ops.pad32(Cin))))      # the forward wants the row to cover Cin rounded up to 32
        xf[..., :cs] = xb

        def fwd(ws):
            out = ga.ChannelWindow((N, H, W, 8), 4, Cout, device=DEV)
            ops.conv_small_cout_fwd(dev(xf), Cin, ops.conv_small_cout_pack_weight(dev(w.detach().float())), dev(b.detach().float()), Cout,
                                    out=out.tensor, out_coff=4)
            return [out]

        need = ops.lib().dim_conv_small_cout_bwd_workspace_floats(N, H, W, Cin, Cout, 3, 3)
        wmax = w.grad.abs().max().item()

        def bwd(ws):
            dx = ga.ChannelWindow((N, H, W, cs), 0, Cin, device=DEV)
            dw, db = ga.dense((Cout, Cin, 3, 3), device=DEV), ga.dense((Cout,), device=DEV)
            ops.conv_small_cout_bwd(dev(xb), Cin, dev(nhwc(dy.float())), dev(w.detach().float()), dx.tensor, dw.tensor, db.tensor,
                                    accumulate_dx=False, workspace=ws)
            return [dx, dw, db]

        def verify(got, what):
            elem_bar(1e-4, 2e-5)(got[0], nhwc(x.grad).numpy(), what + " dx")
            elem_bar(1e-4, 2e-5 * wmax)(got[1], w.grad.numpy(), what + " dw")
            elem_bar(1e-4, 1e-4)(got[2], b.grad.numpy(), what + " db")

        return Row(0, fwd, lambda got, what: fwd_bar(got[0], y_ref, what)), Row(need, bwd, verify)

    N, H, W, Cin, cs, Cout = shape
    fwd, bwd = rows(shape)
    _, stale = rows((1, 7, 6, Cin, cs, Cout))
    contract(fwd, what="conv_small_cout_fwd {}".format(shape))
    contract(bwd, stale, what="conv_small_cout_bwd {}".format(shape))


@pytest.mark.parametrize("as_bf16", [False, True], ids=["f32", "bf16"])
def test_deconv4x4s2_fwd_into_a_concat_buffer(ops, as_bf16):
    """dim_deconv4x4s2_fwd[_bf16], 32 -> 64 channels, 5 x 7 -> 11 x 15, into channels [8, 72) of a 104-wide row, as the decoder writes its
    concat buffers; bar of test_gpu_bf16.py::test_deconv4x4s2_bf16_forward_and_backward (f32: the same bar on unrounded operands)"""
    N, Cin, H, W, Cout, OH, OW = 2, 32, 5, 7, 64, 11, 15
    g = torch.Generator().manual_seed(N + Cin + H + W + Cout + OH + OW)
    x = torch.randn((N, Cin, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Cin, Cout, 4, 4), generator=g, dtype=torch.float64) / np.sqrt(Cin * 4)
    b = torch.randn((Cout,), generator=g, dtype=torch.float64)
    xr, wr = (r16(x), r16(w)) if as_bf16 else (x, w)
    ref = nhwc(F.leaky_relu(F.conv_transpose2d(xr, wr, b, stride=2)[:, :, 1:1 + OH, 1:1 + OW], 0.1)).numpy()

    def call(ws):
        y = ga.ChannelWindow((N, OH, OW, Cout + 40), 8, Cout, device=DEV)
        ops.deconv4x4s2_fwd(dev(nhwc(x.float())), Cin, ops.deconv4x4s2_pack_weight(dev(w.float()), as_bf16=as_bf16), dev(b.float()), y.tensor, Cout,
                            crop=1, slope=0.1, out_coff=8)
        return [y]

    contract(Row(0, call, lambda got, what: F32_BAR(got[0], ref, what)), what="deconv4x4s2_fwd bf16 {}".format(as_bf16))


@pytest.mark.parametrize("shape", [(2, 8, 10, 2, 2, 15, 20), (1, 3, 5, 1, 4, 5, 9)], ids=["2to2", "1to4"])
def test_deconv4x4s2_tiny_bwd(ops, shape):
    """dim_deconv4x4s2_tiny_bwd (no workspace): dx, dW and db in guarded buffers, dy read from channels [66, 66 + Cout) of a 70-wide
    row; inputs, reference and per-element bars of tests/train_head_reference.py, as test_gpu_train_head.py uses them"""
    import train_head_reference as R

    N, H, W, Cin, Cout, OH, OW = shape
    inp = R.deconv_inputs(*shape)
    ref = R.deconv4x4s2_tiny_bwd(inp["x"], inp["dy"], inp["w"], OH, OW)

    def call(ws):
        dx, dw, db = ga.dense((N, H, W, Cin), device=DEV), ga.dense((Cin, Cout, 4, 4), device=DEV), ga.dense((Cout,), device=DEV)
        ops.deconv4x4s2_tiny_bwd(dev(torch.from_numpy(inp["x_wide"])), dev(torch.from_numpy(inp["dy_wide"])), R.DECONV_DY_COFF,
                                 dev(torch.from_numpy(inp["w"])), dx.tensor, dw.tensor, db.tensor, crop=1)
        return [dx, dw, db]

    def verify(got, what):
        for g, name in zip(got, ("dx", "dW", "db")):
            want, bar = ref[name]
            ratio = R.worst_ratio(np.asarray(g, np.float64).reshape(np.shape(want)), want, bar)
            assert ratio <= 1.0, "{} {}: {:.3g} x its bar".format(what, name, ratio)

    contract(Row(0, call, verify), what="deconv4x4s2_tiny_bwd {}".format(shape))


def test_upsample16_fwd_and_bwd(ops):
    """dim_upsample16_fwd / _bwd on a 2 x 2 x 5 x 7 map -> 64 x 96 planes (crop 8); bars of test_gpu_decoder.py"""
    g = torch.Generator().manual_seed(16)
    f = torch.randn((2, 2, 5, 7), generator=g, dtype=torch.float64, requires_grad=True)
    k1 = 1.0 - (torch.arange(32, dtype=torch.float64) - 15.5).abs() / 16.0
    wk = (k1[:, None] * k1[None, :]).expand(2, 1, 32, 32).contiguous()
    OH, OW = 64, 96
    up = F.conv_transpose2d(f, wk, None, stride=16, groups=2)[:, :, 8:8 + OH, 8:8 + OW] * 20.0
    dout = torch.randn(up.shape, generator=g, dtype=torch.float64)
    up.backward(dout)
    ref_up, ref_df = up.detach().numpy(), nhwc(f.grad).numpy()
    fwd_bar, bwd_bar = elem_bar(1e-5, 2e-5), max_bar(1e-5, 1e-5)

    def fwd(ws):
        y = ga.dense((2, 2, OH, OW), device=DEV)
        ops.upsample16_fwd(dev(nhwc(f.detach().float())), dev(wk.float()), OH, OW, crop=8, scale=20.0, out=y.tensor)
        return [y]

    def bwd(ws):
        df = ga.dense((2, 5, 7, 2), device=DEV)
        ops.upsample16_bwd(dev(dout.float()), dev(wk.float()), df.tensor, crop=8, scale=20.0)
        return [df]

    contract(Row(0, fwd, lambda got, what: fwd_bar(got[0], ref_up, what)), what="upsample16_fwd")
    contract(Row(0, bwd, lambda got, what: bwd_bar(got[0], ref_df, what)), what="upsample16_bwd")


# ---------------------------------------------------------------------------------------------------------------- packers
def pack_twice(n, dtype, pack, what, written=None):
    """pack into a NaN-prefilled and into a zero-prefilled buffer of exactly n elements: guards intact, images bit-identical.
    written: the documented number of leading elements a packer writes when that is not all n -- those are bit-identical and the rest
    keeps its prefill (the caller then shows with a forward through the image packed over NaN that no kernel reads the rest).
    -> the image packed over NaN (a tensor aliasing its arena, which the returned list keeps alive)"""
    arenas = []
    for word in (ga.NAN_WORD, ga.ZERO_WORD):
        a = ga.GuardArena(n, dtype=dtype, device=DEV, fill=word)
        pack(a.view())
        a.check("{} packed into {} elements".format(what, n))
        arenas.append(a)
    over_nan, over_zero = (a.payload_bytes().cpu().numpy() for a in arenas)
    esize = arenas[0].nbytes // max(n, 1)
    head = (n if written is None else written) * esize
    diff = np.nonzero(over_nan[:head] != over_zero[:head])[0]
    assert diff.size == 0, "{}: {} bytes of the packed image are not written (elements {} .. {} of {})".format(
        what, diff.size, diff[0] // esize, diff[-1] // esize, n)
    assert (over_nan[head:] == 0xFF).all() and not over_zero[head:].any(), "{}: written behind element {}".format(what, written)
    return arenas[0].view(), arenas


def _pk(ops, name, *args):
    from lib.hip.capi import check, current_stream

    check(getattr(ops.lib(), name)(*args, current_stream()))


def test_pack_conv2d_weight(ops):
    """dim_conv2d_pack_weight[_padded|_bf16]: Cin 8 (with its three-term image behind the f32 weights) through the first layer on both
    pipes, Cin 96 -> 64 filters, and 96 -> 64 padded to 128 output channels"""
    from lib.hip.capi import dptr

    L = ops.lib()
    # Cin 8
    shape = (1, 37, 53, 8, 64, 7, 2, 3)
    x, w, b, ref = conv_problem(shape)
    wd = dev(w)
    n = L.dim_conv2d_packed_weight_floats(64, 8, 7, 7)
    wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_conv2d_pack_weight", dptr(wd, f32), dptr(out, f32), 64, 8, 7, 7), "conv2d_pack_weight Cin 8")
    for split in (True, False):
        ops.set_winograd_split(split)
        try:
            for tile in (3, 6):
                y = ops.conv2d_fwd(dev(x), wp, dev(b), 64, 7, 7, 2, 3, slope=0.1, tile=tile).cpu().numpy()
                assert np.isfinite(y).all()
                CONV_BAR(y, ref, ("Cin 8 through the NaN-prefilled image", split, tile))
        finally:
            ops.set_winograd_split(True)
    # the bf16 twin, in the n elements its wrapper allocates: it writes the 13 chunks x 32 x 64 weights and leaves the rest alone (the
    # f32 buffer's three-term image has no bf16 counterpart); the bf16 first layer reads the weights only
    wp16, keep16 = pack_twice(n, bf16, lambda out: _pk(ops, "dim_conv2d_pack_weight_bf16", dptr(wd, f32), dptr(out, bf16), 64, 64, 8, 7, 7),
                              "conv2d_pack_weight_bf16 Cin 8", written=packed_floats(8, 64, 7))
    assert torch.equal(wp16[:packed_floats(8, 64, 7)], wp[:packed_floats(8, 64, 7)].bfloat16())
    _, _, _, ref16 = conv_problem(shape, True)
    for tile in (2, 3, 6):
        y = ops.conv2d_fwd(dev(x), wp16, dev(b), 64, 7, 7, 2, 3, slope=0.1, tile=tile).cpu().numpy()
        assert np.isfinite(y).all()
        F32_BAR(y, ref16, "Cin 8 bf16 through the NaN-prefilled image, tile {}".format(tile))
    # Cin 96
    shape = (3, 9, 11, 96, 64, 3, 2, 1)
    x, w, b, ref = conv_problem(shape)
    wd = dev(w)
    n = L.dim_conv2d_packed_weight_floats(64, 96, 3, 3)
    assert n == 9 * 96 * 64
    wp, keep2 = pack_twice(n, f32, lambda out: _pk(ops, "dim_conv2d_pack_weight", dptr(wd, f32), dptr(out, f32), 64, 96, 3, 3), "conv2d_pack_weight Cin 96")
    y = ops.conv2d_fwd(dev(x), wp, dev(b), 64, 3, 3, 2, 1, slope=0.1, tile=3).cpu().numpy()
    CONV_BAR(y, ref, "Cin 96 through the NaN-prefilled image")
    # padded: 64 filters in 128 output channels (the pad filters and their bias are zero: LeakyReLU(0) = 0)
    for as16 in (False, True):
        npad = 9 * 96 * 128
        if as16:
            wpp, keep3 = pack_twice(npad, bf16, lambda out: _pk(ops, "dim_conv2d_pack_weight_bf16", dptr(wd, f32), dptr(out, bf16), 64, 128, 96, 3, 3),
                                    "conv2d_pack_weight_bf16 padded")
        else:
            wpp, keep3 = pack_twice(npad, f32, lambda out: _pk(ops, "dim_conv2d_pack_weight_padded", dptr(wd, f32), dptr(out, f32), 64, 128, 96, 3, 3),
                                    "conv2d_pack_weight_padded")
        bp = torch.zeros(128, device=DEV)
        bp[:64] = dev(b)
        y = ops.conv2d_fwd(dev(x), wpp, bp, 128, 3, 3, 2, 1, slope=0.1, tile=4).cpu().numpy()
        assert np.isfinite(y).all() and not y[..., 64:].any()
        F32_BAR(y[..., :64], conv_problem(shape, True)[3] if as16 else ref, "padded through the NaN-prefilled image, bf16 {}".format(as16))
    del keep, keep16, keep2, keep3


def test_pack_conv2d_dgrad_weight(ops):
    """dim_conv2d_dgrad_pack_weight[_bf16], 64 -> 96 channels (dx padded to 128), 3x3 / stride 2: the four phase kernels"""
    from lib.hip.capi import dptr

    shape = (2, 9, 11, 96, 64)
    N, H, W, Cin, Cout = shape
    n = ops.lib().dim_conv2d_dgrad_packed_weight_floats(Cout, Cin, 3, 3, 2, 1)
    for as16 in (False, True):
        w, dy, ref = dgrad_problem(shape, 3, 2, 1, rounded=as16)
        wd = dev(w)
        if as16:
            wp, keep = pack_twice(n, bf16, lambda out: _pk(ops, "dim_conv2d_dgrad_pack_weight_bf16", dptr(wd, f32), dptr(out, bf16), Cout, Cin, 3, 3, 2, 1),
                                  "conv2d_dgrad_pack_weight_bf16")
        else:
            wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_conv2d_dgrad_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin, 3, 3, 2, 1),
                                  "conv2d_dgrad_pack_weight")
        dx = ga.ChannelWindow((N, H, W, 128 + 64), 0, 128, device=DEV)
        ops.conv2d_dgrad(dev(dy), Cout, wp, dx.tensor, Cin, 3, 3, 2, 1, accumulate=False)
        dx.check("dgrad through the NaN-prefilled image")
        got = dx.inside()
        assert np.isfinite(got).all() and not got[..., Cin:].any()       # the pad channels of dx come from zero weight columns
        # bars: test_gpu_backward.py (f32: 2e-5 max + 1e-5), test_gpu_bf16.py (exact: 1e-4 max + 1e-5)
        (max_bar(1e-4, 1e-5) if as16 else max_bar(2e-5, 1e-5))(got[..., :Cin], ref, "dgrad through the NaN-prefilled image, bf16 {}".format(as16))
        del keep


@pytest.mark.parametrize("kind", ["s1m2", "s1m4", "s2", "5x5", "5x5dgrad", "s1m2dgrad", "s1m4dgrad"])
def test_pack_winograd_weight(ops, wino_split, kind):
    """dim_winograd[_dgrad]_pack_weight (m 2, 4), dim_winograd3x3s2_pack_weight, dim_winograd5x5s2[_dgrad]_pack_weight, Cin 96 -> 64 filters:
    the f32 planes and the three-term image behind them, both read by the forward on its two arithmetics"""
    from lib.hip.capi import dptr

    L = ops.lib()
    if kind == "5x5dgrad":
        shape = (1, 15, 21, 32, 64)
        N, H, W, Cin, Cout = shape
        w, dy, ref = dgrad_problem(shape, 5, 2, 2)
        wd = dev(w)
        wp, keep = pack_twice(L.dim_winograd5x5s2_packed_weight_floats(Cout, Cin), f32,
                              lambda out: _pk(ops, "dim_winograd5x5s2_dgrad_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin), kind)
        dx = ga.dense((N, H, W, Cin), device=DEV)
        ops.conv2d_dgrad_winograd5x5s2(dev(dy), Cout, wp, dx.tensor, Cin)
        dx.check(kind)
        F32_BAR(dx.inside(), ref, kind + " through the NaN-prefilled image")
        return
    if kind in ("s1m2dgrad", "s1m4dgrad"):      # dim_winograd_dgrad_pack_weight: Cin output and Cout input channels, same size function
        m = int(kind[3])
        shape = (1, 8, 10, 64, 96)
        N, H, W, Cin, Cout = shape
        w, dy, ref = dgrad_problem(shape, 3, 1, 1)
        wd = dev(w)
        wp, keep = pack_twice(L.dim_winograd_packed_weight_floats(Cin, Cout, m), f32,
                              lambda out: _pk(ops, "dim_winograd_dgrad_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin, m), kind)
        dx = ga.dense((N, H, W, Cin), device=DEV)
        ops.conv2d_fwd_winograd(dev(dy), Cout, wp, None, Cin, slope=1.0, tile=3, out=dx.tensor, m=m)
        dx.check(kind)
        F32_BAR(dx.inside(), ref, kind + " through the NaN-prefilled image")
        return
    shape = {"s1m2": (1, 8, 10, 96, 64), "s1m4": (1, 8, 10, 96, 64), "s2": (1, 9, 11, 96, 64), "5x5": (1, 6, 9, 96, 64)}[kind]
    N, H, W, Cin, Cout = shape
    x, w, b, ref = wino_problem(kind, shape)
    wd = dev(w)
    if kind in ("s1m2", "s1m4"):
        m = WINO[kind][4]
        n = L.dim_winograd_packed_weight_floats(Cout, Cin, m)
        wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_winograd_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin, m), kind)
        y = ops.conv2d_fwd_winograd(dev(x), Cin, wp, dev(b), Cout, slope=0.1, tile=3, m=m)
    elif kind == "s2":
        n = L.dim_winograd3x3s2_packed_weight_floats(Cout, Cin)
        wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_winograd3x3s2_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin), kind)
        y = ops.conv2d_fwd_winograd3x3s2(dev(x), Cin, wp, dev(b), Cout, slope=0.1, tile=3)
    else:
        n = L.dim_winograd5x5s2_packed_weight_floats(Cout, Cin)
        wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_winograd5x5s2_pack_weight", dptr(wd, f32), dptr(out, f32), Cout, Cin), kind)
        y = ops.conv2d_fwd_winograd5x5s2(dev(x), Cin, wp, dev(b), Cout, slope=0.1, tile=3)
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    F32_BAR(y, ref, kind + " through the NaN-prefilled image")
    del keep


def test_pack_fc_weights(ops):
    """dim_fc_pack_weight through dim_fc_fwd, and dim_fc_dgrad_pack_weight[_bf16] through the kernel that reads it: fc6's input
    gradient as deepim/core/module.py runs it, a 1x1 convolution from dz (B,1,1,Out) to the C H W "channels" of the NHWC feature map,
    against float64 dz . W (bf16: on bf16-rounded operands), dx in a guarded buffer; bars: the f32 / exact bf16 forward bar"""
    from lib.hip.capi import dptr

    C, H, W, Out, B = 64, 3, 5, 256, 3
    w, b = fc_weights(C, H, W, Out)
    wd = dev(w)
    n = Out * C * H * W
    wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_fc_pack_weight", dptr(wd, f32), dptr(out, f32), Out, C, H, W), "fc_pack_weight")
    x, ref = fc_problem(B, C, H, W, Out)
    y = ops.fc_fwd(dev(x), wp, dev(b), Out, slope=0.1).cpu().numpy()
    assert np.isfinite(y).all()
    elem_bar(1e-4, 5e-5)(y, ref, "fc_fwd through the NaN-prefilled image")
    back = ops.fc_unpack_weight(wp, torch.empty_like(wd), C, H, W)
    assert torch.equal(back, wd)
    wg, keep_g = pack_twice(n, f32, lambda out: _pk(ops, "dim_fc_dgrad_pack_weight", dptr(wd, f32), dptr(out, f32), Out, C, H, W), "fc_dgrad_pack_weight")
    wg16, keep_g16 = pack_twice(n, bf16, lambda out: _pk(ops, "dim_fc_dgrad_pack_weight_bf16", dptr(wd, f32), dptr(out, bf16), Out, C, H, W),
                                "fc_dgrad_pack_weight_bf16")
    assert torch.equal(wg16, wg.bfloat16())
    g = torch.Generator().manual_seed(61)
    dz = torch.randn((B, Out), generator=g)
    for image, rnd in ((wg, lambda t: t.double()), (wg16, r16)):
        ref_dx = (rnd(dz) @ rnd(w)).reshape(B, C, H, W).permute(0, 2, 3, 1).reshape(B, 1, 1, H * W * C).numpy()
        dx = ga.dense((B, 1, 1, H * W * C), device=DEV)
        ops.conv2d_fwd_ex(dev(dz).view(B, 1, 1, Out), 0, Out, image, None, dx.tensor, 0, H * W * C, 1, 1, 1, 0, accumulate=False)
        dx.check("fc6 input gradient through the NaN-prefilled image")
        got = dx.inside()
        assert np.isfinite(got).all()
        F32_BAR(got, ref_dx, "fc6 input gradient through the NaN-prefilled image, {}".format(image.dtype))
    del keep, keep_g, keep_g16


def test_pack_deconv_and_small_cout_weights(ops):
    """dim_deconv4x4s2_pack_weight[_bf16] (Cin 96 -> 64) and dim_conv_small_cout_pack_weight (Cin 70: CinPad 96, the pad columns are
    written as zeros), each through its forward"""
    from lib.hip.capi import dptr

    N, Cin, H, W, Cout, OH, OW = 1, 96, 5, 7, 64, 10, 14
    g = torch.Generator().manual_seed(5)
    x = torch.randn((N, Cin, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((Cin, Cout, 4, 4), generator=g, dtype=torch.float64) / np.sqrt(Cin * 4)
    b = torch.randn((Cout,), generator=g, dtype=torch.float64)
    wd = dev(w.float())
    n = ops.lib().dim_deconv4x4s2_packed_weight_floats(Cin, Cout)
    for as16 in (False, True):
        xr, wr = (r16(x), r16(w)) if as16 else (x, w)
        ref = nhwc(F.leaky_relu(F.conv_transpose2d(xr, wr, b, stride=2)[:, :, 1:1 + OH, 1:1 + OW], 0.1)).numpy()
        if as16:
            wp, keep = pack_twice(n, bf16, lambda out: _pk(ops, "dim_deconv4x4s2_pack_weight_bf16", dptr(wd, f32), dptr(out, bf16), Cin, Cout),
                                  "deconv4x4s2_pack_weight_bf16")
        else:
            wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_deconv4x4s2_pack_weight", dptr(wd, f32), dptr(out, f32), Cin, Cout),
                                  "deconv4x4s2_pack_weight")
        y = ga.dense((N, OH, OW, Cout), device=DEV)
        ops.deconv4x4s2_fwd(dev(nhwc(x.float())), Cin, wp, dev(b.float()), y.tensor, Cout, crop=1, slope=0.1)
        y.check("deconv through the NaN-prefilled image")
        F32_BAR(y.inside(), ref, "deconv through the NaN-prefilled image, bf16 {}".format(as16))
        del keep
    # small Cout
    Cin, Cout = 70, 2
    xs = torch.randn((1, Cin, 6, 9), generator=g)
    ws = torch.randn((Cout, Cin, 3, 3), generator=g) / np.sqrt(9 * Cin)
    bs = torch.randn((Cout,), generator=g) * 0.1
    ref = nhwc(F.conv2d(xs.double(), ws.double(), bs.double(), padding=1)).numpy()
    wsd = dev(ws)
    n = Cout * 9 * ops.pad32(Cin)
    wp, keep = pack_twice(n, f32, lambda out: _pk(ops, "dim_conv_small_cout_pack_weight", dptr(wsd, f32), dptr(out, f32), Cout, Cin, 3, 3),
                          "conv_small_cout_pack_weight")
    xb = torch.zeros((1, 6, 9, 96), device=DEV)
    xb[..., :Cin] = dev(nhwc(xs))
    y = ops.conv_small_cout_fwd(xb, Cin, wp, dev(bs), Cout).cpu().numpy()
    assert np.isfinite(y).all()
    elem_bar(1e-4, 2e-5)(y, ref, "small Cout through the NaN-prefilled image")
    del keep
