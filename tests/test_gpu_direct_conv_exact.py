"""The direct convolution stack (csrc/conv_gather.hip, conv_bf16_tiles.hip, conv_first.hip, wgrad.hip and the host planning in
csrc/conv.hip) against torch's float64 result, EQUAL per element, on every small map.

tests/direct_conv_exact.py has the data classes (small integers, and nine-bit integers that bf16 rounding changes), the float64
reference and assert_exact_domain(), the condition under which float32 accumulation in any order gives the float64 result bit for
bit; it is asserted for every case before the kernel is called.  There is no tolerance anywhere in this file: every comparison is
np.array_equal (numeric: -0.0 equals 0.0), and a failure reports the number of wrong elements and the first one with both values.

Every call writes into a sentinel-filled output in a guard arena (tests/guard_arena.py): a ChannelWindow with sentinel channels on
both sides where the entry takes a channel stride / offset, a dense arena otherwise; reads inputs whose PAD_IN pad channels are NaN
where the entry takes an input stride; and works in a NaN workspace of exactly the queried size.  Guards and sentinels are checked
after every call.  A call the library refuses (DIM_ERR_ARG) must leave its output untouched, and must be in the REFUSED table of its
family, which holds what include/deepim_hip.h documents.

A test function is one (family, geometry, channel counts, data class) and loops over the sizes; the kernel choices (tiles, split-K,
accumulate) of one size run inside the loop so that they share the size's reference, which is computed once.
PLANS lists every function's cases without touching the GPU: tests/test_direct_conv_exact_host.py walks it.

Measured on an MI355X: DESIGN.md, "The direct convolutions pinned exactly"."""
import collections
import itertools

import numpy as np
import pytest
import torch

import direct_conv_exact as dc
import guard_arena as ga
from direct_conv_exact import K3S1, K3S2, K5S2, K7S2, DECONV, Geometry, SLOPE, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD_IN, PAD_OUT, COFF = 8, 16, 4
f32, bf16 = torch.float32, torch.bfloat16

EDGE, SWEEP, SMALL_BATCH = dc.EDGE, dc.SWEEP, dc.SMALL_BATCH
SPLIT_SIZES = ((1, 1), (3, 5), (8, 8), (16, 17), (33, 9))                      # split-K on a few sizes
EX_SIZES = ((1, 1), (1, 16), (16, 1), (2, 3), (5, 8), (8, 5), (16, 16), (16, 17), (17, 16), (17, 17), (9, 33), (32, 10))
DECONV_EDGE = tuple(range(1, 10)) + (15, 16, 17)
DECONV_SIZES = tuple((h, w) for h in DECONV_EDGE for w in DECONV_EDGE)
PATCH_WGRAD_SIZES = ((30, 40), (33, 37), (35, 35), (40, 32), (41, 30), (37, 33))   # Ho * Wo >= 1200: the patch form of the bf16 wgrad


def pad0_sizes(k):
    """maps at pad 0 (H, W >= k): one output pixel, one row / column more, an odd map"""
    return ((k, k), (k, k + 1), (k + 1, k), (k + 2, k + 5), (9, 11))


def sized(g):
    """(geometry, N, H, W) of a sweep: every (H, W) in EDGE x EDGE at N = 2 and pad (k - 1) / 2, N = 5 on the maps up to 3 x 3, pad 0"""
    return ([(g, 2, h, w) for h, w in SWEEP] + [(g, 5, h, w) for h, w in SMALL_BATCH] +
            [(Geometry(g.k, g.s, 0), 2, h, w) for h, w in pad0_sizes(g.k)])


# A run is one library call: `key` names the problem (direct_conv_exact.problem), the rest says which reference it is compared with
# (pipe, accumulate, window, fold -- what assert_exact_domain needs too) and `how` is the kernel choice, read by the family's runner.
Run = collections.namedtuple("Run", "key pipe accumulate window fold how")


def run(family, g, kind, N, H, W, Cin, Cout, pipe, how, accumulate=False, window=None, fold=False):
    return Run((family, g, kind, N, H, W, Cin, Cout), pipe, accumulate, window, fold, how)


# ---------------------------------------------------------------------------------------------------------------- refusals
# What the library refuses with DIM_ERR_ARG, per family, as include/deepim_hip.h documents it: (name, predicate of a run)
def _how(r, name, default=None):
    return dict(r.how).get(name, default)


T9_STRIDE2 = "tile 9 at stride 2 needs Cout % 128 == 0"
T9_F32_DECONV = "tile 9 is bf16-only"
REFUSED = {
    "fwd": (
        ("a 128-wide tile (1, 4) needs Cout % 128 == 0", lambda r: _how(r, "tile") in (1, 4) and r.key[7] % 128 != 0),
        ("tile 4 is not built for the 8-channel layer", lambda r: _how(r, "tile") == 4 and r.key[6] == 8),
        ("tiles 7, 8, 9 are bf16-only", lambda r: _how(r, "tile") in (7, 8, 9) and r.pipe == "f32"),
        ("tile 7: 3x3 or 5x5 / stride 2, Cout % 128 == 0; a 5x5 / stride-1 request is refused",
         lambda r: _how(r, "tile") == 7 and (r.key[7] % 128 != 0 or (r.key[1].k == 5 and r.key[1].s == 1))),
        ("tile 8 needs Cout % 256 == 0", lambda r: _how(r, "tile") == 8 and r.key[7] % 256 != 0),
        (T9_STRIDE2, lambda r: _how(r, "tile") == 9 and r.key[1].s == 2 and r.key[7] % 128 != 0),
        ("tile 9 at stride 1 takes KH, KW <= 3", lambda r: _how(r, "tile") == 9 and r.key[1].s == 1 and r.key[1].k > 3),
        ("tile 6 is the 8-channel 7x7 / stride-2 / 64-filter layer", lambda r: _how(r, "tile") == 6 and (r.key[6] != 8 or r.key[7] != 64)),
        ("an empty output at pad 0", lambda r: min(dc.out_hw(r.key[4], r.key[5], r.key[1])) < 1),
    ),
    "dgrad": (
        ("tile 7 is bf16-only (an f32 request for tile 9 runs every phase on the gathered-tap kernel)", lambda r: r.pipe == "f32" and _how(r, "tile") == 7),
        ("tile 4 / tile 7 need Cin rounded up to 64 to be a multiple of 128", lambda r: _how(r, "tile") in (4, 7) and -(-r.key[6] // 64) * 64 % 128 != 0),
        ("tile 7 writes a dense output: stride 1 only", lambda r: _how(r, "tile") == 7 and r.key[1].s != 1),
        ("the folded form needs phases of 2 .. 9 taps: 3x3 / stride 1 and 5x5 / stride 2 layers",
         lambda r: r.fold and (r.key[1].k, r.key[1].s) not in ((3, 1), (5, 2))),
    ),
    "wgrad": (
        ("accumulate with more than one split", lambda r: r.accumulate and _how(r, "clamped", 1) > 1),
        ("accumulate in the bf16 patch form", lambda r: r.accumulate and _how(r, "patch", False)),
    ),
    "deconv": (
        (T9_F32_DECONV, lambda r: _how(r, "tile") == 9 and r.pipe == "f32"),
    ),
}


def refusal(r):
    """-> the documented reason the library refuses this run, or None"""
    for name, rule in REFUSED[r.key[0]]:
        if rule(r):
            return name
    return None


# ---------------------------------------------------------------------------------------------------------------- plans (no GPU)
def plan_forward_f32(g, kind):
    """dim_conv2d_fwd, Cin 32 -> Cout 128: tiles 1, 2, 3, 4 (conv_fwd_kernel 128x128 on 4 waves, 128x64, 64x64, 128x128 on 8 waves);
    on a few sizes splits = 3 as one call and as dim_conv2d_fwd_partial + dim_splitk_reduce"""
    for gg, N, H, W in sized(g):
        for tile in (1, 2, 3, 4):
            yield run("fwd", gg, kind, N, H, W, 32, 128, "f32", (("entry", "fwd"), ("tile", tile)))
        if gg.p and N == 2 and (H, W) in SPLIT_SIZES:
            for two_phase in (False, True):
                yield run("fwd", gg, kind, N, H, W, 32, 128, "f32", (("entry", "fwd"), ("tile", 3), ("splits", 3), ("two_phase", two_phase)))


def plan_first_layer(kind):
    """Cin 8, 7x7 / stride 2 / pad 3, 64 filters: tiles 2, 3 (conv_fwd_kernel<.., CIN8>), tile 6 (conv1_halo_*: the three-term kernel
    with the switch on, the f32 kernel with it off, the bf16 kernel on bf16 weights)"""
    for gg, N, H, W in sized(K7S2):
        for tile, split, pipe in ((2, 1, "f32"), (3, 1, "f32"), (6, 1, "f32"), (6, 0, "f32"), (6, 1, "bf16")):
            yield run("fwd", gg, kind, N, H, W, 8, 64, pipe, (("entry", "fwd"), ("tile", tile), ("wino_split", split)))


def plan_forward_bf16(g, Cin, kind):
    """dim_conv2d_fwd_bf16: tiles 3, 4 (conv_bf16_kernel), 7 (conv_bf16_halo_kernel), 9 (conv_bf16_patch_kernel) at Cout 128, tile 9 at
    Cout 64 (stride 1: its 64-channel form; stride 2: refused), tile 8 (128 x 256) at Cout 256, split-K 2 on tile 3 on a few sizes"""
    for gg, N, H, W in sized(g):
        for tile, Cout in ((3, 128), (4, 128), (7, 128), (9, 128), (9, 64), (8, 256)):
            yield run("fwd", gg, kind, N, H, W, Cin, Cout, "bf16", (("entry", "fwd"), ("tile", tile)))
        if gg.p and N == 2 and (H, W) in SPLIT_SIZES:
            yield run("fwd", gg, kind, N, H, W, Cin, 128, "bf16", (("entry", "fwd"), ("tile", 3), ("splits", 2)))


def plan_forward_ex(g, kind):
    """ops.conv2d_fwd_ex, f32 (tile 3) and bf16 (tiles 3, 9): channel windows inside wider buffers, accumulate on integer content"""
    for H, W in EX_SIZES:
        for pipe, tile in (("f32", 3), ("bf16", 3), ("bf16", 9)):
            for acc in (False, True):
                yield run("fwd", g, kind, 2, H, W, 32, 128, pipe, (("entry", "ex"), ("tile", tile)), accumulate=acc)


def plan_input_gradient(g, Cin, Cout, kind):
    """dim_conv2d_dgrad (tile 3), dim_conv2d_dgrad_bf16 (tile 3; 4 and, at stride 1, 7 where Cin % 128 == 0; 9: every phase of 2 .. 9
    taps on the patch kernel, the single-tap phase of 3x3 / stride 2 on the gathered kernel, phases of extent 0 at H or W = 1),
    accumulate on and off, split-K 2 (Cout >= 64: every phase has two K chunks)"""
    for gg, N, H, W in sized(g):
        choices = [("f32", 3, 1, False), ("bf16", 3, 1, False), ("bf16", 3, 1, True), ("bf16", 9, 1, False), ("bf16", 9, 1, True),
                   ("bf16", 3, 2, False), ("bf16", 3, 2, True)]
        if Cin % 128 == 0:
            choices += [("bf16", 4, 1, False), ("f32", 4, 1, True)] + ([("bf16", 7, 1, False)] if gg.s == 1 else [])
        for pipe, tile, splits, acc in choices:
            yield run("dgrad", gg, kind, N, H, W, Cin, Cout, pipe, (("entry", "dgrad"), ("tile", tile), ("splits", splits)), accumulate=acc)


FOLD_TIES_PIXELS = (1 << 24) // (4 * 272 * 9 * 64)      # 26


def plan_folded_gradient(g, Cin, kind):
    """dim_conv2d_dgrad_bf16_lrelu: dz and db, accumulate_db on and off; y_act from `ints`, whose exact zeros take the slope branch.
    db is a sum over ALL pixels of the batch, in units of 1/4: with `ints` every size of the sweep stays inside the exact domain
    (direct_conv_exact.assert_exact_domain(fold=True) bounds 4 db too), with the ties classes only the maps of N H W <= 26 pixels do
    (4 x 272 x 9 taps x 64 channels x 26 < 2^24), so those classes run on these maps: single blocks, and phases of extent 0"""
    for gg, N, H, W in sized(g):
        if kind != "ints" and N * H * W > FOLD_TIES_PIXELS:
            continue
        for acc_db in (False, True):
            yield run("dgrad", gg, kind, N, H, W, Cin, 64, "bf16", (("entry", "lrelu"), ("accumulate_db", acc_db)), fold=True)


def clamped_splits(N, Ho, Wo, splits, blocks=None):
    """the library's clamp of a pixel-split count: steps of 32 pixels (patch form: 8 x 8 blocks), equal ranges, no empty one"""
    steps = blocks if blocks else -(-N * Ho * Wo // 32)
    s = max(1, min(splits, steps))
    per = -(-steps // s)
    return -(-steps // per)


def plan_weight_gradient(g, Cin, Cout, pipe, kind):
    """dim_conv2d_wgrad / _bf16 (conv_wgrad_kernel / conv_wgrad_bf16_kernel): splits 1, 2, 100 (clamped), dz at channel offset 0 and 4
    of a wider row, accumulate with one split; dim_conv2d_wgrad_oihw against the unpacked packed result and with scale 0.5 on top of
    integer content"""
    for gg, N, H, W in sized(g):
        Ho, Wo = dc.out_hw(H, W, gg)
        for splits, coff, acc, oihw in ((1, 0, False, False), (2, 4, False, False), (100, 0, False, False), (1, 4, True, False),
                                        (2, 0, False, True), (100, 4, True, True)):
            how = (("entry", "oihw" if oihw else "wgrad"), ("splits", splits), ("dz_coff", coff),
                   ("clamped", 1 if oihw else clamped_splits(N, Ho, Wo, splits)))
            yield run("wgrad", gg, kind, N, H, W, Cin, Cout, pipe, how, accumulate=acc)


def plan_weight_gradient_first_layer(kind):
    """Cin 8: the n = 13 * 32 * 64 prefix of the packed buffer"""
    for gg, N, H, W in sized(K7S2):
        Ho, Wo = dc.out_hw(H, W, gg)
        for pipe in ("f32", "bf16"):
            for splits, coff, acc, oihw in ((1, 0, False, False), (2, 4, False, False), (100, 0, False, False), (1, 4, True, False),
                                            (2, 0, False, True)):
                how = (("entry", "oihw" if oihw else "wgrad"), ("splits", splits), ("dz_coff", coff),
                       ("clamped", 1 if oihw else clamped_splits(N, Ho, Wo, splits)))
                yield run("wgrad", gg, kind, N, H, W, 8, 64, pipe, how, accumulate=acc)


def plan_weight_gradient_patch(Cin, Cout, kind):
    """the bf16 patch form (conv_wgrad_bf16_patch_kernel: 3x3 / stride 1 / pad 1, Cout % 128 == 0, Ho Wo >= 1200): the smallest maps
    that qualify, their 8 x 8 blocks hanging over neither, one or both edges; N 1 and 2, splits 1, 7, 100"""
    for (H, W), N in itertools.product(PATCH_WGRAD_SIZES, (1, 2)):
        blocks = N * (-(-H // 8)) * (-(-W // 8))
        for splits in (1, 7, 100):
            how = (("entry", "wgrad"), ("splits", splits), ("dz_coff", 4 if splits == 7 else 0), ("patch", True),
                   ("clamped", clamped_splits(N, H, W, splits, blocks)))
            yield run("wgrad", K3S1, kind, N, H, W, Cin, Cout, "bf16", how)
        yield run("wgrad", K3S1, kind, N, H, W, Cin, Cout, "bf16", (("entry", "oihw"), ("splits", 7), ("dz_coff", 0), ("patch", True), ("clamped", 1)))


def plan_deconvolution(Cin, kind):
    """ops.deconv4x4s2_fwd into a concat buffer at out_coff 4, crop 1: f32 tile 3, bf16 tiles 3 and 9 (the batched four-phase launch of
    the gathered and of the patch kernel); output windows (2h - 1, 2w - 1) and (2h, 2w) as the decoder uses them"""
    for h, w in DECONV_SIZES:
        for window in ((2 * h - 1, 2 * w - 1), (2 * h, 2 * w)):
            for Cout in (64, 128):
                for pipe, tile in (("f32", 3), ("bf16", 3), ("bf16", 9)):
                    yield run("deconv", DECONV, kind, 2, h, w, Cin, Cout, pipe, (("entry", "deconv"), ("tile", tile)), window=window)


FWD_F32 = [(g, k) for g in (K3S1, K5S2) for k in dc.CLASSES]
FWD_BF16 = [(g, c, k) for g in (K3S1, K3S2, K5S2) for c in (32, 64, 96) for k in dc.CLASSES]
DGRAD = [(g, ci, co, k) for g in (K3S1, K3S2, K5S2) for ci, co in ((32, 64), (64, 128), (128, 64)) for k in dc.CLASSES]
FOLDED = [(g, c, k) for g in (K3S1, K5S2) for c in (64, 128) for k in dc.CLASSES]
WGRAD = [(g, ci, co, p, k) for g in (K3S1, K3S2, K5S2) for ci, co in ((32, 64), (64, 128)) for p in ("f32", "bf16") for k in dc.CLASSES]
WGRAD_PATCH = [(ci, co, k) for ci, co in ((32, 128), (96, 256)) for k in ("x_ties", "w_ties")]
DECONVS = [(c, k) for c in (32, 70) for k in dc.CLASSES]

PLANS = ([("forward_f32", plan_forward_f32, a) for a in FWD_F32] + [("first_layer", plan_first_layer, (k,)) for k in dc.CLASSES] +
         [("forward_bf16", plan_forward_bf16, a) for a in FWD_BF16] + [("forward_ex", plan_forward_ex, a) for a in FWD_F32] +
         [("input_gradient", plan_input_gradient, a) for a in DGRAD] + [("folded_gradient", plan_folded_gradient, a) for a in FOLDED] +
         [("weight_gradient", plan_weight_gradient, a) for a in WGRAD] +
         [("weight_gradient_first_layer", plan_weight_gradient_first_layer, (k,)) for k in dc.CLASSES] +
         [("weight_gradient_patch", plan_weight_gradient_patch, a) for a in WGRAD_PATCH] + [("deconvolution", plan_deconvolution, a) for a in DECONVS])


def ident(v):
    return "k{}s{}p{}".format(*v) if isinstance(v, Geometry) else str(v)


# ---------------------------------------------------------------------------------------------------------------- scaffolding
@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


@pytest.fixture
def arithmetic(ops):
    """sets the arithmetic of the first layer's tile 6 for the calls of one test; the default (three terms) is back afterwards"""
    try:
        yield ops.set_winograd_split
    finally:
        ops.set_winograd_split(True)


def dev(a):
    return torch.tensor(np.asarray(a), dtype=f32, device=DEV)      # a copy: the problems' arrays are read-only


def padded(a, before=0, zero_to=0):
    """(..., C) -> device (..., before + C' + PAD_IN): NaN in front of and behind the channels, which nothing may read; zero_to: the
    channels [C, zero_to) are zero (an entry whose packed weights are zero there reads them)"""
    C = a.shape[-1]
    t = torch.full(a.shape[:-1] + (before + max(C, zero_to) + PAD_IN,), float("nan"), device=DEV)
    t[..., before:before + C] = dev(a)
    t[..., before + C:before + max(C, zero_to)] = 0.0
    return t


class Buffers(object):
    """the guarded outputs and workspaces of one size, reused by the size's runs (an arena is two 1 MiB guards: allocating one per call
    would dominate the run time); every reuse starts from the sentinel / NaN fill"""

    def __init__(self, spaces):
        self.pool, self.spaces = {}, spaces

    def window(self, shape, coff, C, prior=None):
        key = ("w", tuple(shape), coff, C)
        if key not in self.pool:
            self.pool[key] = ga.ChannelWindow(shape, coff, C, device=DEV)
        w = self.pool[key]
        w.arena.fill(ga.SENTINEL_WORD)
        if prior is not None:
            w.tensor[..., coff:coff + C] = prior
        return w

    def workspace(self, floats):
        """NaN words (every byte 0xFF); kept for the whole function: the size depends on the channel counts and the split count only"""
        if not floats:
            return None
        if int(floats) not in self.spaces:
            self.spaces[int(floats)] = ga.GuardArena(int(floats), device=DEV, fill=ga.NAN_WORD)
        ws = self.spaces[int(floats)]
        ws.payload_bytes().fill_(255)
        return ws


def untouched(w, before, what):
    """after a refusal: every byte of the output is what it was before the call (the sentinel, and the prior content of an accumulate call)"""
    w.arena.check(what)
    assert torch.equal(w.arena.payload_bytes(), before), "{}: refused, but wrote".format(what)


def guarded(call, outs, ws, r, what):
    """one library call on guarded buffers -> True when it ran, False when the library refused it with DIM_ERR_ARG (then nothing was
    written, and the refusal is a documented one); a call that runs must not be one the table says is refused"""
    from lib.hip import capi

    why = refusal(r)
    before = [o.arena.payload_bytes().clone() for o in outs] if why else None
    try:
        call()
    except capi.DeepIMHipError as e:
        assert "error -1:" in str(e), (what, str(e))
        assert why is not None, "{}: refused, which include/deepim_hip.h does not document: {}".format(what, e)
        for o, b in zip(outs, before):
            untouched(o, b, what)
        if ws is not None:
            ws.check(what + ": workspace of a refused call")
            assert bool((ws.payload_bytes() == 255).all()), "{}: refused, but wrote into the workspace".format(what)
        return False
    assert why is None, "{}: ran, but the table says it is refused ({})".format(what, why)
    for o in outs:
        o.check(what)
    if ws is not None:
        ws.check(what + ": workspace")
    return True


def same(got, want, what):
    m = dc.mismatch(got, want)
    assert m is None, "{}: {} of {} elements differ; first at {}: got {!r}, expected {!r}".format(what, m[0], np.asarray(want).size, m[1], m[2], m[3])


def describe(r):
    family, g, kind, N, H, W, Cin, Cout = r.key
    return "{} {} {} N{} {}x{} {}->{} {} {}{}{}".format(family, ident(g), kind, N, H, W, Cin, Cout, r.pipe, dict(r.how),
                                                       " accumulate" if r.accumulate else "", " window {}".format(r.window) if r.window else "")


# ---------------------------------------------------------------------------------------------------------------- runners
class Runner(object):
    """executes the runs of one plan; packed weights are kept per problem, buffers per size"""

    def __init__(self, ops, arithmetic=None):
        self.ops, self.L, self.arithmetic = ops, ops.lib(), arithmetic
        self.size, self.bufs, self.packed, self.count, self.refused, self.spaces = None, None, {}, 0, collections.Counter(), {}

    def __call__(self, r):
        size = (r.key[1],) + r.key[3:6]
        if size != self.size:
            self.size, self.bufs, self.packed = size, Buffers(self.spaces), {}
        self.key = r.key
        p = dc.problem(*r.key)
        what = describe(r)
        if min(p.Ho, p.Wo) >= 1:
            dc.assert_exact_domain(p, r.pipe, r.accumulate, r.window, r.fold)
        ran = getattr(self, "_" + dict(r.how)["entry"])(p, r, what)
        self.count += 1
        if not ran:
            self.refused[refusal(r)] += 1
        return ran

    def weights(self, name, make, pipe):
        """the f32 packed array, or its bf16 image through to_bf16 (what the reference rounds)"""
        key = (self.key, name, pipe)
        if key not in self.packed:
            wp = make()
            self.packed[key] = self.ops.to_bf16(wp) if pipe == "bf16" else wp
        return self.packed[key]

    # ---- forward
    def _fwd(self, p, r, what):
        ops, g, h = self.ops, p.g, dict(r.how)
        N, H, W, Cin, Cout = p.N, p.H, p.W, p.Cin, p.Cout
        Ho, Wo = max(p.Ho, 0), max(p.Wo, 0)
        if self.arithmetic:
            self.arithmetic(bool(h.get("wino_split", 1)))
        wp = self.weights("fwd", lambda: ops.conv2d_pack_weight(dev(p.w)), r.pipe)
        splits = h.get("splits", 1)
        need = self.L.dim_conv2d_workspace_floats(N, H, W, Cin, Cout, g.k, g.k, g.s, g.p, splits) if min(Ho, Wo) >= 1 else 0
        ws = self.bufs.workspace(need)
        y = self.bufs.window((N, max(Ho, 1), max(Wo, 1), Cout), 0, Cout)      # an empty output: any buffer, which must stay untouched
        x, b = dev(p.x), dev(p.b)

        def call():
            ops.conv2d_fwd(x, wp, b, Cout, g.k, g.k, g.s, g.p, slope=SLOPE, splits=splits, tile=h["tile"], out=y.tensor,
                           workspace=None if ws is None else ws.view(), events=[] if h.get("two_phase") else None)

        if not guarded(call, [y], ws, r, what):
            return False
        same(y.inside(), dc.reference(p, r.pipe), what)
        return True

    def _ex(self, p, r, what):
        ops, g, h = self.ops, p.g, dict(r.how)
        N, Cin, Cout = p.N, p.Cin, p.Cout
        wp = self.weights("fwd", lambda: ops.conv2d_pack_weight(dev(p.w)), r.pipe)
        y = self.bufs.window((N, p.Ho, p.Wo, COFF + Cout + PAD_OUT), COFF, Cout, prior=dev(p.prior) if r.accumulate else None)
        x, b = padded(p.x, before=4), dev(p.b)

        def call():
            ops.conv2d_fwd_ex(x, 4, Cin, wp, b, y.tensor, COFF, Cout, g.k, g.k, g.s, g.p, slope=SLOPE, tile=h["tile"], accumulate=r.accumulate)

        if not guarded(call, [y], None, r, what):
            return False
        same(y.inside(), dc.reference(p, r.pipe, r.accumulate), what)
        return True

    # ---- input gradient
    def _dgrad(self, p, r, what):
        ops, g, h = self.ops, p.g, dict(r.how)
        N, H, W, Cin, Cout = p.N, p.H, p.W, p.Cin, p.Cout
        cpad = ops.pad64(Cin)
        wd = self.weights("dgrad", lambda: ops.conv2d_dgrad_pack_weight(dev(p.w), g.s, g.p), r.pipe)
        prior = None
        if r.accumulate:
            prior = torch.zeros((N, H, W, cpad), device=DEV)
            prior[..., :Cin] = dev(p.prior)
        dx = self.bufs.window((N, H, W, cpad + PAD_OUT), 0, cpad, prior=prior)
        splits = h.get("splits", 1)
        ws = self.bufs.workspace(self.L.dim_conv2d_dgrad_splitk_workspace_floats(N, H, W, cpad + PAD_OUT, splits))
        dy = padded(p.dy)

        def call():
            ops.conv2d_dgrad(dy, Cout, wd, dx.tensor, Cin, g.k, g.k, g.s, g.p, accumulate=r.accumulate, tile=h["tile"], splits=splits,
                             workspace=None if ws is None else ws.view())

        if not guarded(call, [dx], ws, r, what):
            return False
        got = dx.inside()
        same(got[..., :Cin], dc.reference(p, r.pipe, r.accumulate), what)
        same(got[..., Cin:], np.zeros(got[..., Cin:].shape), what + ": the pad channels up to 64")
        return True

    def _lrelu(self, p, r, what):
        ops, g, h = self.ops, p.g, dict(r.how)
        N, H, W, Cin, Cout = p.N, p.H, p.W, p.Cin, p.Cout
        wd = self.weights("dgrad", lambda: ops.conv2d_dgrad_pack_weight(dev(p.w), g.s, g.p), "bf16")
        dz = self.bufs.window((N, H, W, Cin), 0, Cin)
        db = self.bufs.window((Cin,), 0, Cin, prior=dev(p.db_prior) if h["accumulate_db"] else None)
        ws = self.bufs.workspace(self.L.dim_conv2d_dgrad_lrelu_workspace_floats(N, H, W, Cin, g.s))
        dy, y_act = padded(p.dy), dev(p.y_act)

        def call():
            ops.conv2d_dgrad_lrelu(dy, Cout, wd, dz.tensor, y_act, Cin, g.k, g.k, g.s, g.p, db.tensor, slope=SLOPE, workspace=ws.view(),
                                   accumulate_db=h["accumulate_db"])

        if not guarded(call, [dz, db], ws, r, what):
            return False
        want_dz, want_db = dc.folded(p, "bf16", h["accumulate_db"])
        same(dz.inside(), want_dz, what + ": dz")
        same(db.inside(), want_db, what + ": db")
        return True

    # ---- weight gradient
    def _wgrad_inputs(self, p, h):
        coff = h["dz_coff"]
        return padded(p.x), padded(p.dz, before=coff)

    def _wgrad(self, p, r, what):
        ops, g, h = self.ops, p.g, dict(r.how)
        Cin, Cout, k = p.Cin, p.Cout, g.k
        n = dc.packed_floats(Cin, Cout, k)
        total = self.L.dim_conv2d_packed_weight_floats(Cout, Cin, k, k)
        assert total >= n
        if h.get("patch"):     # the documented rule of the patch form, and the planner's account of it: 8 x 8 blocks, not 32-pixel steps
            assert g == K3S1 and Cout % 128 == 0 and p.Ho * p.Wo >= 1200 and r.pipe == "bf16"
            blocks = p.N * (-(-p.Ho // 8)) * (-(-p.Wo // 8))
            assert self.L.dim_conv2d_wgrad_bf16_splits(p.N, p.H, p.W, Cin, Cout, 3, 3, 1, 1, 1 << 20) == blocks // 4
        else:
            assert not (g == K3S1 and Cout % 128 == 0 and p.Ho * p.Wo >= 1200)
        dw = self.bufs.window((total,), 0, n, prior=dev(dc.packed(p.prior)) if r.accumulate else None)
        ws = self.bufs.workspace(self.L.dim_conv2d_wgrad_workspace_floats(Cout, Cin, k, k, h["splits"]))
        x, dz = self._wgrad_inputs(p, h)

        def call():
            ops.conv2d_wgrad(x, Cin, dz, Cout, k, k, g.s, g.p, dw.tensor, splits=h["splits"], dz_coff=h["dz_coff"],
                             workspace=None if ws is None else ws.view(), accumulate=r.accumulate, bf16_mfma=r.pipe == "bf16")

        if not guarded(call, [dw], ws, r, what):
            return False
        same(dw.inside(), dc.packed(dc.reference(p, r.pipe, r.accumulate)), what)
        return True

    def _oihw(self, p, r, what):
        """accumulate: dw starts as the integer prior and the call adds 0.5 x the gradient (exact: a power of two)"""
        ops, g, h = self.ops, p.g, dict(r.how)
        Cin, Cout, k = p.Cin, p.Cout, g.k
        dw = self.bufs.window((Cout, Cin * k * k), 0, Cin * k * k, prior=dev(p.prior).reshape(Cout, -1) if r.accumulate else None)
        ws = self.bufs.workspace(self.L.dim_conv2d_wgrad_workspace_floats(Cout, Cin, k, k, h["splits"] + 1))
        x, dz = self._wgrad_inputs(p, h)

        def call():
            ops.conv2d_wgrad_oihw(x, Cin, dz, Cout, k, k, g.s, g.p, dw.tensor.view(Cout, Cin, k, k), splits=h["splits"], dz_coff=h["dz_coff"],
                                  workspace=ws.view(), bf16_mfma=r.pipe == "bf16", scale=SCALE if r.accumulate else 1.0, accumulate=r.accumulate)

        if not guarded(call, [dw], ws, r, what):
            return False
        grad = dc.reference(p, r.pipe)
        want = p.prior + SCALE * grad if r.accumulate else grad
        same(dw.inside().reshape(want.shape), want, what)
        if not r.accumulate:    # the packed entry + the layout converter: equal
            packed = torch.zeros((self.L.dim_conv2d_packed_weight_floats(Cout, Cin, k, k),), device=DEV)
            ops.conv2d_wgrad(x, Cin, dz, Cout, k, k, g.s, g.p, packed, splits=h["splits"], dz_coff=h["dz_coff"], bf16_mfma=r.pipe == "bf16")
            two = ops.conv2d_unpack_weight(packed, torch.empty((Cout, Cin, k, k), device=DEV))
            same(dw.inside().reshape(want.shape), two.cpu().numpy(), what + ": against unpack of packed")
        return True

    # ---- deconvolution
    def _deconv(self, p, r, what):
        ops, h = self.ops, dict(r.how)
        N, Cin, Cout = p.N, p.Cin, p.Cout
        OH, OW = r.window
        w = dev(p.w)
        wp = self.weights("deconv", lambda: ops.deconv4x4s2_pack_weight(w), r.pipe)
        y = self.bufs.window((N, OH, OW, COFF + Cout + PAD_OUT), COFF, Cout)
        x, b = padded(p.x, zero_to=ops.pad32(Cin)), dev(p.b)

        def call():
            ops.deconv4x4s2_fwd(x, Cin, wp, b, y.tensor, Cout, crop=1, slope=SLOPE, out_coff=COFF, tile=h["tile"])

        if not guarded(call, [y], None, r, what):
            return False
        same(y.inside(), dc.reference(p, r.pipe, window=r.window), what)
        return True


def execute(ops, plan, args, arithmetic=None, expect_refused=()):
    runner = Runner(ops, arithmetic)
    for r in plan(*args):
        runner(r)
    print("%s%s: %d calls, %d refused %s" % (plan.__name__, tuple(ident(a) for a in args), runner.count, sum(runner.refused.values()), dict(runner.refused)))
    assert sorted(runner.refused) == sorted(expect_refused), (sorted(runner.refused), sorted(expect_refused))
    return runner


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("g,kind", FWD_F32, ids=ident)
def test_forward_f32(ops, g, kind):
    execute(ops, plan_forward_f32, (g, kind))


@pytest.mark.parametrize("kind", dc.CLASSES)
def test_first_layer(ops, arithmetic, kind):
    execute(ops, plan_first_layer, (kind,), arithmetic)


@pytest.mark.parametrize("g,Cin,kind", FWD_BF16, ids=ident)
def test_forward_bf16(ops, g, Cin, kind):
    """tile 9 at Cout 64 exists at stride 1 only: at stride 2 the patch kernel is built for 128 channels and the request is refused"""
    execute(ops, plan_forward_bf16, (g, Cin, kind), expect_refused=[T9_STRIDE2] if g.s == 2 else [])


@pytest.mark.parametrize("g,kind", FWD_F32, ids=ident)
def test_forward_ex(ops, g, kind):
    execute(ops, plan_forward_ex, (g, kind))


@pytest.mark.parametrize("g,Cin,Cout,kind", DGRAD, ids=ident)
def test_input_gradient(ops, g, Cin, Cout, kind):
    execute(ops, plan_input_gradient, (g, Cin, Cout, kind))


@pytest.mark.parametrize("g,Cin,kind", FOLDED, ids=ident)
def test_folded_gradient(ops, g, Cin, kind):
    execute(ops, plan_folded_gradient, (g, Cin, kind))


@pytest.mark.parametrize("g,Cin,Cout,pipe,kind", WGRAD, ids=ident)
def test_weight_gradient(ops, g, Cin, Cout, pipe, kind):
    """accumulate with splits == 1 runs; (100 splits, accumulate) through the OIHW entry runs too: the slabs are summed on top of dw"""
    execute(ops, plan_weight_gradient, (g, Cin, Cout, pipe, kind))


@pytest.mark.parametrize("kind", dc.CLASSES)
def test_weight_gradient_first_layer(ops, kind):
    execute(ops, plan_weight_gradient_first_layer, (kind,))


@pytest.mark.parametrize("Cin,Cout,kind", WGRAD_PATCH, ids=ident)
def test_weight_gradient_patch_form(ops, Cin, Cout, kind):
    execute(ops, plan_weight_gradient_patch, (Cin, Cout, kind))


@pytest.mark.parametrize("Cin,kind", DECONVS, ids=ident)
def test_deconvolution(ops, Cin, kind):
    execute(ops, plan_deconvolution, (Cin, kind))


REFUSALS = [
    run("fwd", Geometry(5, 1, 2), "ints", 2, 9, 11, 32, 128, "bf16", (("entry", "fwd"), ("tile", 7))),      # the documented refusal of 5x5 / stride 1
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 64, "f32", (("entry", "fwd"), ("tile", 1))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 64, "f32", (("entry", "fwd"), ("tile", 4))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 128, "f32", (("entry", "fwd"), ("tile", 7))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 128, "f32", (("entry", "fwd"), ("tile", 9))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 128, "bf16", (("entry", "fwd"), ("tile", 8))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 64, "bf16", (("entry", "fwd"), ("tile", 7))),
    run("fwd", K5S2, "ints", 2, 9, 11, 32, 64, "bf16", (("entry", "fwd"), ("tile", 9))),
    run("fwd", Geometry(5, 1, 2), "ints", 2, 9, 11, 32, 128, "bf16", (("entry", "fwd"), ("tile", 9))),
    run("fwd", K7S2, "ints", 2, 9, 11, 8, 64, "f32", (("entry", "fwd"), ("tile", 4))),
    run("fwd", K3S1, "ints", 2, 9, 11, 32, 64, "f32", (("entry", "fwd"), ("tile", 6))),
    run("fwd", Geometry(3, 1, 0), "ints", 2, 2, 9, 32, 128, "f32", (("entry", "fwd"), ("tile", 3))),           # an empty output at pad 0
    run("fwd", Geometry(5, 2, 0), "ints", 2, 9, 4, 32, 128, "bf16", (("entry", "fwd"), ("tile", 9))),
    run("dgrad", K3S1, "ints", 2, 9, 11, 128, 64, "f32", (("entry", "dgrad"), ("tile", 7), ("splits", 1))),
    run("dgrad", K3S1, "ints", 2, 9, 11, 64, 64, "bf16", (("entry", "dgrad"), ("tile", 7), ("splits", 1))),
    run("dgrad", K3S1, "ints", 2, 9, 11, 32, 64, "bf16", (("entry", "dgrad"), ("tile", 4), ("splits", 1))),
    run("dgrad", K3S2, "ints", 2, 9, 11, 128, 64, "bf16", (("entry", "dgrad"), ("tile", 7), ("splits", 1))),
    run("dgrad", K3S2, "ints", 2, 9, 11, 64, 64, "bf16", (("entry", "lrelu"), ("accumulate_db", False)), fold=True),
    run("wgrad", K3S1, "ints", 2, 9, 11, 32, 64, "f32", (("entry", "wgrad"), ("splits", 2), ("dz_coff", 0), ("clamped", 2)), accumulate=True),
    run("wgrad", K3S1, "ints", 2, 9, 11, 32, 64, "bf16", (("entry", "wgrad"), ("splits", 100), ("dz_coff", 4), ("clamped", 7)), accumulate=True),
    run("wgrad", K3S1, "ints", 1, 30, 40, 32, 128, "bf16", (("entry", "wgrad"), ("splits", 1), ("dz_coff", 0), ("patch", True), ("clamped", 1)), accumulate=True),
    run("deconv", DECONV, "ints", 2, 5, 6, 32, 128, "f32", (("entry", "deconv"), ("tile", 9)), window=(10, 12)),
]


@pytest.mark.parametrize("r", REFUSALS, ids=lambda r: "-".join([r.key[0], ident(r.key[1]), r.pipe] + ["%s%s" % kv for kv in r.how[1:]]))
def test_documented_refusals(ops, r):
    """each of these is refused with DIM_ERR_ARG before anything is enqueued: the output keeps its sentinel, the workspace its NaN"""
    assert refusal(r) is not None
    assert Runner(ops)(r) is False, describe(r)
