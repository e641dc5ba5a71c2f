"""csrc/zoom.hip dim_zoom_planes_area / dim_zoom_net_input_area / dim_zoom_area_taps (the zoom with an area filter for windows that
shrink the source) through their lib.hip.ops wrappers against tests/area_zoom_reference.py, which tests/test_area_zoom_host.py pins to
the oracle's BilinearSampler on shifted grids.  The size pairs of tests/source_size_reference.py; B = 9 zoom factors that reach tap
counts (1,1), (2,2), (3,3), unequal ones and the max_taps clamp.  Un-rounded lanes are compared exactly; rounded lanes exactly too
(`rounded_same` reports how many reference values sit within one float32 ulp of a rounding boundary, and allows no difference in the
end) -- the criteria of tests/test_gpu_source_size_kernels.py."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import area_zoom_reference as R  # noqa: E402
import source_size_reference as S  # noqa: E402

DEV = "cuda:0"
SENT = -777.25          # no kernel output takes this value
GUARD = 64
f32 = np.float32
PAIR_IDS = ["{}x{}to{}x{}".format(s[0], s[1], n[0], n[1]) for s, n in R.SIZE_PAIRS]
T = R.MAX_TAPS


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Out:
    """an output tensor pre-filled with a sentinel, followed by guard words that no kernel may touch"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.flat[:self.n].view(shape)
        self.sent = host(self.flat)[0]

    def get(self, what):
        a = host(self.flat)
        assert np.all(a[self.n:] == self.sent), what + ": wrote past its end"
        return a[:self.n].reshape(tuple(self.t.shape))

    def untouched(self, what):
        assert np.all(self.get(what) == self.sent), what + ": a skipped output was written"


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    print("{}: {} of {} differ, worst {:.3g}".format(what, bad, got.size, worst))
    np.testing.assert_array_equal(got, want, err_msg=what)


def rounded_same(got, want, before, what):
    """a rounded output: got may differ from the reference only where the reference's value before rounding lies within one float32 ulp
    of a rounding boundary -- and with bit-equal samples in front of it, nowhere"""
    diff = got != want
    near = R.round_boundary_distance_ulps(before) <= 1.0
    print("{}: {} of {} differ ({} away from a boundary); {} reference values within 1 ulp of a boundary".format(
        what, int(diff.sum()), diff.size, int((diff & ~near).sum()), int(near.sum())))
    assert not (diff & ~near).any(), what
    assert not diff.any(), what


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def refs():
    """the restatement's network inputs, computed once per (size pair, extra planes, mode) and shared"""
    cache = {}

    def get(src, net, name, mode):
        key = (src, net, name, mode)
        if key not in cache:
            inp = R.zoom_inputs(*src)
            eo, er = {"depth-like": (inp["depth_like"], inp["depth_like"]), "binary": (inp["binary"], inp["depth_like"]),
                      "none": (None, None)}[name]
            with np.errstate(over="ignore", invalid="ignore"):
                cache[key] = R.net_input_area(inp["io"], inp["ir"], eo, er, R.ZOOM_FACTORS, R.ZOOM_MEANS, mode, net[0], net[1], T)
        return cache[key]
    return get


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS, ids=PAIR_IDS)
def test_zoom_planes_area(ops, src, net):
    """dim_zoom_planes_area over every pre x post x add3"""
    (Hs, Ws), (Hn, Wn) = src, net
    inp = R.zoom_inputs(Hs, Ws)
    zf = R.ZOOM_FACTORS
    x3 = inp["io"]
    x4 = np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1)
    zft = dev(zf)
    n = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for add3, pre, post in itertools.product((None, R.ZOOM_MEANS), (0, 1), (0, 1, 2)):
            x = x3 if add3 is not None else x4            # C = 4 also takes the `C > 3: no constants` path
            want, before = R.zoom_planes_area(x, zf, Hn, Wn, T, pre=pre, post=post, add3=add3)
            assert np.all(np.isfinite(want))
            xt = dev(x)
            out = Out((x.shape[0], x.shape[1], Hn, Wn))
            ops.zoom_planes_area(xt, zft, pre=pre, post=post, add3=add3, out=out.t, max_taps=T)
            what = "zoom_planes_area {}->{} add3={} pre={} post={}".format(src, net, add3 is not None, pre, post)
            got = out.get(what)
            if post == 0:
                same(got, want, what)
            else:
                rounded_same(got, want, before, what)
            same(host(xt), x, what + ": the input is not written")
            n += 1
    assert n == 12
    # the output allocated by the wrapper from net_size
    y = ops.zoom_planes_area(dev(x4), zft, net_size=(Hn, Wn), max_taps=T)
    assert tuple(y.shape) == (R.ZOOM_B, 4, Hn, Wn)
    same(host(y), R.zoom_planes_area(x4, zf, Hn, Wn, T)[0], "zoom_planes_area net_size")


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS, ids=PAIR_IDS)
def test_zoom_net_input_area(ops, refs, src, net):
    """dim_zoom_net_input_area: modes 0-3, every lane of X, with and without the four NCHW outputs"""
    (Hs, Ws), (Hn, Wn) = src, net
    inp = R.zoom_inputs(Hs, Ws)
    zf, means, B = R.ZOOM_FACTORS, R.ZOOM_MEANS, R.ZOOM_B
    io, ir, zft = dev(inp["io"]), dev(inp["ir"]), dev(zf)
    tag = "zoom_net_input_area {}->{}".format(src, net)
    for name, eo, er in (("depth-like", inp["depth_like"], inp["depth_like"]), ("binary", inp["binary"], inp["depth_like"])):
        ref = refs(src, net, name, 0)
        eot, ert = dev(eo), dev(er)
        X = Out((B, Hn, Wn, 8))
        nchw = [Out((B, 3, Hn, Wn)), Out((B, 3, Hn, Wn)), Out((B, 1, Hn, Wn)), Out((B, 1, Hn, Wn))]
        ops.zoom_net_input_area(io, ir, eot, ert, zft, means, 0, X=X.t, nchw_out=tuple(o.t for o in nchw), max_taps=T)
        got = X.get(tag)
        same(got[..., :6], ref["X"][..., :6], "{} {} X[0:6]".format(tag, name))
        for lane, k in ((6, 0), (7, 1)):
            rounded_same(got[..., lane], ref["X"][..., lane], ref["pre_round"][k][:, 0], "{} {} X[{}]".format(tag, name, lane))
        same(nchw[0].get(tag), ref["nchw"][0], "{} {} z_image_observed".format(tag, name))
        same(nchw[1].get(tag), ref["nchw"][1], "{} {} z_image_rendered".format(tag, name))
        rounded_same(nchw[2].get(tag), ref["nchw"][2], ref["pre_round"][0], "{} {} z_mask_observed".format(tag, name))
        rounded_same(nchw[3].get(tag), ref["nchw"][3], ref["pre_round"][1], "{} {} z_mask_rendered".format(tag, name))
        X2 = Out((B, Hn, Wn, 8))
        ops.zoom_net_input_area(io, ir, eot, ert, zft, means, 0, X=X2.t, max_taps=T)                 # no NCHW outputs
        np.testing.assert_array_equal(bits(X2.get(tag)), bits(got))
        r2 = refs(src, net, name, 2)["X"]
        X2 = Out((B, Hn, Wn, 8))
        ops.zoom_net_input_area(io, ir, eot, ert, zft, means, 2, X=X2.t, max_taps=T)
        same(X2.get(tag), r2, "{} {} mode 2".format(tag, name))
        r3 = refs(src, net, name, 3)
        X3 = Out((B, Hn, Wn, 8))
        ops.zoom_net_input_area(io, ir, eot, ert, zft, means, 3, X=X3.t, max_taps=T)
        g3 = X3.get(tag)
        rounded_same(g3[..., 0], r3["X"][..., 0], r3["pre_round"][0][:, 0], "{} {} mode 3 lane 0".format(tag, name))
        rounded_same(g3[..., 1], r3["X"][..., 1], r3["pre_round"][1][:, 0], "{} {} mode 3 lane 1".format(tag, name))
        same(g3[..., 2:], np.zeros_like(g3[..., 2:]), "{} {} mode 3 lanes 2-7".format(tag, name))
        same(host(eot), eo, tag + ": the extra planes are not written")
    r1 = refs(src, net, "none", 1)["X"]
    for extra in ((None, None), (dev(inp["binary"]), dev(inp["depth_like"]))):
        X1 = Out((B, Hn, Wn, 8))
        ops.zoom_net_input_area(io, ir, extra[0], extra[1], zft, means, 1, X=X1.t, max_taps=T)
        same(X1.get(tag), r1, "{} mode 1".format(tag))
    same(host(io), inp["io"], tag + ": image_observed is not written")
    same(host(ir), inp["ir"], tag + ": image_rendered is not written")
    same(host(zft), zf, tag + ": the zoom factor is not written")


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS + ((S.SAME_SIZE, S.SAME_SIZE),), ids=PAIR_IDS + ["same-size"])
def test_one_tap_gives_the_bits_of_the_src_entry_points(ops, src, net):
    """max_taps = 1: every output's bits equal dim_zoom_net_input_src / dim_zoom_planes_src, for every factor.  max_taps = 4: the rows
    of the batch whose taps are (1,1) equal the `_src` outputs bit for bit, the others differ"""
    (Hs, Ws), (Hn, Wn) = src, net
    inp = R.zoom_inputs(Hs, Ws)
    zf, means, B = R.ZOOM_FACTORS, R.ZOOM_MEANS, R.ZOOM_B
    io, ir, eo, er, zft = dev(inp["io"]), dev(inp["ir"]), dev(inp["binary"]), dev(inp["depth_like"]), dev(zf)
    n_xy = R.taps(zf, Hs, Ws, Hn, Wn, T)
    one = [b for b in range(B) if tuple(n_xy[b]) == (1, 1)]
    more = [b for b in range(B) if tuple(n_xy[b]) != (1, 1) and b not in (3, 4)]   # (rows 3 and 4, far outside and 1e30, read nothing)
    assert one and (more or (Hs, Ws) == (6, 8) or src == net)

    def rows(a, idx):
        return bits(a)[idx]

    def check(new_t, old, what):
        """new_t[1], new_t[T]: Out of the area entry point at max_taps 1 and T"""
        o, n1, n4 = old.get(what), new_t[1].get(what), new_t[T].get(what)
        np.testing.assert_array_equal(bits(n1), bits(o), err_msg=what + " max_taps 1")
        np.testing.assert_array_equal(rows(n4, one), rows(o, one), err_msg=what + " max_taps 4, rows with taps (1,1)")
        for b in more:
            assert (bits(n4)[b] != bits(o)[b]).any(), "{}: row {} with taps {} equals the bilinear output".format(what, b, n_xy[b])

    old = [Out((B, 3, Hn, Wn)), Out((B, 3, Hn, Wn)), Out((B, 1, Hn, Wn)), Out((B, 1, Hn, Wn))]
    Xo = Out((B, Hn, Wn, 8))
    ops.zoom_net_input_src(io, ir, eo, er, zft, means, 0, X=Xo.t, nchw_out=tuple(o.t for o in old))
    new, Xn = {}, {}
    for t in (1, T):
        new[t] = [Out((B, 3, Hn, Wn)), Out((B, 3, Hn, Wn)), Out((B, 1, Hn, Wn)), Out((B, 1, Hn, Wn))]
        Xn[t] = Out((B, Hn, Wn, 8))
        ops.zoom_net_input_area(io, ir, eo, er, zft, means, 0, X=Xn[t].t, nchw_out=tuple(o.t for o in new[t]), max_taps=t)
    check(Xn, Xo, "X mode 0")
    for k in (0, 1):                       # the images (the masks of a row with more taps may round to the same 0 / 1 everywhere)
        check({t: new[t][k] for t in new}, old[k], "nchw {}".format(k))
    for k in (2, 3):
        np.testing.assert_array_equal(bits(new[1][k].get("nchw")), bits(old[k].get("nchw")))
        np.testing.assert_array_equal(rows(new[T][k].get("nchw"), one), rows(old[k].get("nchw"), one))
    for mode in (1, 2, 3):
        Xo, Xn = Out((B, Hn, Wn, 8)), {1: Out((B, Hn, Wn, 8)), T: Out((B, Hn, Wn, 8))}
        ops.zoom_net_input_src(io, ir, eo, er, zft, means, mode, X=Xo.t)
        for t in (1, T):
            ops.zoom_net_input_area(io, ir, eo, er, zft, means, mode, X=Xn[t].t, max_taps=t)
        if mode == 3:
            np.testing.assert_array_equal(bits(Xn[1].get("X")), bits(Xo.get("X")))
            np.testing.assert_array_equal(rows(Xn[T].get("X"), one), rows(Xo.get("X"), one))
        else:
            check(Xn, Xo, "X mode {}".format(mode))
    x4 = dev(np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1))
    for add3, pre, post in itertools.product((None, means), (0, 1), (0, 1, 2)):
        x = io if add3 is not None else x4
        shape = (B, x.shape[1], Hn, Wn)
        yo, yn = Out(shape), {1: Out(shape), T: Out(shape)}
        ops.zoom_planes_src(x, zft, pre=pre, post=post, add3=add3, out=yo.t)
        for t in (1, T):
            ops.zoom_planes_area(x, zft, pre=pre, post=post, add3=add3, out=yn[t].t, max_taps=t)
        if pre == 0 and post == 0:
            check(yn, yo, "planes add3={}".format(add3 is not None))
        else:
            np.testing.assert_array_equal(bits(yn[1].get("y")), bits(yo.get("y")), err_msg="planes pre={} post={}".format(pre, post))
            np.testing.assert_array_equal(rows(yn[T].get("y"), one), rows(yo.get("y"), one))


def test_zoom_area_taps(ops):
    """dim_zoom_area_taps == taps() on the factor table at every size pair and max_taps, and on the boundary cases of the host test"""
    zft = dev(R.ZOOM_FACTORS)
    for (src, net), max_taps in itertools.product(R.SIZE_PAIRS, (1, 2, T, 8)):
        out = Out((R.ZOOM_B, 2), torch.int32)
        ops.zoom_area_taps(zft, src, net, max_taps, out=out.t)
        np.testing.assert_array_equal(out.get("taps"), R.taps(R.ZOOM_FACTORS, *src, *net, max_taps), err_msg=str((src, net, max_taps)))
    zf, want = R.boundary_cases()
    src, net = R.BOUNDARY_SIZES
    got = host(ops.zoom_area_taps(dev(zf), src, net, R.BOUNDARY_MAX_TAPS))
    assert got.dtype == np.int32
    print("boundary taps", got.T.tolist())
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, R.taps(zf, *src, *net, R.BOUNDARY_MAX_TAPS))
    same(host(zft), R.ZOOM_FACTORS, "the zoom factor is not written")


def test_the_boundary_factors_sample_with_their_counts(ops):
    """the sampler itself takes the counts of dim_zoom_area_taps at the boundaries (NaN, inf and 1e30 windows aside, whose samples
    are not finite or read nothing): the planes equal the restatement run with those counts"""
    zf, want = R.boundary_cases()
    keep = np.isfinite(zf).all(axis=1) & (np.abs(zf[:, 0]) < 1e29)
    zf, want = zf[keep], want[keep]
    (Hs, Ws), (Hn, Wn) = R.BOUNDARY_SIZES
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, size=(len(zf), 2, Hs, Ws)).astype(f32)
    ref = R.zoom_sample_area(x, zf, Hn, Wn, R.BOUNDARY_MAX_TAPS)
    np.testing.assert_array_equal(R.taps(zf, Hs, Ws, Hn, Wn, R.BOUNDARY_MAX_TAPS), want)
    out = Out(ref.shape)
    ops.zoom_planes_area(dev(x), dev(zf), out=out.t, max_taps=R.BOUNDARY_MAX_TAPS)
    same(out.get("boundary"), ref, "zoom_planes_area at the tap boundaries")
    # one count less or more is another output: the comparison above does tell the counts apart
    for b in (0, 1):
        other = R.zoom_sample_area(x[b:b + 1], zf[b:b + 1], Hn, Wn, n_xy=want[b:b + 1] + 1)
        assert (other != ref[b:b + 1]).any()


@pytest.mark.parametrize("src,net", R.STRIPE_PAIRS, ids=["24x32to12x16", "48x64to12x16"])
def test_stripes_finer_than_a_network_pixel_come_out_grey(ops, src, net):
    """the stripe assertion of tests/test_area_zoom_host.py on the device's output"""
    x, zft = dev(R.stripe_source(*src)), dev(R.FULL_FRAME)
    area = host(ops.zoom_planes_area(x, zft, net_size=net, max_taps=T))
    bil = host(ops.zoom_planes_src(x, zft, net_size=net))
    R.check_stripes(area, bil, "device {}->{}".format(src, net))
    same(area, R.zoom_sample_area(R.stripe_source(*src), R.FULL_FRAME, *net, T), "stripes against the restatement")


def test_bad_arguments_return_the_error_code_with_a_message(ops):
    import ctypes

    from lib.hip import capi
    from lib.hip.capi import DeepIMHipError

    (Hs, Ws), (Hn, Wn) = R.SIZE_PAIRS[0]
    inp = R.zoom_inputs(Hs, Ws)
    io, ir, m, zft = dev(inp["io"]), dev(inp["ir"]), dev(inp["binary"]), dev(R.ZOOM_FACTORS)
    B = R.ZOOM_B
    X = Out((B, Hn, Wn, 8))
    y = Out((B, 1, Hn, Wn))
    taps = Out((B, 2), torch.int32)
    for bad in (0, 9, -1):
        with pytest.raises(DeepIMHipError, match="max_taps"):
            ops.zoom_net_input_area(io, ir, m, m, zft, R.ZOOM_MEANS, 0, X=X.t, max_taps=bad)
        with pytest.raises(DeepIMHipError, match="max_taps"):
            ops.zoom_planes_area(m, zft, out=y.t, max_taps=bad)
        with pytest.raises(DeepIMHipError, match="max_taps"):
            ops.zoom_area_taps(zft, (Hs, Ws), (Hn, Wn), bad, out=taps.t)
    with pytest.raises(DeepIMHipError, match="all four"):
        ops.zoom_net_input_area(io, ir, m, m, zft, R.ZOOM_MEANS, 0, X=X.t, nchw_out=(torch.empty((B, 3, Hn, Wn), device=DEV), None, None, None))
    for mode in (0, 2, 3):
        with pytest.raises(DeepIMHipError, match="extra planes"):
            ops.zoom_net_input_area(io, ir, None, None, zft, R.ZOOM_MEANS, mode, X=X.t)
    with pytest.raises(DeepIMHipError, match="mode"):
        ops.zoom_net_input_area(io, ir, m, m, zft, R.ZOOM_MEANS, 4, X=X.t)
    with pytest.raises(DeepIMHipError, match="pre must be"):
        ops.zoom_planes_area(m, zft, pre=2, out=y.t)
    with pytest.raises(DeepIMHipError, match="post must be"):
        ops.zoom_planes_area(m, zft, post=3, out=y.t)
    # the wrappers refuse tensors whose shapes disagree before anything reaches the library
    with pytest.raises(ValueError, match="X must have shape"):
        ops.zoom_net_input_area(io, ir, m, m, zft, R.ZOOM_MEANS, 0, X=X.t, net_size=(Hn + 1, Wn))
    with pytest.raises(ValueError, match="image_rendered"):
        ops.zoom_net_input_area(io, ir[:, :, :-1].contiguous(), m, m, zft, R.ZOOM_MEANS, 0, X=X.t)
    with pytest.raises(ValueError, match="out must have shape"):
        ops.zoom_area_taps(zft, (Hs, Ws), (Hn, Wn), T, out=torch.empty((B, 3), dtype=torch.int32, device=DEV))
    # the entry points themselves: null pointers and sizes below 2 give DIM_ERR_ARG and a message, and launch nothing
    lib, st = capi.lib(), capi.current_stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    mp = capi.host_f32(R.ZOOM_MEANS, 3)
    calls = [
        lambda: lib.dim_zoom_planes_area(None, p(zft), p(y.t), B, 1, Hs, Ws, Hn, Wn, 0, 0, None, T, st),
        lambda: lib.dim_zoom_planes_area(p(m), p(zft), None, B, 1, Hs, Ws, Hn, Wn, 0, 0, None, T, st),
        lambda: lib.dim_zoom_planes_area(p(m), p(zft), p(y.t), B, 1, 1, Ws, Hn, Wn, 0, 0, None, T, st),
        lambda: lib.dim_zoom_planes_area(p(m), p(zft), p(y.t), B, 1, Hs, Ws, Hn, 1, 0, 0, None, T, st),
        lambda: lib.dim_zoom_net_input_area(p(io), p(ir), p(m), p(m), p(zft), None, B, Hs, Ws, Hn, Wn, mp[1], 0, None, None, None, None, T, st),
        lambda: lib.dim_zoom_net_input_area(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, Ws, Hn, Wn, None, 0, None, None, None, None, T, st),
        lambda: lib.dim_zoom_net_input_area(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, 1, Hn, Wn, mp[1], 0, None, None, None, None, T, st),
        lambda: lib.dim_zoom_net_input_area(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, Ws, 0, Wn, mp[1], 0, None, None, None, None, T, st),
        lambda: lib.dim_zoom_area_taps(None, B, Hs, Ws, Hn, Wn, T, p(taps.t), st),
        lambda: lib.dim_zoom_area_taps(p(zft), B, Hs, Ws, Hn, Wn, T, None, st),
        lambda: lib.dim_zoom_area_taps(p(zft), B, Hs, Ws, 1, Wn, T, p(taps.t), st),
    ]
    for call in calls:
        rc = call()
        assert rc == -1
        msg = lib.dim_last_error().decode()
        assert "null pointer" in msg or ">= 2" in msg, msg
    assert lib.dim_zoom_planes_area(p(m), p(zft), p(y.t), B, 1, Hs, Ws, Hn, Wn, 0, 0, None, 9, st) == -1
    assert "max_taps" in lib.dim_last_error().decode()
    X.untouched("rejected zoom_net_input_area"), y.untouched("rejected zoom_planes_area"), taps.untouched("rejected zoom_area_taps")
