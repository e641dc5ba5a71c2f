"""csrc/zoom.hip dim_zoom_planes_src / dim_zoom_net_input_src (planes of a source size sampled into the network size) through their
lib.hip.ops wrappers against tests/source_size_reference.py, which tests/test_source_size_host.py pins to the oracle's GridGenerator +
BilinearSampler restatement.  Small size pairs that reach every launch path; B = 5 zoom factors with windows hanging off the source
and the 1e30 factor.  Un-rounded lanes are compared exactly; rounded lanes exactly too (`rounded_same` reports how many reference
values sit within one float32 ulp of a rounding boundary, and allows no difference in the end)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import source_size_reference as R  # noqa: E402

DEV = "cuda:0"
SENT = -777.25          # no kernel output takes this value
GUARD = 64
f32 = np.float32
PAIR_IDS = ["{}x{}to{}x{}".format(s[0], s[1], n[0], n[1]) for s, n in R.SIZE_PAIRS]


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

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.flat[:self.n].view(shape)

    def get(self, what):
        a = host(self.flat)
        assert np.all(a[self.n:] == SENT), what + ": wrote past its end"
        return a[:self.n].reshape(tuple(self.t.shape))

    def untouched(self, what):
        assert np.all(self.get(what) == SENT), what + ": a skipped output was written"


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


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS, ids=PAIR_IDS)
def test_zoom_planes_src(ops, src, net):
    """dim_zoom_planes_src over every pre x post x add3"""
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
            want, before = R.zoom_planes_src(x, zf, Hn, Wn, pre=pre, post=post, add3=add3)
            assert np.all(np.isfinite(want))
            xt = dev(x)
            out = Out((x.shape[0], x.shape[1], Hn, Wn))
            ops.zoom_planes_src(xt, zft, pre=pre, post=post, add3=add3, out=out.t)
            what = "zoom_planes_src {}->{} add3={} pre={} post={}".format(src, net, add3 is not None, pre, post)
            got = out.get(what)
            if post == 0:
                same(got, want, what)
            else:
                rounded_same(got, want, before, what)
            same(host(xt), x, what + ": the input is not written")
            n += 1
    assert n == 12
    # the output allocated by the wrapper from net_size
    y = ops.zoom_planes_src(dev(x4), zft, net_size=(Hn, Wn))
    assert tuple(y.shape) == (R.ZOOM_B, 4, Hn, Wn)
    same(host(y), R.zoom_planes_src(x4, zf, Hn, Wn)[0], "zoom_planes_src net_size")


@pytest.mark.parametrize("src,net", R.SIZE_PAIRS, ids=PAIR_IDS)
def test_zoom_net_input_src(ops, src, net):
    """dim_zoom_net_input_src: modes 0-3, every lane of X, with and without the four NCHW outputs"""
    (Hs, Ws), (Hn, Wn) = src, net
    inp = R.zoom_inputs(Hs, Ws)
    zf, means, B = R.ZOOM_FACTORS, R.ZOOM_MEANS, R.ZOOM_B
    io, ir, zft = dev(inp["io"]), dev(inp["ir"]), dev(zf)
    tag = "zoom_net_input_src {}->{}".format(src, net)
    with np.errstate(over="ignore", invalid="ignore"):
        for name, eo, er in (("depth-like", inp["depth_like"], inp["depth_like"]), ("binary", inp["binary"], inp["depth_like"])):
            ref = R.net_input_src(inp["io"], inp["ir"], eo, er, zf, means, 0, Hn, Wn)
            eot, ert = dev(eo), dev(er)
            X = Out((B, Hn, Wn, 8))
            nchw = [Out((B, 3, Hn, Wn)), Out((B, 3, Hn, Wn)), Out((B, 1, Hn, Wn)), Out((B, 1, Hn, Wn))]
            ops.zoom_net_input_src(io, ir, eot, ert, zft, means, 0, X=X.t, nchw_out=tuple(o.t for o in nchw))
            got = X.get(tag)
            same(got[..., :6], ref["X"][..., :6], "{} {} X[0:6]".format(tag, name))
            for lane, k in ((6, 0), (7, 1)):
                rounded_same(got[..., lane], ref["X"][..., lane], ref["pre_round"][k][:, 0], "{} {} X[{}]".format(tag, name, lane))
            same(nchw[0].get(tag), ref["nchw"][0], "{} {} z_image_observed".format(tag, name))
            same(nchw[1].get(tag), ref["nchw"][1], "{} {} z_image_rendered".format(tag, name))
            rounded_same(nchw[2].get(tag), ref["nchw"][2], ref["pre_round"][0], "{} {} z_mask_observed".format(tag, name))
            rounded_same(nchw[3].get(tag), ref["nchw"][3], ref["pre_round"][1], "{} {} z_mask_rendered".format(tag, name))
            X2 = Out((B, Hn, Wn, 8))
            ops.zoom_net_input_src(io, ir, eot, ert, zft, means, 0, X=X2.t)                 # no NCHW outputs
            np.testing.assert_array_equal(bits(X2.get(tag)), bits(got))
            r2 = R.net_input_src(inp["io"], inp["ir"], eo, er, zf, means, 2, Hn, Wn)["X"]
            X2 = Out((B, Hn, Wn, 8))
            ops.zoom_net_input_src(io, ir, eot, ert, zft, means, 2, X=X2.t)
            same(X2.get(tag), r2, "{} {} mode 2".format(tag, name))
            r3 = R.net_input_src(inp["io"], inp["ir"], eo, er, zf, means, 3, Hn, Wn)
            X3 = Out((B, Hn, Wn, 8))
            ops.zoom_net_input_src(io, ir, eot, ert, zft, means, 3, X=X3.t)
            g3 = X3.get(tag)
            rounded_same(g3[..., 0], r3["X"][..., 0], r3["pre_round"][0][:, 0], "{} {} mode 3 lane 0".format(tag, name))
            rounded_same(g3[..., 1], r3["X"][..., 1], r3["pre_round"][1][:, 0], "{} {} mode 3 lane 1".format(tag, name))
            same(g3[..., 2:], np.zeros_like(g3[..., 2:]), "{} {} mode 3 lanes 2-7".format(tag, name))
        r1 = R.net_input_src(inp["io"], inp["ir"], None, None, zf, means, 1, Hn, Wn)["X"]
        for extra in ((None, None), (dev(inp["binary"]), dev(inp["depth_like"]))):
            X1 = Out((B, Hn, Wn, 8))
            ops.zoom_net_input_src(io, ir, extra[0], extra[1], zft, means, 1, X=X1.t)
            same(X1.get(tag), r1, "{} mode 1".format(tag))
    same(host(io), inp["io"], tag + ": the inputs are not written")


def test_equal_sizes_equal_the_same_size_entry_points(ops):
    """with (16,36)->(16,36) the _src entry points give the bits of dim_zoom_net_input / _ex / dim_zoom_planes"""
    H, W = R.SAME_SIZE
    inp = R.zoom_inputs(H, W)
    zf, means, B = R.ZOOM_FACTORS, R.ZOOM_MEANS, R.ZOOM_B
    io, ir, eo, er, zft = dev(inp["io"]), dev(inp["ir"]), dev(inp["binary"]), dev(inp["depth_like"]), dev(zf)
    old = [Out((B, 3, H, W)), Out((B, 3, H, W)), Out((B, 1, H, W)), Out((B, 1, H, W))]
    new = [Out((B, 3, H, W)), Out((B, 3, H, W)), Out((B, 1, H, W)), Out((B, 1, H, W))]
    Xo, Xn = Out((B, H, W, 8)), Out((B, H, W, 8))
    ops.zoom_net_input(io, ir, eo, er, zft, means, X=Xo.t, nchw_out=tuple(o.t for o in old))
    ops.zoom_net_input_src(io, ir, eo, er, zft, means, 0, X=Xn.t, nchw_out=tuple(o.t for o in new))
    np.testing.assert_array_equal(bits(Xn.get("X")), bits(Xo.get("X")))
    for a, b in zip(new, old):
        np.testing.assert_array_equal(bits(a.get("nchw")), bits(b.get("nchw")))
    for mode in (0, 1, 2, 3):
        Xo, Xn = Out((B, H, W, 8)), Out((B, H, W, 8))
        ops.zoom_net_input_ex(io, ir, eo, er, zft, means, mode, X=Xo.t)
        ops.zoom_net_input_src(io, ir, eo, er, zft, means, mode, X=Xn.t)
        np.testing.assert_array_equal(bits(Xn.get("X")), bits(Xo.get("X")), err_msg="mode {}".format(mode))
    x4 = dev(np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1))
    for add3, pre, post in itertools.product((None, means), (0, 1), (0, 1, 2)):
        x = io if add3 is not None else x4
        yo, yn = Out(tuple(x.shape)), Out(tuple(x.shape))
        ops.zoom_planes(x, zft, pre=pre, post=post, add3=add3, out=yo.t)
        ops.zoom_planes_src(x, zft, pre=pre, post=post, add3=add3, out=yn.t)
        np.testing.assert_array_equal(bits(yn.get("y")), bits(yo.get("y")), err_msg="planes pre={} post={}".format(pre, post))


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
    with pytest.raises(DeepIMHipError, match="all four"):
        ops.zoom_net_input_src(io, ir, m, m, zft, R.ZOOM_MEANS, 0, X=X.t, nchw_out=(torch.empty((B, 3, Hn, Wn), device=DEV), None, None, None))
    for mode in (0, 2, 3):
        with pytest.raises(DeepIMHipError, match="extra planes"):
            ops.zoom_net_input_src(io, ir, None, None, zft, R.ZOOM_MEANS, mode, X=X.t)
    with pytest.raises(DeepIMHipError, match="mode"):
        ops.zoom_net_input_src(io, ir, m, m, zft, R.ZOOM_MEANS, 4, X=X.t)
    with pytest.raises(DeepIMHipError, match="pre must be"):
        ops.zoom_planes_src(m, zft, pre=2, out=y.t)
    with pytest.raises(DeepIMHipError, match="post must be"):
        ops.zoom_planes_src(m, zft, post=3, out=y.t)
    # the wrappers refuse tensors whose shapes disagree before anything reaches the library
    with pytest.raises(ValueError, match="X must have shape"):
        ops.zoom_net_input_src(io, ir, m, m, zft, R.ZOOM_MEANS, 0, X=X.t, net_size=(Hn + 1, Wn))
    with pytest.raises(ValueError, match="image_rendered"):
        ops.zoom_net_input_src(io, ir[:, :, :-1].contiguous(), m, m, zft, R.ZOOM_MEANS, 0, X=X.t)
    # the entry points themselves: null pointers and sizes below 2 give DIM_ERR_ARG and a message, and launch nothing
    lib, st = capi.lib(), capi.current_stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    mp = capi.host_f32(R.ZOOM_MEANS, 3)
    calls = [
        lambda: lib.dim_zoom_planes_src(None, p(zft), p(y.t), B, 1, Hs, Ws, Hn, Wn, 0, 0, None, st),
        lambda: lib.dim_zoom_planes_src(p(m), p(zft), None, B, 1, Hs, Ws, Hn, Wn, 0, 0, None, st),
        lambda: lib.dim_zoom_planes_src(p(m), p(zft), p(y.t), B, 1, 1, Ws, Hn, Wn, 0, 0, None, st),
        lambda: lib.dim_zoom_planes_src(p(m), p(zft), p(y.t), B, 1, Hs, Ws, Hn, 1, 0, 0, None, st),
        lambda: lib.dim_zoom_net_input_src(p(io), p(ir), p(m), p(m), p(zft), None, B, Hs, Ws, Hn, Wn, mp[1], 0, None, None, None, None, st),
        lambda: lib.dim_zoom_net_input_src(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, Ws, Hn, Wn, None, 0, None, None, None, None, st),
        lambda: lib.dim_zoom_net_input_src(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, 1, Hn, Wn, mp[1], 0, None, None, None, None, st),
        lambda: lib.dim_zoom_net_input_src(p(io), p(ir), p(m), p(m), p(zft), p(X.t), B, Hs, Ws, 0, Wn, mp[1], 0, None, None, None, None, st),
    ]
    for call in calls:
        rc = call()
        assert rc != 0
        msg = lib.dim_last_error().decode()
        assert "null pointer" in msg or ">= 2" in msg, msg
    X.untouched("rejected zoom_net_input_src"), y.untouched("rejected zoom_planes_src")
