"""The per-pixel kernels that build the network's inputs and labels, each through its lib.hip.ops wrapper against the plain restatement of
tests/pixel_kernels_reference.py, at the smallest shapes that still reach every launch path (partial blocks, dead waves, widths that
are no multiple of the block, several blocks per row):

  csrc/data.hip   dim_test_blobs_from_raw, dim_pair_blobs_from_raw, dim_mask_dilate, dim_calc_flow_labels, dim_point_clouds
  csrc/zoom.hip   dim_mask_bbox, dim_zoom_factor, dim_zoom_planes, dim_zoom_net_input, dim_zoom_net_input_ex

tests/test_pixel_kernels_host.py pins the restatements to the project's host code and shows that these inputs separate every named
mutant.  Integer and single-rounded float32 outputs are compared exactly; float64-then-rounded outputs to one float32 ulp."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pixel_kernels_reference as R  # noqa: E402

DEV = "cuda:0"
SENT = -777.25          # no kernel output takes this value
ISENT = -99
GUARD = 64
f32 = np.float32


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from lib.hip import ops as o

    return o


def dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.as_tensor(a).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


class Out:
    """an output tensor pre-filled with a sentinel, followed by guard words that no kernel may touch"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.fill = ISENT if dtype == torch.int32 else SENT
        self.flat = torch.full((self.n + GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.flat[:self.n].view(shape)

    def get(self, what):
        a = host(self.flat)
        assert np.all(a[self.n:] == self.fill), what + ": wrote past its end"
        return a[:self.n].reshape(tuple(self.t.shape))

    def untouched(self, what):
        assert np.all(self.get(what) == self.fill), what + ": a skipped output was written"


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    print("{}: {} of {} differ, worst {:.3g}".format(what, bad, got.size, worst))
    np.testing.assert_array_equal(got, want, err_msg=what)


# ------------------------------------------------------------------------------------------------ raw pixels -> blobs
BLOB_OUT_SHAPES = {"image_observed": 3, "image_rendered": 3, "mask_rendered": 1, "depth_rendered": 1, "depth_a_out": 1, "depth_b_out": 1,
                   "mask_label": 1, "label_raw": 1, "bbox_ren": 0, "bbox_label": 0}
BLOB_IN = ("obs", "bg", "use_bg", "ren", "depth_ren", "depth_a", "depth_b", "label", "mask_idx")
ALL_OUT = tuple(BLOB_OUT_SHAPES)
# name -> (inputs left out (NULL), outputs passed).  An image output whose input is NULL is skipped: it must keep its sentinel.
PAIR_CASES = {
    "all": ((), ALL_OUT),
    "use_bg_null": (("use_bg",), ALL_OUT),                      # pastes every sample
    "no_background": (("bg",), ALL_OUT),
    "no_observed": (("obs",), ALL_OUT),
    "no_rendered_image": (("ren",), ALL_OUT),
    "mask_idx_null": (("mask_idx",), ALL_OUT),                  # the object's label value defaults to 1
    "depth_only": (("obs", "bg", "use_bg", "ren", "depth_b", "label", "mask_idx"),
                   ("image_observed", "image_rendered", "mask_rendered", "depth_rendered", "depth_a_out", "bbox_ren")),
    "label_only": (("obs", "bg", "use_bg", "ren", "depth_ren", "depth_a", "depth_b"), ("image_observed", "mask_label", "bbox_label")),
    "few_outputs": ((), ("image_rendered", "mask_rendered", "bbox_label", "depth_b_out")),
}
_DT = {"obs": np.uint8, "bg": np.uint8, "ren": np.uint8, "label": np.uint8, "use_bg": np.int32, "mask_idx": np.int32, "depth_ren": np.uint16,
       "depth_a": np.uint16, "depth_b": np.uint16}


def _blob_outs(names, H, W):
    return {k: Out((R.BLOB_B, 4), torch.int32) if BLOB_OUT_SHAPES[k] == 0 else Out((R.BLOB_B, BLOB_OUT_SHAPES[k], H, W)) for k in names}


def _check_blobs(outs, ref, tag):
    for k, o in outs.items():
        if k in ref:
            same(o.get(k), ref[k], "{} {}".format(tag, k))
        else:
            o.untouched("{} {}".format(tag, k))


@pytest.mark.parametrize("case", list(PAIR_CASES))
@pytest.mark.parametrize("H,W", R.BLOB_SHAPES)
def test_pair_blobs_from_raw(ops, H, W, case):
    """dim_pair_blobs_from_raw"""
    absent, out_names = PAIR_CASES[case]
    inp = R.blob_inputs(H, W)
    if case == "mask_idx_null":
        inp["label"] = np.where(inp["label"] == 7, 1, inp["label"]).astype(np.uint8)
    inp = {k: v for k, v in inp.items() if k not in absent}
    ref = R.blobs(inp)
    outs = _blob_outs(out_names, H, W)
    ops.pair_blobs_from_raw(R.BLOB_B, H, W, R.DEPTH_FACTOR, R.PIXEL_MEANS_BGR, mask_thr=R.MASK_THR,
                            **{k + "_bgr" if k in ("obs", "bg", "ren") else k: dev(inp.get(k), _DT[k]) for k in BLOB_IN if k in inp},
                            **{k: o.t for k, o in outs.items()})
    _check_blobs(outs, ref, "pair_blobs {}x{} {}".format(H, W, case))


@pytest.mark.parametrize("case", ["all", "no_observed", "no_rendered_image", "images_only", "mask_only", "bbox_only"])
@pytest.mark.parametrize("H,W", R.BLOB_SHAPES)
def test_test_blobs_from_raw(ops, H, W, case):
    """dim_test_blobs_from_raw"""
    inp = R.blob_inputs(H, W)
    ref = R.blobs({k: inp[k] for k in ("obs", "ren", "depth_ren") if not (case == "no_observed" and k == "obs") and
                   not (case == "no_rendered_image" and k == "ren")})
    ref["bbox"] = ref.pop("bbox_ren")
    names = {"images_only": ("image_observed", "image_rendered"), "mask_only": ("mask_rendered",), "bbox_only": ("bbox",)}.get(
        case, ("image_observed", "image_rendered", "mask_rendered", "bbox"))
    outs = {k: Out((R.BLOB_B, 4), torch.int32) if k == "bbox" else Out((R.BLOB_B, 3 if k.startswith("image") else 1, H, W)) for k in names}
    t = lambda k: outs[k].t if k in outs else None
    ops.test_blobs_from_raw(None if case == "no_observed" else dev(inp["obs"]), None if case == "no_rendered_image" else dev(inp["ren"]),
                            dev(inp["depth_ren"]), R.DEPTH_FACTOR, R.PIXEL_MEANS_BGR, t("image_observed"), t("image_rendered"),
                            t("mask_rendered"), t("bbox"), mask_thr=R.MASK_THR)
    _check_blobs(outs, ref, "test_blobs {}x{} {}".format(H, W, case))


def test_blobs_reject_bad_arguments(ops):
    from lib.hip.capi import DeepIMHipError

    H, W = R.BLOB_SHAPES[0]
    inp = R.blob_inputs(H, W)
    B = R.BLOB_B
    plane, box = Out((B, 1, H, W)), Out((B, 4), torch.int32)
    img = Out((B, 3, H, W))
    pair = lambda **kw: ops.pair_blobs_from_raw(B, kw.pop("H", H), kw.pop("W", W), R.DEPTH_FACTOR, R.PIXEL_MEANS_BGR, **kw)
    with pytest.raises(DeepIMHipError, match="multiple of 4"):
        pair(W=W + 2, ren_bgr=dev(np.zeros((B, H, W + 2, 3), np.uint8)), image_rendered=Out((B, 3, H, W + 2)).t)
    with pytest.raises(DeepIMHipError, match="multiple of 4"):
        ops.test_blobs_from_raw(None, None, dev(np.zeros((B, H, W + 2), np.uint16)), R.DEPTH_FACTOR, R.PIXEL_MEANS_BGR, None, None,
                                Out((B, 1, H, W + 2)).t, None)
    for kw in (dict(mask_rendered=plane.t), dict(depth_rendered=plane.t), dict(bbox_ren=box.t), dict(depth_a_out=plane.t),
               dict(depth_b_out=plane.t, depth_a=dev(inp["depth_a"])), dict(mask_label=plane.t), dict(label_raw=plane.t),
               dict(bbox_label=box.t), dict(obs_bgr=dev(inp["obs"]), bg_bgr=dev(inp["bg"]), image_observed=img.t)):
        with pytest.raises(DeepIMHipError):
            pair(**kw)
    # nothing was launched
    plane.untouched("rejected plane"), box.untouched("rejected box"), img.untouched("rejected image")


# ------------------------------------------------------------------------------------------------ mask dilation
@pytest.mark.parametrize("H,W", R.DILATE_SHAPES)
def test_mask_dilate(ops, H, W):
    """dim_mask_dilate"""
    masks, box = R.dilate_inputs(H, W)
    m = dev(masks)
    for name, thick in R.dilate_thickness_cases(H, W, box).items():
        out = Out(masks.shape)
        ops.mask_dilate(m, dev(thick), out=out.t)
        same(out.get(name), R.mask_dilate(masks, thick), "mask_dilate {}x{} {}".format(H, W, name))
    same(host(m), masks, "mask_dilate input")


def test_mask_dilate_rejects_in_place(ops):
    from lib.hip.capi import DeepIMHipError

    masks, _ = R.dilate_inputs(*R.DILATE_SHAPES[0])
    m = dev(masks)
    with pytest.raises(DeepIMHipError, match="in place"):
        ops.mask_dilate(m, dev(np.ones((R.DILATE_B, 4), np.int32)), out=m)
    same(host(m), masks, "mask_dilate in place: nothing launched")


# ------------------------------------------------------------------------------------------------ flow labels
def _flow_case(ops, s, thresh, tag, everywhere=False):
    B, _, H, W = s["depth_src"].shape
    ds, dt, P = dev(s["depth_src"]), dev(s["depth_tgt"]), dev(s["P12"], np.float64)
    for rep, wt in itertools.product((False, True), R.FLOW_WEIGHT_TYPES):
        ref = R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], thresh=thresh, standard_rep=rep, weight_type=wt)
        keep = np.ones_like(ref["tie"]) if everywhere else ~ref["tie"]
        n_valid = int(ref["valid"].sum())
        assert everywhere or (~keep).sum() <= 0.01 * n_valid
        flow, w = Out((B, 2, H, W)), Out((B, 2, H, W))
        ops.calc_flow_labels(ds, dt, P, s["Kinv"], flow.t, w.t, thresh=thresh, standard_rep=rep, weight_type=wt)
        what = "{} standard_rep={} weights={}".format(tag, rep, wt)
        got_f, got_w = flow.get(what), w.get(what)
        k2 = np.broadcast_to(keep, got_w.shape)
        same(got_w[k2], ref["weights"][k2], what + " weights")
        want = ref["flow"].astype(f32)
        bar = R.ulp32(ref["flow"]) + 1e-10
        err = np.abs(got_f.astype(np.float64) - want.astype(np.float64))
        print("{} flow: worst {:.3g} ulp over {} compared pixels ({} near ties left out)".format(
            what, float((err / R.ulp32(ref["flow"]))[k2].max()), int(keep.sum()), int((~keep).sum())))
        assert np.all(err[k2] <= bar[k2]), what
        unseen = np.broadcast_to((ref["visible"] == 0) & keep, got_f.shape)
        assert np.all(got_f[unseen] == 0), what
    # flow_weights NULL: the flow alone ("[h, w]" order, the default)
    ref = R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], thresh=thresh)
    keep = np.broadcast_to(np.ones_like(ref["tie"]) if everywhere else ~ref["tie"], (B, 2, H, W))
    flow = Out((B, 2, H, W))
    ops.calc_flow_labels(ds, dt, P, s["Kinv"], flow.t, None, thresh=thresh)
    err = np.abs(flow.get(tag).astype(np.float64) - ref["flow"].astype(f32).astype(np.float64))
    assert np.all(err[keep] <= (R.ulp32(ref["flow"]) + 1e-10)[keep]), tag + " without weights"


@pytest.mark.parametrize("H,W", R.FLOW_SHAPES)
def test_calc_flow_labels(ops, H, W):
    """dim_calc_flow_labels on the tilted-plane scene: visibility and weights equal outside the reference's near-tie set (at most 1 % of
    the valid sources, asserted on the reference alone by the host test), flow within one float32 ulp of float32(reference) + 1e-10"""
    _flow_case(ops, R.flow_scene(H, W), R.FLOW_THRESH, "calc_flow_labels {}x{}".format(H, W))


def test_calc_flow_labels_half_to_even(ops):
    """dim_calc_flow_labels on exact half-integer projections, an exact threshold tie and pz ~ 0 over a hole: compared everywhere"""
    s = R.flow_half_scene()
    _flow_case(ops, s, s["thresh"], "calc_flow_labels half-integer scene", everywhere=True)


# ------------------------------------------------------------------------------------------------ point clouds
@pytest.mark.parametrize("n", R.POINT_SIZES)
def test_point_clouds(ops, n):
    """dim_point_clouds"""
    inp = R.point_inputs(n)
    model, weights, observed = R.point_clouds(inp["table"], inp["table_off"], inp["idx"], inp["pose"])
    outs = [Out((R.POINT_B, 3, n)) for _ in range(3)]
    ops.point_clouds(dev(inp["table"]), dev(inp["table_off"]), dev(inp["idx"]), dev(inp["pose"]), outs[0].t, outs[1].t, outs[2].t)
    same(outs[0].get("model"), model, "point_clouds n={} model".format(n))
    same(outs[1].get("weights"), weights, "point_clouds n={} weights".format(n))
    got = outs[2].get("observed").astype(np.float64)
    err = np.abs(got - observed) / R.ulp32(observed)
    print("point_clouds n={} observed: worst {:.3g} ulp".format(n, float(err.max())))
    assert np.all(err <= 1.0)


# ------------------------------------------------------------------------------------------------ bbox, zoom window
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W", R.BBOX_SHAPES)
def test_mask_bbox_and_zoom_factor(ops, H, W, mode):
    """dim_mask_bbox, dim_zoom_factor"""
    xo, xr, thr, means = R.bbox_pairs(H, W, mode)
    B = len(xo)
    want_o, want_r = R.mask_bbox(xo, thr, mode, means), R.mask_bbox(xr, thr, mode, means)
    bo, br = Out((B, 4), torch.int32), Out((B, 4), torch.int32)
    ops.mask_bbox(dev(xo), thr, mode=mode, means3=means, out=bo.t)
    ops.mask_bbox(dev(xr), thr, mode=mode, means3=means, out=br.t)
    same(bo.get("bbox"), want_o, "mask_bbox {}x{} mode {} observed".format(H, W, mode))
    same(br.get("bbox"), want_r, "mask_bbox {}x{} mode {} rendered".format(H, W, mode))
    pose, K = R.zoom_factor_pose(B, H, W)
    want_zf, want_status = R.zoom_factor(want_o, want_r, pose, K, H, W)
    zf, status = Out((B, 4)), Out((B,), torch.int32)
    ops.zoom_factor(bo.t, br.t, dev(pose), K, H, W, out=zf.t, status=status.t)
    same(status.get("status"), want_status, "zoom_factor status")
    got = zf.get("zoom_factor")
    print("zoom_factor {}x{} mode {}: worst {:.3g}".format(H, W, mode, float(np.abs(got - want_zf).max())))
    np.testing.assert_allclose(got, want_zf, rtol=2e-6, atol=2e-6)      # the compiler may contract the float32 K t
    zf2 = Out((B, 4))
    ops.zoom_factor(bo.t, br.t, dev(pose), K, H, W, out=zf2.t)            # status NULL
    same(zf2.get("zoom_factor"), got, "zoom_factor without status")


def test_mask_bbox_rejects_bad_width(ops):
    from lib.hip.capi import DeepIMHipError

    with pytest.raises(DeepIMHipError, match="multiple of 4"):
        ops.mask_bbox(torch.zeros((1, 1, 8, 38), device=DEV), 0.3)


# ------------------------------------------------------------------------------------------------ zoom sampling
def rounded_same(got, want, before, what):
    """a rounded output: got may differ from the reference only where the reference's value before rounding lies within one float32 ulp
    of a rounding boundary -- and with bit-equal samples in front of it, nowhere"""
    diff = got != want
    near = R.round_boundary_distance_ulps(before) <= 1.0
    print("{}: {} of {} differ ({} away from a boundary); {} reference values within 1 ulp of a boundary".format(
        what, int(diff.sum()), diff.size, int((diff & ~near).sum()), int(near.sum())))
    assert not (diff & ~near).any(), what
    assert not diff.any(), what


def test_zoom_planes(ops):
    """dim_zoom_planes: every pre / post / scale_mode / inverse / add3 combination.  The un-rounded outputs are bit-equal to the float32
    restatement (one rounding per operation, in oracle/zoom.py's order) with the factor supplied by the test."""
    H, W = R.ZOOM_PLANES_SHAPE
    inp = R.zoom_inputs(H, W)
    zf = R.ZOOM_FACTORS
    x3 = inp["io"]
    x4 = np.concatenate([inp["depth_like"], inp["binary"], inp["flow"]], axis=1)
    zft = dev(zf)
    n = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for add3, inverse, pre in itertools.product((None, R.ZOOM_MEANS), (False, True), (0, 1)):
            x = x3 if add3 is not None else x4            # C = 4 also takes the `C > 3: no constants` path
            sampled = R.zoom_sample(x, zf, add3, pre, inverse)
            assert np.all(np.isfinite(sampled))
            xt = dev(x)
            for post, scale_mode in itertools.product((0, 1, 2), (0, 1, 2)):
                want, before = R.zoom_post(sampled, zf, post, scale_mode)
                out = Out(x.shape)
                ops.zoom_planes(xt, zft, inverse=inverse, pre=pre, post=post, add3=add3, scale_mode=scale_mode, out=out.t)
                what = "zoom_planes add3={} inverse={} pre={} post={} scale={}".format(add3 is not None, inverse, pre, post, scale_mode)
                got = out.get(what)
                if post == 0:
                    same(got, want, what)
                else:
                    rounded_same(got, want, before, what)
                n += 1
    assert n == 72
    # C = 1 and 2 with constants: only the first C are read
    for C in (1, 2):
        x = np.ascontiguousarray(x3[:, :C])
        same(host(ops.zoom_planes(dev(x), zft, add3=R.ZOOM_MEANS)), R.zoom_sample(x, zf, R.ZOOM_MEANS[:C]), "zoom_planes C={}".format(C))


@pytest.mark.parametrize("H,W", R.NET_INPUT_SHAPES)
def test_zoom_net_input(ops, H, W):
    """dim_zoom_net_input (with and without its four NCHW outputs) and dim_zoom_net_input_ex modes 0-3, every lane of X included"""
    inp = R.zoom_inputs(H, W)
    zf, means = R.ZOOM_FACTORS, R.ZOOM_MEANS
    B = R.ZOOM_B
    io, ir, zft = dev(inp["io"]), dev(inp["ir"]), dev(zf)
    tag = "zoom_net_input {}x{}".format(H, W)
    with np.errstate(over="ignore", invalid="ignore"):
        # the masks: once depth-like on both sides (rounding boundaries, the 0.2 threshold), once binary / depth-like
        for name, eo, er in (("depth-like", inp["depth_like"], inp["depth_like"]), ("binary", inp["binary"], inp["depth_like"])):
            ref = R.net_input(inp["io"], inp["ir"], eo, er, zf, means, 0)
            eot, ert = dev(eo), dev(er)
            X = Out((B, H, W, 8))
            nchw = [Out((B, 3, H, W)), Out((B, 3, H, W)), Out((B, 1, H, W)), Out((B, 1, H, W))]
            ops.zoom_net_input(io, ir, eot, ert, zft, means, X=X.t, nchw_out=tuple(o.t for o in nchw))
            got = X.get(tag)
            same(got[..., :6], ref["X"][..., :6], "{} {} X[0:6]".format(tag, name))
            for lane, k in ((6, 0), (7, 1)):
                rounded_same(got[..., lane], ref["X"][..., lane], ref["pre_round"][k][:, 0], "{} {} X[{}]".format(tag, name, lane))
            same(nchw[0].get(tag), ref["nchw"][0], "{} {} z_image_observed".format(tag, name))
            same(nchw[1].get(tag), ref["nchw"][1], "{} {} z_image_rendered".format(tag, name))
            rounded_same(nchw[2].get(tag), ref["nchw"][2], ref["pre_round"][0], "{} {} z_mask_observed".format(tag, name))
            rounded_same(nchw[3].get(tag), ref["nchw"][3], ref["pre_round"][1], "{} {} z_mask_rendered".format(tag, name))
            bits = lambda a: np.ascontiguousarray(a).view(np.int32)
            X2 = Out((B, H, W, 8))
            ops.zoom_net_input(io, ir, eot, ert, zft, means, X=X2.t)                      # no NCHW outputs
            np.testing.assert_array_equal(bits(X2.get(tag)), bits(got))
            X0 = Out((B, H, W, 8))
            ops.zoom_net_input_ex(io, ir, eot, ert, zft, means, 0, X=X0.t)                 # mode 0 = dim_zoom_net_input, bit for bit
            np.testing.assert_array_equal(bits(X0.get(tag)), bits(got))
            # mode 2: plain samples / 255 in lanes 6, 7; mode 3: the rounded masks in lanes 0, 1, zeros in 2-7
            r2 = R.net_input(inp["io"], inp["ir"], eo, er, zf, means, 2)["X"]
            X2 = Out((B, H, W, 8))
            ops.zoom_net_input_ex(io, ir, eot, ert, zft, means, 2, X=X2.t)
            same(X2.get(tag), r2, "{} {} mode 2".format(tag, name))
            r3 = R.net_input(inp["io"], inp["ir"], eo, er, zf, means, 3)
            X3 = Out((B, H, W, 8))
            ops.zoom_net_input_ex(io, ir, eot, ert, zft, means, 3, X=X3.t)
            g3 = X3.get(tag)
            rounded_same(g3[..., 0], r3["X"][..., 0], r3["pre_round"][0][:, 0], "{} {} mode 3 lane 0".format(tag, name))
            rounded_same(g3[..., 1], r3["X"][..., 1], r3["pre_round"][1][:, 0], "{} {} mode 3 lane 1".format(tag, name))
            same(g3[..., 2:], np.zeros_like(g3[..., 2:]), "{} {} mode 3 lanes 2-7".format(tag, name))
        # mode 1: images only, with and without the two extra planes; lanes 6, 7 are zero, not left as they were
        r1 = R.net_input(inp["io"], inp["ir"], None, None, zf, means, 1)["X"]
        for extra in ((None, None), (dev(inp["binary"]), dev(inp["depth_like"]))):
            X1 = Out((B, H, W, 8))
            ops.zoom_net_input_ex(io, ir, extra[0], extra[1], zft, means, 1, X=X1.t)
            same(X1.get(tag), r1, "{} mode 1".format(tag))


def test_zoom_net_input_rejects_bad_arguments(ops):
    from lib.hip.capi import DeepIMHipError

    H, W = R.NET_INPUT_SHAPES[0]
    inp = R.zoom_inputs(H, W)
    io, ir, m, zft = dev(inp["io"]), dev(inp["ir"]), dev(inp["binary"]), dev(R.ZOOM_FACTORS)
    X = Out((R.ZOOM_B, H, W, 8))
    with pytest.raises(DeepIMHipError, match="all four"):
        ops.zoom_net_input(io, ir, m, m, zft, R.ZOOM_MEANS, X=X.t, nchw_out=(torch.empty_like(io), None, None, None))
    for mode in (0, 2, 3):
        with pytest.raises(DeepIMHipError, match="extra planes"):
            ops.zoom_net_input_ex(io, ir, None, None, zft, R.ZOOM_MEANS, mode, X=X.t)
    with pytest.raises(DeepIMHipError, match="mode"):
        ops.zoom_net_input_ex(io, ir, m, m, zft, R.ZOOM_MEANS, 4, X=X.t)
    X.untouched("rejected zoom_net_input")
