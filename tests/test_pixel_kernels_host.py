"""CPU: the restatements of tests/pixel_kernels_reference.py are pinned to the project's host code and goldens (calc_flow and
tests/golden/flow_golden.npz, mask_dilate under the draws of draw_dilate_thickness, oracle/data_layer.py, oracle/zoom.py), and on
every input set the GPU tests use each named mutant changes at least one output element -- inputs that could not tell a wrong kernel
from the right one would make tests/test_gpu_pixel_kernels.py pass for nothing."""
import os

import numpy as np
import pytest

import pixel_kernels_reference as R
from oracle import data_layer as odl, zoom as ozoom

f32 = np.float32


def differs(a, b):
    if isinstance(a, dict):
        return any(differs(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return any(differs(x, y) for x, y in zip(a, b) if x is not None)
    return not np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------------ raw pixels -> blobs
@pytest.mark.parametrize("H,W", R.BLOB_SHAPES)
def test_blobs_reference_vs_oracle(H, W):
    inp = R.blob_inputs(H, W)
    ref = R.blobs(inp)
    means = R.PIXEL_MEANS_BGR.astype(np.float64)       # the float32 means the kernel gets, exactly; uint8 - mean is exact in float64
    assert set(np.unique(inp["depth_ren"])) >= set(R.DEPTH_SPECIALS)
    for b in range(R.BLOB_B):
        pasted = odl.paste_background(inp["obs"][b], inp["bg"][b], inp["label"][b]) if inp["use_bg"][b] else inp["obs"][b]
        np.testing.assert_array_equal(ref["image_observed"][b], odl.image_blob(pasted, means)[0].astype(f32))
        np.testing.assert_array_equal(ref["image_rendered"][b], odl.image_blob(inp["ren"][b], means)[0].astype(f32))
        np.testing.assert_array_equal(ref["mask_rendered"][b], odl.mask_rendered_blob(inp["depth_ren"][b], R.DEPTH_FACTOR)[0])
        np.testing.assert_array_equal(ref["depth_rendered"][b, 0], odl.depth_metres(inp["depth_ren"][b], R.DEPTH_FACTOR))
        np.testing.assert_array_equal(ref["depth_a_out"][b, 0], odl.depth_metres(inp["depth_a"][b], R.DEPTH_FACTOR))
        np.testing.assert_array_equal(ref["depth_b_out"][b, 0], odl.depth_metres(inp["depth_b"][b], R.DEPTH_FACTOR))
        m_obs, _ = odl.masks_test(np.ones((H, W), np.uint16), R.DEPTH_FACTOR, "mask_gt_observed", False, inp["label"][b], inp["mask_idx"][b])
        np.testing.assert_array_equal(ref["mask_label"][b], m_obs[0])
        for box, mask in ((ref["bbox_ren"][b], ref["depth_rendered"][b, 0] > f32(0.2)), (ref["bbox_label"][b], ref["mask_label"][b, 0] != 0)):
            if mask.any():
                x0, y0, x1, y1 = odl.min_rect(mask)
                assert box.tolist() == [x0, x1, y0, y1]
            else:
                assert box.tolist() == [W, -1, H, -1]
    # the cases the inputs promise
    assert ref["bbox_ren"][0].tolist() == [0, W - 1, 0, H - 1] and ref["bbox_label"][0].tolist() == [0, W - 1, 0, H - 1]
    assert ref["bbox_ren"][1].tolist() == [W - 1, W - 1, H - 1, H - 1] and ref["bbox_label"][1].tolist() == [W - 1, W - 1, H - 1, H - 1]
    assert ref["bbox_ren"][2].tolist() == [W, -1, H, -1] and ref["bbox_label"][2].tolist() == [W, -1, H, -1]
    d200 = inp["depth_ren"] == 200
    assert d200.any() and np.all(ref["mask_rendered"][:, 0][d200] == f32(200) / f32(1000))      # AT the threshold: stays depth
    assert np.all(ref["mask_rendered"][:, 0][inp["depth_ren"] == 201] == 1)
    # use_bg NULL pastes every sample; without a background nothing is pasted
    all_bg = R.blobs(dict(inp, use_bg=None))["image_observed"]
    assert differs(all_bg[1], ref["image_observed"][1]) and not differs(all_bg[0], ref["image_observed"][0])
    np.testing.assert_array_equal(R.blobs(dict(inp, bg=None))["image_observed"][1], ref["image_observed"][1])
    # mask_idx NULL means label value 1
    one = R.blobs(dict(inp, label=(inp["label"] == 7).astype(np.uint8), mask_idx=None))
    np.testing.assert_array_equal(one["mask_label"][:, 0], (inp["label"] == 7).astype(f32))


@pytest.mark.parametrize("mutant", R.MUTANTS["blobs"])
@pytest.mark.parametrize("H,W", R.BLOB_SHAPES)
def test_blobs_inputs_separate_mutants(H, W, mutant):
    inp = R.blob_inputs(H, W)
    assert differs(R.blobs(inp), R.blobs(inp, mutant=mutant))


# ------------------------------------------------------------------------------------------------ mask dilation
@pytest.mark.parametrize("H,W", R.DILATE_SHAPES)
def test_dilate_reference_vs_host(H, W):
    from deepim.core.loader import draw_dilate_thickness
    from lib.utils.mask_dilate import mask_dilate

    masks, box = R.dilate_inputs(H, W)
    seen = set()
    for seed in range(24):
        np.random.seed(seed)
        thick = np.array([draw_dilate_thickness(10) for _ in range(R.DILATE_B)], np.int32)
        np.random.seed(seed)
        want = np.stack([mask_dilate(masks[b, 0], 10) for b in range(R.DILATE_B)])[:, None]
        np.random.seed(seed)
        np.testing.assert_array_equal(np.stack([odl.mask_dilate(masks[b, 0], 10) for b in range(R.DILATE_B)])[:, None], want)
        np.testing.assert_array_equal(R.mask_dilate(masks, thick), want)
        seen |= {tuple(t > 0) for t in thick}
    assert len(seen) >= 6                # the draws skip different sides
    # the explicit cases of the GPU test: thickness 0 is the clamp alone, a displacement past the border adds nothing on that side
    cases = R.dilate_thickness_cases(H, W, box)
    clamped = np.minimum(masks, 1)
    np.testing.assert_array_equal(R.mask_dilate(masks, cases["none"]), clamped)
    r0, r1, c0, c1 = box
    reach, beyond = R.mask_dilate(masks, cases["reach"]), R.mask_dilate(masks, cases["beyond"])
    assert reach[0, 0, H - 1, c0] == 1 and reach[0, 0, 0, c0] == 1 and reach[0, 0, r0, W - 1] == 1 and reach[0, 0, r0, 0] == 1
    # one step further and the copy of the block's last row / column has left the frame: that side marks one line less
    assert (beyond[0] != 0).sum() < (reach[0] != 0).sum() or W > 64
    tall = R.mask_dilate(masks, cases["tall"])
    np.testing.assert_array_equal(tall[:, :, :, : W - H][masks[:, :, :, : W - H] != 0], clamped[:, :, :, : W - H][masks[:, :, :, : W - H] != 0])
    assert masks.max() > 1 and np.any((masks > 0) & (masks < 0.2))


@pytest.mark.parametrize("mutant", R.MUTANTS["dilate"])
@pytest.mark.parametrize("H,W", R.DILATE_SHAPES)
def test_dilate_inputs_separate_mutants(H, W, mutant):
    masks, box = R.dilate_inputs(H, W)
    cases = R.dilate_thickness_cases(H, W, box)
    assert any(differs(R.mask_dilate(masks, t), R.mask_dilate(masks, t, mutant=mutant)) for t in cases.values())


# ------------------------------------------------------------------------------------------------ flow labels
def _calc_flow_batch(s, standard_rep):
    from lib.pair_matching.flow import calc_flow

    flows, vis = [], []
    for b in range(len(s["depth_src"])):
        f, v, _ = calc_flow(s["depth_src"][b, 0], s["pose_src"][b], s["pose_tgt"][b], s["K"], s["depth_tgt"][b, 0], thresh=R.FLOW_THRESH,
                            standard_rep=standard_rep)
        flows.append(f.transpose(2, 0, 1)), vis.append(v[None])
    return np.stack(flows), np.stack(vis)


@pytest.mark.parametrize("H,W", R.FLOW_SHAPES)
def test_flow_reference_vs_calc_flow(H, W):
    s = R.flow_scene(H, W)
    for rep in (False, True):
        ref = R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], standard_rep=rep)
        flow, vis = _calc_flow_batch(s, rep)
        np.testing.assert_array_equal(ref["visible"], vis)
        err = np.abs(ref["flow"] - flow).max()
        print("flow restatement vs calc_flow {}x{} standard_rep={}: {:.2g}".format(H, W, rep, err))
        assert err < 1e-12
    valid, inside, seen = ref["valid"], ref["inside"], ref["visible"] != 0
    n_valid = int(valid.sum())
    print("valid {} inside {} outside {} visible {} near-tie {}".format(n_valid, int(inside.sum()), n_valid - int(inside.sum()), int(seen.sum()),
                                                                       int(ref["tie"].sum())))
    # the near-tie set (where a last-bit difference of the device's float64 may legitimately flip the predicate): at most 1 % of the sources
    assert ref["tie"].sum() <= 0.01 * n_valid
    # the scene reaches every branch: holes in the source, projections inside and outside, seen and occluded, holes in the target
    assert 0.1 * valid.size < (~valid).sum() < 0.3 * valid.size
    assert inside.sum() > 0.2 * n_valid and (valid & ~inside).sum() > 0.2 * n_valid
    assert seen.sum() > 100 and (inside & ~seen).sum() > 100
    # ... and leaves the frame on every side
    sides = _outside_sides(s)
    assert all(n > 0 for n in sides), sides
    # weights by type, against the data layer's restatement of get_pair_flow
    for wt in R.FLOW_WEIGHT_TYPES:
        w = R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], weight_type=wt)["weights"]
        d0 = s["depth_src"][:, 0] == 0
        want = {"all": np.ones_like(d0), "viz": seen[:, 0], "valid": d0 | seen[:, 0]}[wt]
        np.testing.assert_array_equal(w[:, 0], want.astype(f32))
        np.testing.assert_array_equal(w[:, 1], w[:, 0])
    assert differs(R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], weight_type="valid")["weights"], ref["weights"])


def _outside_sides(s):
    """how many valid source pixels project past the left, right, top and bottom border"""
    B, _, H, W = s["depth_src"].shape
    v, u = np.mgrid[0:H, 0:W]
    n = [0, 0, 0, 0]
    for b in range(B):
        d = s["depth_src"][b, 0].astype(np.float64)
        X = np.einsum("ij,jhw->ihw", s["Kinv"], np.stack([u, v, np.ones_like(u)]).astype(np.float64)) * d
        xp = np.einsum("ij,jhw->ihw", s["P12"][b][:, :3], X) + s["P12"][b][:, 3].reshape(3, 1, 1)
        cw, ch = np.round(xp[0] / (xp[2] + 1e-15)), np.round(xp[1] / (xp[2] + 1e-15))
        ok = d != 0
        for i, m in enumerate((cw < 0, cw >= W, ch < 0, ch >= H)):
            n[i] += int((m & ok).sum())
    return n


def test_flow_reference_vs_golden(golden_dir):
    """the reference's own calc_flow outputs (stored as float32)"""
    g = np.load(os.path.join(golden_dir, "flow_golden.npz"))
    K = g["K"]
    n = 3
    P = R.flow_P12(K, g["pose_src"][:n], g["pose_tgt"][:n])
    ref = R.flow_labels(g["depth_src"][:n, None], g["depth_tgt"][:n, None], P, np.linalg.inv(K.astype(np.float64)))
    np.testing.assert_array_equal(ref["visible"][:, 0], g["visible"][:n])
    np.testing.assert_allclose(ref["flow"].transpose(0, 2, 3, 1), g["flow"][:n], atol=1e-6)     # "[h, w]" order
    assert ref["visible"].sum() > 1500


def _half(s, **kw):
    return R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], thresh=s["thresh"], **kw)


def test_flow_half_integer_scene_is_half_to_even():
    s = R.flow_half_scene()
    ref, away = _half(s), _half(s, mutant="round_half_away")
    H, W = s["depth_src"].shape[2:]
    assert ref["tie"][:2].all()                                # every projection IS a half-integer
    # +0.5: u + 0.5 -> the even neighbour, inside unless it is W (u = W - 1 odd -> W): all but the last column / row are seen, and
    # source (0, 0), whose target pixel (0, 0) sits exactly at the threshold
    want0 = np.zeros((H, W))
    want0[: H - 1, : W - 1] = 1
    want0[0, 0] = 0
    np.testing.assert_array_equal(ref["visible"][0, 0], want0)
    want1 = np.ones((H, W))                                    # -0.5 at u = 0 rounds to -0: pixel 0
    want1[:2, :2] = 0                                          # ... where the target is at the threshold
    np.testing.assert_array_equal(ref["visible"][1, 0], want1)
    np.testing.assert_array_equal(np.abs(ref["flow"][0][:, want0 == 1]), 0.5)
    np.testing.assert_array_equal(ref["visible"][2], 0)
    for b in (0, 1):                                           # half away from zero lands on holes or outside for every even u or v
        assert (away["visible"][b] != ref["visible"][b]).sum() >= H * W // 2
    assert _half(s, mutant="thresh_le")["visible"][0, 0, 0, 0] == 1
    assert _half(s, mutant="no_hole_test")["visible"][2].all()
    # numpy's own rounding (what calc_flow uses) agrees
    assert np.round(0.5) == 0 and np.round(1.5) == 2 and np.round(-0.5) == 0


@pytest.mark.parametrize("mutant", R.MUTANTS["flow"])
def test_flow_inputs_separate_mutants(mutant):
    def run(s, **kw):
        return [R.flow_labels(s["depth_src"], s["depth_tgt"], s["P12"], s["Kinv"], thresh=s.get("thresh", R.FLOW_THRESH), standard_rep=rep, weight_type=wt, **kw)
                for rep in (False, True) for wt in R.FLOW_WEIGHT_TYPES]
    keys = ("flow", "visible", "weights")
    for s in [R.flow_scene(*hw) for hw in R.FLOW_SHAPES[:1]] + [R.flow_half_scene()]:
        if mutant == "channels_swapped":      # must show for EITHER standard_rep on its own
            a, b = run(s), run(s, mutant=mutant)
            if all(differs(x["flow"], y["flow"]) for x, y in zip(a, b)):
                return
        elif any(differs({k: x[k] for k in keys}, {k: y[k] for k in keys}) for x, y in zip(run(s), run(s, mutant=mutant))):
            return
    raise AssertionError("the flow inputs do not separate " + mutant)


# ------------------------------------------------------------------------------------------------ point clouds
@pytest.mark.parametrize("n", R.POINT_SIZES)
def test_point_reference_vs_oracle(n):
    inp = R.point_inputs(n)
    model, weights, observed = R.point_clouds(inp["table"], inp["table_off"], inp["idx"], inp["pose"])
    assert (inp["idx"][1] < 0).all() and len(set(inp["table_off"].tolist())) == 3
    if n > 40:
        assert (inp["idx"][0, 40:] < 0).all() and (inp["idx"][0, :40] >= 0).all()
    sizes = {300: 40, 0: 300, 340: 270}
    for b in range(R.POINT_B):
        # oracle.data_layer.point_clouds shuffles with numpy's global RNG: feed it the class's points already in the drawn order
        keep = inp["idx"][b][inp["idx"][b] >= 0]
        pts = inp["table"][inp["table_off"][b]:inp["table_off"][b] + sizes[int(inp["table_off"][b])]][keep]
        state = np.random.get_state()
        try:
            real_shuffle = np.random.shuffle
            np.random.shuffle = lambda a: None
            m, w, o = odl.point_clouds(pts.astype(np.float64).reshape(-1, 3), n, inp["pose"][b].astype(np.float64))
        finally:
            np.random.shuffle = real_shuffle
            np.random.set_state(state)
        np.testing.assert_array_equal(model[b], m[0].astype(f32))
        np.testing.assert_array_equal(weights[b], w[0].astype(f32))
        np.testing.assert_allclose(observed[b], o[0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("mutant", R.MUTANTS["points"])
@pytest.mark.parametrize("n", R.POINT_SIZES)
def test_point_inputs_separate_mutants(n, mutant):
    inp = R.point_inputs(n)
    a = R.point_clouds(inp["table"], inp["table_off"], inp["idx"], inp["pose"])
    b = R.point_clouds(inp["table"], inp["table_off"], inp["idx"], inp["pose"], mutant=mutant)
    assert differs(a, b)


# ------------------------------------------------------------------------------------------------ bbox, zoom window
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W", R.BBOX_SHAPES)
def test_bbox_reference_vs_oracle(H, W, mode):
    x, thr, means = R.bbox_inputs(H, W, mode)
    box = R.mask_bbox(x, thr, mode, means)
    assert box[:4].tolist() == [[0, 0, 0, 0], [W - 1, W - 1, 0, 0], [0, 0, H - 1, H - 1], [W - 1, W - 1, H - 1, H - 1]]
    assert box[4].tolist() == [6, 6, H - 3, H - 3]          # everything AT the threshold is out, the one value above it is in
    assert box[5].tolist() == [W, -1, H, -1]
    valid = (x[:, 0] > f32(thr)) if mode == 0 else (np.sum(x + means.reshape(1, 3, 1, 1), axis=1) > f32(thr))   # zoom_mask.py / zoom_image.py
    for b in range(len(x)):
        nz_x, nz_y = ozoom._bbox(valid[b])
        if len(nz_x):
            assert box[b].tolist() == [nz_x.min(), nz_x.max(), nz_y.min(), nz_y.max()]
    if mode == 1:
        at = np.sum(x[4] + means.reshape(3, 1, 1), axis=0)
        assert (at == f32(thr)).sum() > 10                   # the sums really sit ON the threshold


@pytest.mark.parametrize("H,W", R.BBOX_SHAPES)
def test_zoom_factor_reference_cases(H, W):
    xo, xr, thr, means = R.bbox_pairs(H, W, 0)
    bo, br = R.mask_bbox(xo, thr, 0), R.mask_bbox(xr, thr, 0)
    pose, K = R.zoom_factor_pose(len(xo), H, W)
    zf, status = R.zoom_factor(bo, br, pose, K, H, W)
    assert status.tolist() == [0, 0, 0, 0, 0, 1, 2]
    assert zf[5].tolist() == [1, 1, 0, 0] and np.all(np.isfinite(zf)) and np.all(zf[:5, 0] > 0)
    # the boxes alone decide the window: the oracle on the full masks gives the same factors
    keep = [b for b in range(len(xo)) if not status[b] & 1]
    want, empty = ozoom.zoom_factor_from_valid(xo[keep, 0] > f32(thr), xr[keep, 0] > f32(thr), pose[keep], K, H, W)
    np.testing.assert_array_equal(zf[keep], want)
    assert empty.tolist() == [bool(status[b] & 2) for b in keep]


# ------------------------------------------------------------------------------------------------ zoom sampling
def _oracle_sample(x, zf, H, W):
    return ozoom.bilinear_sampler(x, ozoom._grid_from_factor(zf, H, W))


@pytest.mark.parametrize("H,W", (R.ZOOM_PLANES_SHAPE,) + R.NET_INPUT_SHAPES)
def test_zoom_reference_vs_oracle(H, W):
    inp = R.zoom_inputs(H, W)
    zf = R.ZOOM_FACTORS
    bgr_means = R.ZOOM_MEANS[::-1]
    np.testing.assert_array_equal(R.inverse_zoom_factor(zf, H, W), ozoom.inverse_zoom_factor(zf, H, W))
    eq = np.testing.assert_array_equal
    with np.errstate(over="ignore", invalid="ignore"):
        eq(R.zoom_sample(inp["depth_like"], zf), _oracle_sample(inp["depth_like"], zf, H, W))
        zio, zir = ozoom.zoom_image_with_factor(zf, inp["io"], inp["ir"], bgr_means, H, W)
        eq(R.zoom_planes(inp["io"], zf, add3=R.ZOOM_MEANS)[0], zio)
        eq(R.zoom_planes(inp["ir"], zf, add3=R.ZOOM_MEANS)[0], zir)
        for inv in (False, True):
            eq(R.zoom_planes(inp["depth_like"], zf, inverse=inv, pre=1, post=1)[0], ozoom.zoom_mask_with_factor(zf, inp["depth_like"], inv, H, W))
        rf, rw = ozoom.zoom_flow(zf, inp["flow"], np.tile(inp["binary"], (1, 2, 1, 1)), False, H, W)
        eq(R.zoom_planes(inp["flow"], zf, scale_mode=1)[0], rf)
        eq(R.zoom_planes(np.tile(inp["binary"], (1, 2, 1, 1)), zf, post=2)[0], rw)
        eq(R.zoom_planes(inp["flow"], zf, inverse=True, scale_mode=2)[0], ozoom.zoom_flow(zf, inp["flow"], None, True, H, W))
        d0, d1 = ozoom.zoom_depth(zf, inp["depth_like"], inp["binary"], H, W)
        eq(R.zoom_planes(inp["depth_like"], zf)[0], d0)
        # the fused network input = the oracle's Concat of its zoomed pieces
        full = R.net_input(inp["io"], inp["ir"], inp["depth_like"], inp["depth_like"], zf, R.ZOOM_MEANS, 0)
        zmo = ozoom.mx_round(_oracle_sample(inp["depth_like"], zf, H, W))
        zmr = ozoom.zoom_mask_with_factor(zf, inp["depth_like"], False, H, W)
        want = np.concatenate([zio / f32(255), zir / f32(255), zmo, zmr], axis=1).transpose(0, 2, 3, 1)
        eq(full["X"], want)
        for got, w in zip(full["nchw"], (zio, zir, zmo, zmr)):
            eq(got, w)
        m1 = R.net_input(inp["io"], inp["ir"], None, None, zf, R.ZOOM_MEANS, 1)["X"]
        eq(m1[..., :6], want[..., :6]), eq(m1[..., 6:], 0)
        m2 = R.net_input(inp["io"], inp["ir"], inp["depth_like"], inp["binary"], zf, R.ZOOM_MEANS, 2)["X"]
        eq(m2[..., :6], want[..., :6]), eq(m2[..., 6], d0[:, 0] / f32(255)), eq(m2[..., 7], d1[:, 0] / f32(255))
        m3 = R.net_input(inp["io"], inp["ir"], inp["depth_like"], inp["depth_like"], zf, R.ZOOM_MEANS, 3)["X"]
        eq(m3[..., 0], zmo[:, 0]), eq(m3[..., 1], zmr[:, 0]), eq(m3[..., 2:], 0)
    # what the factors promise: the identity lands on (float32: very nearly on) the pixel centres, exactly so in part of the columns;
    # the far window and the 1e30 window sample nothing but padding
    ident = R.zoom_sample(inp["flow"], zf)
    np.testing.assert_allclose(ident[1], inp["flow"][1], atol=5e-3)
    assert (ident[1] == inp["flow"][1]).mean() > 0.2
    eq(ident[3], 0)
    assert (ident[4] != 0).sum() <= ident.shape[1]             # 1e30 x 0 = 0: only a pixel whose x_t and y_t are exactly 0 samples the centre
    shifted = R.zoom_sample(np.ones((R.ZOOM_B, 1, H, W), f32), zf)[2, 0]
    assert (shifted == 0).any() and (shifted == 1).any() and ((shifted > 0) & (shifted < 1)).any()     # padding, inside, the mixed border
    # rounding boundaries and the binarise threshold are really hit
    pre = R.zoom_sample(inp["depth_like"], zf)
    assert (R.round_boundary_distance_ulps(pre[1]) == 0).sum() > 10 and (inp["depth_like"] == f32(0.2)).sum() > 10


@pytest.mark.parametrize("mutant", R.MUTANTS["zoom"])
@pytest.mark.parametrize("H,W", (R.ZOOM_PLANES_SHAPE,) + R.NET_INPUT_SHAPES)
def test_zoom_inputs_separate_mutants(H, W, mutant):
    inp = R.zoom_inputs(H, W)
    zf = R.ZOOM_FACTORS
    runs = ((inp["io"], dict(add3=R.ZOOM_MEANS)), (inp["depth_like"], dict(pre=1, post=1)), (inp["depth_like"], dict(post=1)),
            (inp["flow"], dict(scale_mode=1)), (inp["flow"], dict(inverse=True, scale_mode=2)))
    with np.errstate(over="ignore", invalid="ignore"):
        assert any(differs(R.zoom_planes(x, zf, **kw)[0], R.zoom_planes(x, zf, mutant=mutant, **kw)[0]) for x, kw in runs)


@pytest.mark.parametrize("mutant", R.MUTANTS["net_input"])
@pytest.mark.parametrize("H,W", R.NET_INPUT_SHAPES)
def test_net_input_inputs_separate_mutants(H, W, mutant):
    inp = R.zoom_inputs(H, W)
    mode = int(mutant[4])
    args = (inp["io"], inp["ir"], inp["depth_like"], inp["binary"], R.ZOOM_FACTORS, R.ZOOM_MEANS, mode)
    with np.errstate(over="ignore", invalid="ignore"):
        assert differs(R.net_input(*args)["X"], R.net_input(*args, mutant=mutant)["X"])
