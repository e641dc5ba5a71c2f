"""Plain numpy restatements of the per-pixel kernels that build the network's inputs and labels (csrc/data.hip: raw pixels -> blobs,
mask dilation, first-iteration flow labels, point clouds; csrc/zoom.hip: bbox reduction, zoom window, affine bilinear gather and the
fused network input), their named mutants, and the seeded inputs tests/test_pixel_kernels_host.py and tests/test_gpu_pixel_kernels.py
share.

Where the project already pins an operation on the host (lib.pair_matching.flow.calc_flow, lib.utils.mask_dilate.mask_dilate,
oracle/zoom.py, oracle/data_layer.py) that code is the authority: the host test shows the restatement here equal to it, and the
restatement exists because the kernels take the random draws, the projection matrix and the zoom factor as INPUTS and write outputs
(bounding boxes, weights, NHWC lanes) that the host code never forms.

Arithmetic: the blob kernels do one float32 operation per output (a subtraction or a division), so numpy float32 gives the same bits;
flow labels and point clouds are float64 per pixel, rounded once; the zoom sampler is float32 with ONE rounding per operation in the
order oracle/zoom.py evaluates them.  `mutant=NAME` evaluates a plausible wrong kernel instead (MUTANTS lists them per operation).
"""
import numpy as np

f32 = np.float32

MUTANTS = {
    "blobs": ("channels_not_reversed", "means_not_reversed", "thr_ge", "depth_halves_swapped", "depth_signed", "paste_ignores_use_bg",
              "paste_where_not_object", "bbox_max_exclusive", "bbox_empty_zero"),
    "dilate": ("sides_permuted", "no_border_guard", "grow_nonzero", "no_clamp"),
    "flow": ("round_half_away", "clamp_outside", "thresh_le", "no_hole_test", "channels_swapped", "valid_without_d0"),
    "points": ("no_table_off", "negative_reads_0", "pose_transposed", "padded_weight_1"),
    "zoom": ("grid_W", "corner_clamped", "round_half_even", "bin_ge", "mean_kept", "scale_wy", "forward_for_inverse"),
    "net_input": ("mode1_lanes", "mode2_lanes", "mode3_lanes", "mode2_no_255"),
}


def _check(op, mutant):
    assert mutant is None or mutant in MUTANTS[op], (op, mutant)


# =================================================================================================================== raw pixels -> blobs
PIXEL_MEANS_BGR = np.array([102.9801, 115.9465, 122.7717], f32)   # config order (B, G, R)
DEPTH_FACTOR = 1000.0
MASK_THR = 0.2
BLOB_SHAPES = ((13, 36), (40, 52))      # 117 threads: one partial block with a half-dead and two dead waves; 520: two full blocks + one partial
BLOB_B = 3
BLOB_MASK_IDX = np.array([2, 5, 3], np.int32)
BLOB_USE_BG = np.array([1, 0, 1], np.int32)
DEPTH_SPECIALS = (0, 199, 200, 201, 32768, 65535)


def bbox_of(pred, mutant=None):
    """{min_x, max_x, min_y, max_y} of a boolean (H, W) image, {W, -1, H, -1} when empty"""
    H, W = pred.shape
    ys, xs = np.nonzero(pred)
    if len(xs) == 0:
        return np.array([0, 0, 0, 0] if mutant == "bbox_empty_zero" else [W, -1, H, -1], np.int32)
    e = 1 if mutant == "bbox_max_exclusive" else 0
    return np.array([xs.min(), xs.max() + e, ys.min(), ys.max() + e], np.int32)


def blob_inputs(H, W):
    """B = 3 raw pairs: sample 0 an object touching all four frame borders (a cross through the frame), sample 1 a one-pixel object in
    the last pixel, sample 2 empty (no depth above the threshold, no pixel of its mask_idx).  Depths hold 0, 199, 200, 201 (the
    threshold is `>` at factor 1000), 32768 and 65535 (the top bit of a 16-bit half); labels hold 0, the object's value and a third."""
    rng = np.random.default_rng(1000 * H + W)
    B = BLOB_B
    obs = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    ren = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    bg = ((obs.astype(np.int64) + rng.integers(1, 255, size=obs.shape)) % 256).astype(np.uint8)      # differs from obs everywhere
    low = np.array([0, 199, 200, 7, 150, 200, 0, 63], np.uint16)
    high = np.array([201, 32768, 65535, 900, 40000, 32767, 201, 65534], np.uint16)
    pick = lambda tab: tab[rng.integers(0, len(tab), size=(H, W))]
    cross = np.zeros((H, W), bool)
    cross[H // 2, :] = True
    cross[:, W // 3] = True
    cross[2:5, 3:9] = True
    depth = np.zeros((B, H, W), np.uint16)
    depth[0] = np.where(cross, pick(high), pick(low))
    depth[1] = pick(low)
    depth[1, H - 1, W - 1] = 201
    depth[2] = pick(low)
    depth_a = rng.integers(0, 65536, size=(B, H, W)).astype(np.uint16)
    depth_b = rng.integers(0, 65536, size=(B, H, W)).astype(np.uint16)
    depth_a[:, 1, :6] = DEPTH_SPECIALS
    depth_b[:, H - 1, W - 6:] = DEPTH_SPECIALS
    label = np.zeros((B, H, W), np.uint8)
    label[0] = np.where(cross, 2, np.where(rng.random((H, W)) < 0.3, 7, 0))
    label[1] = np.where(rng.random((H, W)) < 0.4, 2, 0)
    label[1, H - 1, W - 1] = 5
    label[2] = np.where(rng.random((H, W)) < 0.5, rng.choice(np.array([2, 7], np.uint8), size=(H, W)), 0)
    return {"obs": obs, "bg": bg, "use_bg": BLOB_USE_BG.copy(), "ren": ren, "depth_ren": depth, "depth_a": depth_a, "depth_b": depth_b,
            "label": label, "mask_idx": BLOB_MASK_IDX.copy()}


def _image_planes(bgr_u8, means_bgr, mutant):
    """(B,H,W,3) uint8 BGR -> (B,3,H,W): plane c = float32(bgr[2 - c]) - means[2 - c], one float32 subtraction"""
    B, H, W, _ = bgr_u8.shape
    out = np.empty((B, 3, H, W), f32)
    for c in range(3):
        ch = c if mutant == "channels_not_reversed" else 2 - c
        mc = c if mutant == "means_not_reversed" else 2 - c
        out[:, c] = bgr_u8[..., ch].astype(f32) - f32(means_bgr[mc])
    return out


def _metres(depth_u16, depth_factor, mutant):
    d = np.asarray(depth_u16, np.uint16)
    if mutant == "depth_halves_swapped":      # the two 16-bit halves of every 32-bit word: pixels 2k and 2k + 1 exchanged
        d = d.reshape(-1, 2)[:, ::-1].reshape(d.shape)
    if mutant == "depth_signed":
        d = d.view(np.int16)
    return d.astype(f32) / f32(depth_factor)


def blobs(inp, depth_factor=DEPTH_FACTOR, means_bgr=PIXEL_MEANS_BGR, thr=MASK_THR, mutant=None):
    """the outputs of dim_pair_blobs_from_raw for the inputs present in `inp` (a missing / None input switches its outputs off):
    image_observed, image_rendered, mask_rendered, depth_rendered, depth_a_out, depth_b_out, mask_label, label_raw, bbox_ren, bbox_label"""
    _check("blobs", mutant)
    g = lambda k: inp.get(k)
    out = {}
    thr = f32(thr)
    label, idx = g("label"), g("mask_idx")
    if label is not None:
        B = label.shape[0]
        idx = np.ones(B, np.int32) if idx is None else idx
        on = label == idx.reshape(B, 1, 1).astype(np.int64)
        out["mask_label"] = on.astype(f32)[:, None]
        out["label_raw"] = label.astype(f32)[:, None]
        out["bbox_label"] = np.stack([bbox_of(on[b], mutant) for b in range(B)])
    if g("obs") is not None:
        im = g("obs")
        if g("bg") is not None:
            B = im.shape[0]
            use = np.ones(B, bool) if (g("use_bg") is None or mutant == "paste_ignores_use_bg") else g("use_bg") != 0
            where = (label != idx.reshape(B, 1, 1)) if mutant == "paste_where_not_object" else (label == 0)
            im = np.where((where & use.reshape(B, 1, 1))[..., None], g("bg"), im)
        out["image_observed"] = _image_planes(im, means_bgr, mutant)
    if g("ren") is not None:
        out["image_rendered"] = _image_planes(g("ren"), means_bgr, mutant)
    if g("depth_ren") is not None:
        d = _metres(g("depth_ren"), depth_factor, mutant)
        above = (d >= thr) if mutant == "thr_ge" else (d > thr)
        out["depth_rendered"] = d[:, None]
        out["mask_rendered"] = np.where(above, f32(1), d)[:, None]
        out["bbox_ren"] = np.stack([bbox_of(above[b], mutant) for b in range(d.shape[0])])
    for k in ("depth_a", "depth_b"):
        if g(k) is not None:
            out[k + "_out"] = _metres(g(k), depth_factor, mutant)[:, None]
    return out


# =================================================================================================================== mask dilation
DILATE_SHAPES = ((14, 37), (12, 260))
DILATE_B = 4


def dilate_inputs(H, W):
    """(masks (4,1,H,W), box): sample 0 a binary block `box` = (r0, r1, c0, c1) (inclusive) with a hole and a second block two columns
    away (a gap both sides can reach: the clamp at 1), sample 1 touching every border, sample 2 raw label values 2 and 5, sample 3 the
    block with fractional values below 0.2 around it (non-zero: they neither grow nor are grown into)"""
    m = np.zeros((DILATE_B, 1, H, W), f32)
    r0, r1, c0, c1 = 4, 8, 10, 20
    m[0, 0, r0:r1 + 1, c0:c1 + 1] = 1
    m[0, 0, 6, 14:17] = 0
    m[0, 0, r0:r1 + 1, c1 + 3:c1 + 5] = 1
    m[1, 0, 0, :] = 1
    m[1, 0, H - 1, 3:] = 1
    m[1, 0, :, 0] = 1
    m[1, 0, 2:, W - 1] = 1
    m[1, 0, H // 2, W // 2] = 1
    m[2, 0, r0:r1 + 1, c0:c1 + 1] = 2
    m[2, 0, 1:3, W - 3:W] = 5
    m[2, 0, H - 2:, 0:2] = 5
    m[3, 0, r0:r1 + 1, c0:c1 + 1] = 1
    m[3, 0, r0 - 2:r0, c0:c1 + 1] = 0.1
    m[3, 0, r0:r1 + 1, c1 + 1:c1 + 3] = 0.15
    m[3, 0, H - 1, W - 4:] = 1
    return m, (r0, r1, c0, c1)


def dilate_thickness_cases(H, W, box):
    """name -> (4,4) int32 {down, up, right, left} per sample"""
    r0, r1, c0, c1 = box
    reach = (H - 1 - r1, r0, W - 1 - c1, c0)                  # the displaced boundary lands on the last row / column inside
    one = lambda t: np.tile(np.array(t, np.int32), (DILATE_B, 1))
    cases = {"down": one((3, 0, 0, 0)), "up": one((0, 2, 0, 0)), "right": one((0, 0, 4, 0)), "left": one((0, 0, 0, 5)),
             "all": one((1, 2, 3, 4)), "gap": one((0, 0, 1, 1)), "none": one((0, 0, 0, 0)), "reach": one(reach),
             "beyond": one(tuple(t + 1 for t in reach)), "tall": one((H, H + 3, H, H + 1)), "wide": one((H - 1, 1, W, W - 1)),
             "mixed": np.array([(1, 0, 7, 0), (0, 3, 0, 2), (10, 10, 10, 10), (2, 1, 2, 1)], np.int32)}
    return cases


def mask_dilate(masks, thick, mutant=None):
    """out = in + (number of sides whose displaced boundary of the ORIGINAL mask hits the pixel), only on zero pixels, clamped at 1"""
    _check("dilate", mutant)
    B, _, H, W = masks.shape
    out = np.empty_like(masks)
    for b in range(B):
        m = masks[b, 0]
        flat = m.ravel()
        t = [int(v) for v in thick[b]]
        if mutant == "sides_permuted":
            t = [t[1], t[0], t[3], t[2]]
        for y in range(H):
            for x in range(W):
                v = m[y, x]
                acc = v
                if v == 0 or mutant == "grow_nonzero":
                    if t[0] > 0 and y >= t[0] and m[y - t[0], x] != 0:
                        acc += f32(1)
                    if t[1] > 0 and y + t[1] < H and m[y + t[1], x] != 0:
                        acc += f32(1)
                    if mutant == "no_border_guard":     # the flat read runs into the neighbouring row
                        for o in ((y * W + x - t[2]) if t[2] > 0 else -1, (y * W + x + t[3]) if t[3] > 0 else -1):
                            if 0 <= o < H * W and flat[o] != 0:
                                acc += f32(1)
                    else:
                        if t[2] > 0 and x >= t[2] and m[y, x - t[2]] != 0:
                            acc += f32(1)
                        if t[3] > 0 and x + t[3] < W and m[y, x + t[3]] != 0:
                            acc += f32(1)
                out[b, 0, y, x] = acc if (mutant == "no_clamp" or acc <= 1) else f32(1)
    return out


# =================================================================================================================== flow labels
FLOW_THRESH = 3e-3
FLOW_SHAPES = ((24, 36), (5, 260))
FLOW_B = 2
FLOW_WEIGHT_TYPES = ("all", "viz", "valid")


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def flow_P12(K, pose_src, pose_tgt):
    """calc_flow's projection as the train loader forms it on the host (deepim/core/loader.py, TrainDataLoader._stage)"""
    from lib.utils.projection import se3_inverse, se3_mul

    return np.stack([np.matmul(K, se3_mul(t, se3_inverse(s))) for s, t in zip(pose_src, pose_tgt)]).astype(np.float64)


def flow_scene(H, W):
    """B = 2 pairs with a skewed K and rotated poses on both sides: a tilted source plane with 20 % holes that the relative motion
    (a roll about the optical axis + a move towards the camera) spreads past every frame border; the target depth is the source's own
    pz splatted at its rounded pixel with an offset from {0, +-0.5, +-2} x thresh (seen / occluded on either side), then 10 % holes."""
    rng = np.random.default_rng(7 * H + W)
    f = 1.1 * max(H, W)
    K = np.array([[f, 0.03 * f, 0.48 * W], [0, 0.95 * f, 0.53 * H], [0, 0, 1]], np.float64)
    Kinv = np.linalg.inv(K)
    v, u = np.mgrid[0:H, 0:W]
    ds, dt, ps, pt = [], [], [], []
    for b in range(FLOW_B):
        src = np.concatenate([_rot((0.3, -0.5, 0.2), 0.4 + 0.2 * b), [[0.03], [-0.02], [0.8]]], axis=1)
        k = min(1.0, 3.0 * H / W)          # a wide, flat frame: less roll and shift, so that a good part still lands inside
        rel = np.concatenate([_rot((0.15 * k, -0.1 * k, 1.0), (0.45 - 0.8 * b) * k), [[0.02 - 0.05 * b], [-0.03 * k], [-0.33 + 0.05 * b]]], axis=1)
        tgt = np.concatenate([rel[:, :3] @ src[:, :3], (rel[:, :3] @ src[:, 3] + rel[:, 3]).reshape(3, 1)], axis=1)
        src, tgt = src.astype(f32), tgt.astype(f32)
        d = (0.8 + 0.05 * (u - W / 2) / W - 0.08 * (v - H / 2) / H).astype(f32)
        d[rng.random((H, W)) < 0.2] = 0
        P = flow_P12(K, [src], [tgt])[0]
        tg = np.zeros((H, W), f32)
        offs = np.array([0, 0.5, -0.5, 2, -2]) * FLOW_THRESH
        for y in range(H):
            for x in range(W):
                if d[y, x] == 0:
                    continue
                X = float(d[y, x]) * (Kinv @ np.array([x, y, 1.0]))
                xp = P @ np.append(X, 1.0)
                pz = xp[2] + 1e-15
                cw, ch = np.round(xp[0] / pz), np.round(xp[1] / pz)
                if 0 <= cw < W and 0 <= ch < H:
                    tg[int(ch), int(cw)] = f32(pz + offs[rng.integers(0, 5)])
        tg[rng.random((H, W)) < 0.1] = 0
        ds.append(d), dt.append(tg), ps.append(src), pt.append(tgt)
    return {"K": K, "Kinv": Kinv, "depth_src": np.stack(ds)[:, None], "depth_tgt": np.stack(dt)[:, None], "pose_src": np.stack(ps),
            "pose_tgt": np.stack(pt), "P12": flow_P12(K, ps, pt)}


def flow_half_scene():
    """projections that are EXACT half-integers: Kinv = I, depth 16 and P = [I | 0] + a shift of the third column give pz = 16 + 1e-15
    = 16 (absorbed: half an ulp of 16 is 1.8e-15) and (pw, ph) = (u + a, v + c) with a, c = +0.5 (sample 0) / -0.5 (sample 1).  The
    target holds depth only at even rows and columns: np.round's half-to-even finds it for every in-frame source pixel, half away from
    zero lands on an odd column / row (a hole) for every even u or v, or at -1 (outside, where half-to-even gives -0 -> pixel 0).  thresh = 2^-8 is exact in
    float32 next to 16: target pixel (0, 0) sits at EXACTLY pz + thresh (not seen: the test is `<`), pixel (2, 2) at pz + thresh / 2.
    Sample 2 has P = 0: every source pixel projects to pz = 1e-15 at pixel (0, 0) of an all-hole target, where |0 - pz| < thresh holds
    and only the hole test |dt| > 1e-10 keeps it unseen."""
    H, W, B = 4, 8, 3
    thresh = 2.0 ** -8
    d = np.full((B, 1, H, W), 16, f32)
    tg = np.zeros((B, 1, H, W), f32)
    tg[:2, :, 0::2, 0::2] = 16
    tg[:2, :, 0, 0] = 16 + thresh
    tg[:2, :, 2, 2] = 16 + thresh / 2
    P = np.zeros((B, 3, 4))
    P[:2, 0, 0] = P[:2, 1, 1] = P[:2, 2, 2] = 1
    P[0, 0, 2], P[0, 1, 2] = 0.5, 0.5
    P[1, 0, 2], P[1, 1, 2] = -0.5, -0.5
    return {"Kinv": np.eye(3), "depth_src": d, "depth_tgt": tg, "P12": P, "thresh": thresh}


def flow_labels(depth_src, depth_tgt, P12, Kinv, thresh=FLOW_THRESH, standard_rep=False, weight_type="viz", mutant=None):
    """float64 per pixel -> {"flow" (B,2,H,W) f64, "visible" (B,1,H,W), "weights" (B,2,H,W), "tie" (B,1,H,W) bool, "valid", "inside"}.
    tie: | |dt - pz| - thresh | < 1e-9 or a projected coordinate within 1e-9 of a half-integer (valid source pixels only)"""
    _check("flow", mutant)
    B, _, H, W = depth_src.shape
    flow = np.zeros((B, 2, H, W))
    vis = np.zeros((B, 1, H, W), f32)
    wts = np.zeros((B, 2, H, W), f32)
    tie = np.zeros((B, 1, H, W), bool)
    inside = np.zeros((B, 1, H, W), bool)
    rnd = (lambda x: np.sign(x) * np.floor(np.abs(x) + 0.5)) if mutant == "round_half_away" else np.round
    Kinv = np.asarray(Kinv, np.float64).reshape(3, 3)
    for b in range(B):
        P = np.asarray(P12[b], np.float64)
        for v in range(H):
            for u in range(W):
                ds = depth_src[b, 0, v, u]
                if ds == 0 and mutant is None:       # a hole: never seen, flow 0 (the general path below says the same, slowly)
                    wts[b, :, v, u] = 0 if weight_type == "viz" else 1
                    continue
                d = float(ds)
                r = Kinv[:, 0] * u + Kinv[:, 1] * v + Kinv[:, 2]
                X = d * r
                xp = P[:, 0] * X[0] + P[:, 1] * X[1] + P[:, 2] * X[2] + P[:, 3]
                pz = xp[2] + 1e-15
                pw, ph = xp[0] / pz, xp[1] / pz
                seen = False
                if ds != 0:
                    cw, ch = rnd(pw), rnd(ph)
                    ok = 0 <= cw < W and 0 <= ch < H
                    inside[b, 0, v, u] = ok
                    tie[b, 0, v, u] = abs(pw - np.floor(pw) - 0.5) < 1e-9 or abs(ph - np.floor(ph) - 0.5) < 1e-9
                    if mutant == "clamp_outside":
                        cw, ch, ok = min(max(cw, 0), W - 1), min(max(ch, 0), H - 1), True
                    if ok:
                        dt = float(depth_tgt[b, 0, int(ch), int(cw)])
                        gap = abs(dt - pz)
                        tie[b, 0, v, u] |= abs(gap - thresh) < 1e-9
                        seen = (gap <= thresh if mutant == "thresh_le" else gap < thresh) and (mutant == "no_hole_test" or abs(dt) > 1e-10)
                fw, fh = (pw - u, ph - v) if seen else (0.0, 0.0)
                first_w = bool(standard_rep) != (mutant == "channels_swapped")
                flow[b, :, v, u] = (fw, fh) if first_w else (fh, fw)
                vis[b, 0, v, u] = seen
                if weight_type == "all":
                    w = 1
                elif weight_type == "viz":
                    w = seen
                else:
                    w = seen or (ds == 0 and mutant != "valid_without_d0")
                wts[b, :, v, u] = w
    return {"flow": flow, "visible": vis, "weights": wts, "tie": tie, "valid": depth_src != 0, "inside": inside}


def ulp32(x):
    """the spacing of float32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(f32)).astype(np.float64)


# =================================================================================================================== point clouds
POINT_SIZES = (1, 255, 257)
POINT_B = 3


def point_inputs(n):
    """three classes of 300, 40 and 270 points in one table; sample 0 draws from the 40-point class (slots past 40 are -1), sample 1 is
    all -1, sample 2 draws from the last class; rotated poses"""
    rng = np.random.default_rng(50 + n)
    sizes = (300, 40, 270)
    table = (rng.normal(size=(sum(sizes), 3)) * 0.05).astype(f32)
    off = np.array([300, 0, 340], np.int32)
    idx = np.full((POINT_B, n), -1, np.int32)
    keep = rng.permutation(40)[:min(40, n)]
    idx[0, :len(keep)] = keep
    idx[2] = rng.permutation(270)[:n] if n <= 270 else -1
    if n == 1:
        idx[0, 0], idx[2, 0] = 39, 269           # the last point of a class
    pose = np.stack([np.concatenate([_rot(rng.normal(size=3), 0.5 + b), rng.normal(size=(3, 1)) * 0.3 + [[0], [0], [0.8]]], axis=1)
                     for b in range(POINT_B)]).astype(f32)
    return {"table": table, "table_off": off, "idx": idx, "pose": pose}


def point_clouds(table, table_off, idx, pose, mutant=None):
    """-> model (B,3,n) f32, weights (B,3,n) f32, observed (B,3,n) float64 = R p + t"""
    _check("points", mutant)
    B, n = idx.shape
    model, weights, observed = np.zeros((B, 3, n), f32), np.zeros((B, 3, n), f32), np.zeros((B, 3, n))
    for b in range(B):
        T = pose[b].astype(np.float64)
        R = T[:, :3].T if mutant == "pose_transposed" else T[:, :3]
        for j in range(n):
            i = int(idx[b, j])
            if i < 0 and mutant == "negative_reads_0":
                i = 0
            p = np.zeros(3, f32)
            if i >= 0:
                p = table[(0 if mutant == "no_table_off" else int(table_off[b])) + i]
            model[b, :, j] = p
            weights[b, :, j] = 1 if (idx[b, j] >= 0 or mutant == "padded_weight_1") else 0
            observed[b, :, j] = R @ p.astype(np.float64) + T[:, 3]
    return model, weights, observed


# =================================================================================================================== bbox + zoom window
BBOX_SHAPES = ((13, 36), (21, 260))      # two / three 8-row groups, the last one partial
ZOOM_MEANS = np.array([122.75, 116.0, 102.5], f32)     # per PLANE (R, G, B); multiples of 1/4 so that mode 1 sums are exact


def bbox_inputs(H, W, mode):
    """(x (B,C,H,W), thr, means3 or None): a single pixel in each corner (4 samples), a sample whose only bright pixels sit EXACTLY at the
    threshold except one just above it, an empty sample, a block.  mode 0: C = 1, the plane itself; mode 1: C = 3, x + means summed over
    the planes (threshold 0.5: with these means every sum below is exact in float32)."""
    thr = f32(0.3) if mode == 0 else f32(0.5)
    B = 7
    val = np.zeros((B, H, W), f32)
    for b, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        val[b, y, x] = 1
    val[4, 2:H - 1, 1:W - 2:3] = thr
    # just above: the next float32 (mode 0) / the next value that survives the round trip through x - mean (mode 1: 2^-17 steps at 122)
    val[4, H - 3, 6] = np.nextafter(thr, f32(1)) if mode == 0 else thr + f32(2.0 ** -16)
    val[6, 3:H - 4, 5:W - 9] = 0.75
    if mode == 0:
        return val[:, None].copy(), float(thr), None
    x = np.zeros((B, 3, H, W), f32)
    x[:, 0] = val * f32(0.5)
    x[:, 2] = val * f32(0.5)
    x[4, 0], x[4, 2] = val[4], 0               # keep the next-after value in one plane (halving it would still be exact, this is plainer)
    return (x - ZOOM_MEANS.reshape(1, 3, 1, 1)).astype(f32), float(thr), ZOOM_MEANS.copy()


def bbox_pairs(H, W, mode):
    """observed / rendered boxes for the zoom window: the builder's samples against a rotation of themselves -> corner boxes, an empty
    rendered box (sample 6 against 5), an empty observed box (5 against 4), both empty never (the reference has no such case)"""
    x, thr, means = bbox_inputs(H, W, mode)
    return x, np.roll(x, 1, axis=0), thr, means


def zoom_factor_pose(B, H, W):
    K = np.array([[1.2 * W, 0, 0.5 * W - 0.7], [0, 1.1 * W, 0.5 * H + 0.4], [0, 0, 1]], f32)
    rng = np.random.default_rng(3)
    pose = np.tile(np.eye(3, 4, dtype=f32), (B, 1, 1))
    pose[:, :, 3] = np.stack([rng.uniform(-0.15, 0.15, B), rng.uniform(-0.1, 0.1, B), rng.uniform(0.5, 1.2, B)], axis=1)
    return pose, K


def mask_bbox(x, thr, mode, means3=None):
    B, C, H, W = x.shape
    if mode == 0:
        s = x[:, 0]
    else:
        m = np.asarray(means3, f32)
        s = ((x[:, 0] + m[0]) + (x[:, 1] + m[1])) + (x[:, 2] + m[2])
    return np.stack([bbox_of(s[b] > f32(thr)) for b in range(B)])


def zoom_factor(bbox_obs, bbox_ren, src_pose, K, H, W):
    """the zoom window of oracle.zoom.zoom_factor_from_valid from the two boxes (any mask with the same box gives the same window);
    an empty observed box -> factor (1, 1, 0, 0), status bit 0 (the reference raises there); empty rendered box -> status bit 1"""
    from oracle import zoom as ozoom

    B = len(bbox_obs)
    zf, status = np.zeros((B, 4), f32), np.zeros(B, np.int32)

    def corners(box):
        m = np.zeros((1, H, W), bool)
        if box[1] >= 0:
            m[0, box[2], box[0]] = m[0, box[3], box[1]] = True
        return m
    for b in range(B):
        status[b] = (1 if bbox_obs[b][1] < 0 else 0) | (2 if bbox_ren[b][1] < 0 else 0)
        if status[b] & 1:
            zf[b] = (1, 1, 0, 0)
        else:
            zf[b] = ozoom.zoom_factor_from_valid(corners(bbox_obs[b]), corners(bbox_ren[b]), src_pose[b:b + 1], K, H, W)[0][0]
    return zf, status


# =================================================================================================================== zoom sampling
ZOOM_B = 5
ZOOM_PLANES_SHAPE = (17, 37)
NET_INPUT_SHAPES = ((16, 36), (9, 128), (6, 260))     # block 256 with idle lanes, block 128, block 256 across two blocks
# zoom in (wy != wx); exact identity (integer coordinates: the right / bottom corner has weight 0 and is out of range in the last column
# / row); a window larger than the frame and shifted (zero padding on several sides); far outside (every corner invalid); 1e30 (the
# clamp before the int cast)
ZOOM_FACTORS = np.array([[0.3, 0.4, 0.1, -0.05], [1, 1, 0, 0], [1.7, 1.7, 0.6, -0.4], [1, 1, 5, 0], [1e30, 1e30, 0, 0]], f32)


def inverse_zoom_factor(zf, H, W):
    """zoom_flow.py:35-44 in explicit float32, one rounding per operation, as load_affine of csrc/zoom.hip documents"""
    zf = np.asarray(zf, f32).reshape(-1, 4)
    wx_in, wy_in, tx_in, ty_in = zf[:, 0], zf[:, 1], zf[:, 2], zf[:, 3]
    Wf, Hf, half, two, one = f32(W), f32(H), f32(0.5), f32(2), f32(1)
    wx, wy = one / wx_in, one / wy_in
    crop_w, crop_h = wx_in * Wf, wy_in * Hf
    cx = ((tx_in * half) * Wf) + (half * Wf)
    cy = ((ty_in * half) * Hf) + (half * Hf)
    tx = (((Wf * half) - cx) / crop_w) * two
    ty = (((Hf * half) - cy) / crop_h) * two
    out = np.stack([wx, wy, tx, ty], axis=1)
    assert out.dtype == f32
    return out


def mx_round(x, mutant=None):
    x = np.asarray(x, f32)
    if mutant == "round_half_even":
        return np.round(x)
    return np.copysign(np.floor(np.abs(x) + f32(0.5)), x).astype(f32)


def round_boundary_distance_ulps(pre):
    """how many float32 ulps the pre-round value lies from the nearest k + 0.5"""
    a = np.abs(np.asarray(pre, f32)).astype(np.float64)
    return np.abs(a - (np.floor(a) + 0.5)) / ulp32(a + 0.5)


def zoom_sample(x, zf, add=None, pre=0, inverse=False, mutant=None):
    """x (B,C,H,W) f32 -> sample(pre(x) + add) - add, un-rounded, float32 with one rounding per operation:
       x_t = -1 + j * f32(2 / (W - 1));  x_s = wx * x_t + tx;  x_r = (x_s + 1) * (W - 1) / 2;  weights 1 - (x_r - floor x_r);
       out = tl wy0 wx0 + tr wy0 (1 - wx0) + bl (1 - wy0) wx0 + br (1 - wy0)(1 - wx0), corners outside the plane contribute 0"""
    _check("zoom", mutant)
    x = np.asarray(x, f32)
    B, C, H, W = x.shape
    zf = np.asarray(zf, f32).reshape(B, 4)
    if inverse and mutant != "forward_for_inverse":
        zf = inverse_zoom_factor(zf, H, W)
    add = np.zeros(C, f32) if add is None else np.asarray(add, f32)
    one = f32(1)
    gw, gh = (W, H) if mutant == "grid_W" else (W - 1, H - 1)
    xt = f32(-1) + np.arange(W, dtype=f32) * f32(2.0 / gw)
    yt = f32(-1) + np.arange(H, dtype=f32) * f32(2.0 / gh)
    out = np.empty_like(x)
    for b in range(B):
        wx, wy, tx, ty = zf[b]
        with np.errstate(over="ignore", invalid="ignore"):
            xr = (((wx * xt + tx) + one) * f32(W - 1)) / f32(2)
            yr = (((wy * yt + ty) + one) * f32(H - 1)) / f32(2)
        x0f, y0f = np.floor(xr), np.floor(yr)
        wx0 = (one - (xr - x0f))[None, :]
        wy0 = (one - (yr - y0f))[:, None]
        x0 = np.clip(x0f, -2, W + 1).astype(np.int64)
        y0 = np.clip(y0f, -2, H + 1).astype(np.int64)
        for c in range(C):
            p = x[b, c]
            if pre == 1:
                p = np.where((p >= f32(0.2)) if mutant == "bin_ge" else (p > f32(0.2)), one, f32(0))
            p = p + add[c]

            def corner(yy, xx):
                vy, vx = (yy >= 0) & (yy <= H - 1), (xx >= 0) & (xx <= W - 1)
                v = p[np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]]
                return v if mutant == "corner_clamped" else np.where(vy[:, None] & vx[None, :], v, f32(0))
            tl, tr, bl, br = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
            wx1, wy1 = one - wx0, one - wy0
            r = (tl * wy0) * wx0
            r = r + (tr * wy0) * wx1
            r = r + (bl * wy1) * wx0
            r = r + (br * wy1) * wx1
            out[b, c] = r if mutant == "mean_kept" else r - add[c]
    assert out.dtype == f32
    return out


def zoom_post(v, zf, post=0, scale_mode=0, mutant=None):
    """(value as dim_zoom_planes writes it, the value before rounding or None)"""
    v = np.asarray(v, f32)
    before = None
    if post == 1:
        before, v = v, mx_round(v, mutant)
    elif post == 2:
        before = v - f32(0.45)
        v = mx_round(before, mutant)
    s = np.asarray(zf, f32).reshape(-1, 4)[:, 1 if mutant == "scale_wy" else 0].reshape(-1, 1, 1, 1)
    if scale_mode == 1:
        v = v / s
    elif scale_mode == 2:
        v = v * s
    return v.astype(f32), before


def zoom_planes(x, zf, inverse=False, pre=0, post=0, add3=None, scale_mode=0, mutant=None):
    add = None if (add3 is None or x.shape[1] > 3) else add3
    return zoom_post(zoom_sample(x, zf, add, pre, inverse, mutant), zf, post, scale_mode, mutant)


def zoom_inputs(H, W, seed=0):
    """8-bit images minus the plane means, a depth-like mask (0 outside, values that hit the binarise threshold 0.2 and the rounding
    boundaries 0.5 / 1.5 / 2.5 exactly, others in between), a 0/1 mask, a flow-like plane pair"""
    rng = np.random.default_rng(31 * H + W + seed)
    B = ZOOM_B
    mean = ZOOM_MEANS.reshape(1, 3, 1, 1)
    io = (rng.integers(0, 256, size=(B, 3, H, W)).astype(f32) - mean).astype(f32)
    ir = (rng.integers(0, 256, size=(B, 3, H, W)).astype(f32) - mean).astype(f32)
    ir[:, :, : H // 3] = (0 - mean).astype(f32)                                  # rendered background: raw 0
    table = np.array([0, 0, 0, 0.2, 0.5, 1.5, 2.5, 0.19, 0.21, 0.7, 1.0, 1.2], f32)
    depth_like = table[rng.integers(0, len(table), size=(B, 1, H, W))]
    binary = (rng.random((B, 1, H, W)) < 0.5).astype(f32)
    yy, xx = np.mgrid[0:H, 0:W]
    binary[:, 0] *= ((yy - H / 2) ** 2 / (H / 2.2) ** 2 + (xx - W / 2) ** 2 / (W / 2.2) ** 2 < 1.5)
    binary[:, 0, 0, :] = 1
    binary[:, 0, :, W - 1] = 1
    flow = (rng.normal(size=(B, 2, H, W)) * 5).astype(f32)
    return {"io": io, "ir": ir, "depth_like": depth_like, "binary": binary, "flow": flow}


def net_input(io, ir, eo, er, zf, means, mode, mutant=None):
    """dim_zoom_net_input_ex: X (B,H,W,8) NHWC + the four NCHW tensors of mode 0 (z_img_obs, z_img_ren, z_mask_obs, z_mask_ren) +
    the pre-round values of the two mask lanes (None where the mode does not round)
      mode 0: [img_obs / 255 x3, img_ren / 255 x3, round(mask_obs), round(bin02(mask_ren))]
      mode 1: [img_obs / 255 x3, img_ren / 255 x3, 0, 0]
      mode 2: [img_obs / 255 x3, img_ren / 255 x3, extra_obs / 255, extra_ren / 255]   (plain samples)
      mode 3: [round(mask_obs), round(bin02(mask_ren)), 0 x 6]"""
    _check("net_input", mutant)
    B, _, H, W = io.shape
    X = np.zeros((B, H, W, 8), f32)
    c255 = f32(255)
    zio = zoom_sample(io, zf, means)
    zir = zoom_sample(ir, zf, means)
    pre_o = pre_r = zmo = zmr = None
    if mode != 3:
        X[..., 0:3] = (zio / c255).transpose(0, 2, 3, 1)
        X[..., 3:6] = (zir / c255).transpose(0, 2, 3, 1)
    if mode in (0, 3):
        pre_o, pre_r = zoom_sample(eo, zf), zoom_sample(er, zf, pre=1)
        zmo, zmr = mx_round(pre_o), mx_round(pre_r)
        lo = 6 if mode == 0 else (2 if mutant == "mode3_lanes" else 0)
        X[..., lo], X[..., lo + 1] = zmo[:, 0], zmr[:, 0]
    elif mode == 2:
        a, b = zoom_sample(eo, zf)[:, 0], zoom_sample(er, zf)[:, 0]
        if mutant != "mode2_no_255":
            a, b = a / c255, b / c255
        if mutant == "mode2_lanes":
            a, b = b, a
        X[..., 6], X[..., 7] = a, b
    elif mode == 1 and mutant == "mode1_lanes" and eo is not None:
        X[..., 6], X[..., 7] = mx_round(zoom_sample(eo, zf))[:, 0], mx_round(zoom_sample(er, zf, pre=1))[:, 0]
    return {"X": X, "nchw": (zio, zir, zmo, zmr), "pre_round": (pre_o, pre_r)}
