"""numpy restatement of the tracker's colour-histogram segmentation, written from the rule in include/deepim_hip.h (section
"Colour-histogram segmentation of the tracks"), not from csrc/track_seg.hip.

  color_bins     frame_bgr (H,W,3) uint8 -> the colour bin of every pixel
  region         a box grown by the margin and clipped -> (x0, x1, y0, y1) inclusive, or None
  raw_mask       the unfiltered decision of one track: in the region, a model, foreground histogram > background histogram (float32)
  majority       the integer majority filter, as separable box sums (majority_brute: the definition, pixel by pixel)
  seg_mask       dim_track_seg_mask: mask (P,1,H,W) float32, counts (P,2) int32, status bits (P,) int32
  seg_learn      dim_track_seg_learn on copies of the state: float32 division, subtraction, multiplication and addition, each rounded once
"""
import numpy as np

STATUS_TRACK_SEG_NO_MODEL = 131072
AGE_CAP = 1 << 30


def color_bins(frame_bgr, bits):
    f = np.asarray(frame_bgr, np.uint8).astype(np.int64)
    s = 8 - bits
    return ((f[..., 0] >> s) << (2 * bits)) | ((f[..., 1] >> s) << bits) | (f[..., 2] >> s)


def region(box, margin, H, W):
    min_x, max_x, min_y, max_y = (int(v) for v in box)
    if max_x < min_x or max_y < min_y:
        return None
    x0, x1 = max(min_x - margin, 0), min(max_x + margin, W - 1)
    y0, y1 = max(min_y - margin, 0), min(max_y + margin, H - 1)
    if x1 < x0 or y1 < y0:
        return None
    return x0, x1, y0, y1


def region_plane(reg, H, W):
    m = np.zeros((H, W), bool)
    if reg is not None:
        x0, x1, y0, y1 = reg
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def raw_mask(bins, reg, hist_p, age_p, H, W):
    """(H,W) bool.  hist_p (2,NB) float32: the comparison is numpy's float32 `>` (False for a tie and for a NaN on either side)"""
    hist_p = np.asarray(hist_p, np.float32)
    with np.errstate(invalid="ignore"):
        fg_bin = hist_p[0] > hist_p[1]
    return region_plane(reg, H, W) & (int(age_p) > 0) & fg_bin[bins]


def majority(raw, inside, radius):
    """2 * (sum of raw over the (2 radius + 1)^2 window) > (2 radius + 1)^2, inside the region; the sum as row sums of column sums
    of the zero-padded plane (raw is 0 outside the region already)"""
    H, W = raw.shape
    k = 2 * radius + 1
    pad = np.zeros((H + 2 * radius, W + 2 * radius), np.int64)
    pad[radius:radius + H, radius:radius + W] = raw
    cs = np.concatenate([np.zeros((1, pad.shape[1]), np.int64), np.cumsum(pad, axis=0)])
    col = cs[k:] - cs[:-k]                                    # (H, W + 2 radius): sums over k rows
    rs = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(col, axis=1)], axis=1)
    box = rs[:, k:] - rs[:, :-k]                              # (H, W)
    return inside & (2 * box > k * k)


def majority_brute(raw, inside, radius):
    """the definition, one pixel and one neighbour at a time"""
    H, W = raw.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if not inside[y, x]:
                continue
            n = 0
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and inside[yy, xx] and raw[yy, xx]:
                        n += 1
            out[y, x] = 2 * n > (2 * radius + 1) ** 2
    return out


def seg_mask(frame_bgr, bbox, seg_hist, seg_age, bits, margin, radius):
    """-> mask (P,1,H,W) float32, counts (P,2) int32 = {region pixels, mask pixels}, status (P,) int32 (the bits to OR in)"""
    H, W, _ = frame_bgr.shape
    P = len(bbox)
    bins = color_bins(frame_bgr, bits)
    mask, counts, status = np.zeros((P, 1, H, W), np.float32), np.zeros((P, 2), np.int32), np.zeros(P, np.int32)
    for p in range(P):
        reg = region(bbox[p], margin, H, W)
        inside = region_plane(reg, H, W)
        m = majority(raw_mask(bins, reg, seg_hist[p], seg_age[p], H, W), inside, radius)
        mask[p, 0] = m
        counts[p] = (inside.sum(), m.sum())
        if reg is None or int(seg_age[p]) <= 0:
            status[p] = STATUS_TRACK_SEG_NO_MODEL
    return mask, counts, status


def drawn(d):
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def seg_learn(frame_bgr, depth_drawn, depth_fg, bbox, flags, skip_mask, bits, margin, rate, min_pixels, seg_hist, seg_age):
    """-> (seg_hist, seg_age, counts) after one update; the inputs are not modified.  A skipped track keeps its rows bit for bit"""
    H, W, _ = frame_bgr.shape
    P, NB = len(bbox), 1 << (3 * bits)
    bins = color_bins(frame_bgr, bits)
    hist, age = np.array(seg_hist, np.float32, copy=True), np.array(seg_age, np.int32, copy=True)
    counts = np.zeros((P, 2), np.int32)
    rate = np.float32(rate)
    for p in range(P):
        inside = region_plane(region(bbox[p], margin, H, W), H, W)
        dd = drawn(depth_drawn[p, 0])
        fore = inside & (dd if depth_fg is None else drawn(depth_fg[p, 0]))
        back = inside & ~fore & ~dd
        n = (int(fore.sum()), int(back.sum()))
        counts[p] = n
        if (flags is not None and int(flags[p]) & int(skip_mask)) or n[0] < min_pixels or n[1] < min_pixels:
            continue
        for k, sel in enumerate((fore, back)):
            h = np.bincount(bins[sel], minlength=NB).astype(np.float32) / np.float32(n[k])
            if age[p] <= 0:
                hist[p, k] = h
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    hist[p, k] = hist[p, k] + rate * (h - hist[p, k])
        age[p] = min(max(int(age[p]), 0) + 1, AGE_CAP)
    return hist, age, counts


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    u = (a | b).sum()
    return float((a & b).sum()) / u if u else 1.0
