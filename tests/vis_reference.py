"""The rules of dim_vis_overlay (include/deepim_hip.h) restated in numpy.  Everything behind the base colour is integer arithmetic, so
the kernel gives the same bytes: every comparison against this module is np.array_equal.  A plain module (no fixtures, no GPU)."""
import numpy as np


def inside(layers):
    """(..., H, W) float -> bool: value > 0; a NaN is not inside"""
    with np.errstate(invalid="ignore"):
        return np.asarray(layers) > 0


def edge(ins):
    """(..., H, W) bool -> bool: inside, and at least one 4-neighbour that lies inside the frame is not inside"""
    ins = np.asarray(ins, dtype=bool)
    all_in = np.ones_like(ins)
    all_in[..., 1:, :] &= ins[..., :-1, :]    # the neighbour above (row 0 has none)
    all_in[..., :-1, :] &= ins[..., 1:, :]    # below
    all_in[..., :, 1:] &= ins[..., :, :-1]    # left
    all_in[..., :, :-1] &= ins[..., :, 1:]    # right
    return ins & ~all_in


def marked(edges, radius):
    """(..., H, W) bool -> bool: some edge pixel lies in the (2 radius + 1)^2 square centred on the pixel, clipped to the frame"""
    edges = np.asarray(edges, dtype=bool)
    H, W = edges.shape[-2:]
    out = np.zeros_like(edges)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[..., yd, xd] |= edges[..., ys, xs]
    return out


def base_colour(image, pixel_means_bgr):
    """image_observed blob (B,3,H,W) f32 (plane c = BGR channel 2 - c) -> (B,H,W,3) int64 in B,G,R order"""
    image = np.asarray(image, dtype=np.float32)
    means = np.asarray(pixel_means_bgr, dtype=np.float32).reshape(3)
    out = np.zeros(image.shape[:1] + image.shape[2:] + (3,), dtype=np.int64)
    for c in range(3):
        with np.errstate(invalid="ignore"):
            v = np.rint((image[:, c] + means[2 - c]).astype(np.float32))   # one float32 add, half to even
        out[..., 2 - c] = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0)).astype(np.int64)
    return out


def blend(c, colour, a):
    return (np.asarray(c, dtype=np.int64) * (256 - a) + np.asarray(colour, dtype=np.int64) * a + 128) >> 8


def overlay(image, pixel_means_bgr, layers, style, radius):
    """-> out (B,H,W,3) uint8, counts (B,L,2) int32 = {marked pixels, inside pixels}.  layers (L,B,H,W); style (L,5) ints
    {B, G, R, edge_alpha, fill_alpha}"""
    layers = np.asarray(layers)
    style = np.asarray(style, dtype=np.int64).reshape(layers.shape[0], 5)
    out = base_colour(image, pixel_means_bgr)
    B = out.shape[0]
    counts = np.zeros((B, layers.shape[0], 2), dtype=np.int32)
    for l in range(layers.shape[0]):
        ins = inside(layers[l])
        mk = marked(edge(ins), radius)
        counts[:, l, 0] = mk.reshape(B, -1).sum(1)
        counts[:, l, 1] = ins.reshape(B, -1).sum(1)
        colour, edge_alpha, fill_alpha = style[l, :3], int(style[l, 3]), int(style[l, 4])
        fill = ins & ~mk if fill_alpha > 0 else np.zeros_like(ins)
        out = np.where(mk[..., None], blend(out, colour, edge_alpha), np.where(fill[..., None], blend(out, colour, fill_alpha), out))
    return out.astype(np.uint8), counts
