"""Plain-loop numpy restatement of the scene composition rule (csrc/scene.hip), its counts and boxes, and of the LINEMOD light draw
(lib/utils/synthetic.py lm_light_draw; toolkit/LM6d_occ_dsm_1_gen_observed_light.py:130-162 of the reference).  Written from the
rule, one pixel and one layer at a time; shares no code with the kernel or the host layer."""
import math

import numpy as np


def compose(layer_bgr, layer_depth, layer_label, S):
    """layer_bgr (N*S,H,W,3) f32, layer_depth (N*S,1,H,W) f32, layer_label (N*S,) int -> dict of
    scene_bgr (N,H,W,3), scene_depth (N,1,H,W), scene_label (N,1,H,W), vis_mask (N*S,1,H,W), counts (N*S,2) int32 {full, visible},
    vis_bbox (N*S,4) int32 {min x, max x, min y, max y}, empty = {W, -1, H, -1}.
    Winner of a pixel: the used layer (label > 0) with the smallest depth that is finite and > 0; a tie goes to the lower slot."""
    NS, _, H, W = layer_depth.shape
    N = NS // S
    out = {"scene_bgr": np.zeros((N, H, W, 3), np.float32), "scene_depth": np.zeros((N, 1, H, W), np.float32),
           "scene_label": np.zeros((N, 1, H, W), np.float32), "vis_mask": np.zeros((NS, 1, H, W), np.float32),
           "counts": np.zeros((NS, 2), np.int32), "vis_bbox": np.zeros((NS, 4), np.int32)}
    out["vis_bbox"][:] = [W, -1, H, -1]
    for n in range(N):
        for y in range(H):
            for x in range(W):
                win, best = -1, 0.0
                for s in range(S):
                    l = n * S + s
                    if layer_label[l] <= 0:
                        continue
                    d = float(layer_depth[l, 0, y, x])
                    if d > 0:
                        out["counts"][l, 0] += 1
                    if not (math.isfinite(d) and d > 0):
                        continue
                    if win < 0 or d < best:
                        win, best = s, d
                if win < 0:
                    continue
                l = n * S + win
                out["scene_bgr"][n, y, x] = layer_bgr[l, y, x]
                out["scene_depth"][n, 0, y, x] = layer_depth[l, 0, y, x]
                out["scene_label"][n, 0, y, x] = float(layer_label[l])
                out["vis_mask"][l, 0, y, x] = 1.0
                out["counts"][l, 1] += 1
                b = out["vis_bbox"][l]
                b[0], b[1], b[2], b[3] = min(b[0], x), max(b[1], x), min(b[2], y), max(b[3], y)
    return out


LIGHT_DIRS = [[1, 0, 1], [1, 1, 1], [0, 1, 1], [-1, 1, 1], [-1, 0, 1], [0, 0, 1]]
LIGHT_COLORS = [[0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]


def light_from_draws(idx, pose_0, factors, colour_row, ratio_index):
    """the reference rule applied to given draws: position = dir[idx % 6] * 0.5 + (tx, -ty, -tz), intensity = colour * factors"""
    pos = [0.5 * LIGHT_DIRS[idx % 6][0] + pose_0[0][3], 0.5 * LIGHT_DIRS[idx % 6][1] - pose_0[1][3], 0.5 * LIGHT_DIRS[idx % 6][2] - pose_0[2][3]]
    inten = [LIGHT_COLORS[colour_row][i] * factors[i] for i in range(3)]
    return np.array(pos, np.float64), np.array(inten, np.float64), ratio_index


def light_draw(seed, idx, pose_0, n_ratios=5):
    """the documented draw order of lm_light_draw: uniform(0.8, 1.2, 3), integers(0, 7), integers(0, n_ratios)"""
    rng = np.random.default_rng(seed)
    factors = rng.uniform(0.8, 1.2, size=3)
    c = int(rng.integers(0, 7))
    k = int(rng.integers(0, n_ratios))
    return light_from_draws(idx, pose_0, factors, c, k)
