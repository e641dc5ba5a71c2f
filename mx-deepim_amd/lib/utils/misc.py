"""depth_im_to_dist_im with the reference's name (lib/utils/misc.py), numpy host code."""
from __future__ import print_function, division

import numpy as np


def depth_im_to_dist_im(depth_im, K):
    """depth image (Z of the point behind every pixel, 0 = none) -> float64 distance of that point from the camera centre:
    X = ((x - cx) Z) (1 / fx), Y = ((y - cy) Z) (1 / fy), S = sqrt((X X + Y Y) + Z Z), x / y the integer pixel indices"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    d = np.asarray(depth_im).astype(np.float64)
    xs = np.arange(d.shape[1], dtype=np.float64)[None, :]
    ys = np.arange(d.shape[0], dtype=np.float64)[:, None]
    X = ((xs - K[0, 2]) * d) * (1.0 / K[0, 0])
    Y = ((ys - K[1, 2]) * d) * (1.0 / K[1, 1])
    return np.sqrt((X * X + Y * Y) + d * d)
