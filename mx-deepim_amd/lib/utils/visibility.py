"""Visibility masks of the visible surface discrepancy (Hodan et al.), with the reference's names (lib/utils/visibility.py),
numpy host code.  All images are distance images (lib/utils/misc.py depth_im_to_dist_im), 0 = no surface.  The device computes
the same masks inside dim_vsd_errors (csrc/vsd.hip)."""
from __future__ import print_function, division

import numpy as np


def estimate_visib_mask(d_test, d_model, delta):
    """the model surface is visible where both images hold a surface and the model is at most delta behind the scene; the
    difference and the comparison are float32 (delta rounded to float32)"""
    assert d_test.shape == d_model.shape
    both = (d_test > 0) & (d_model > 0)
    behind = d_model.astype(np.float32) - d_test.astype(np.float32)
    return (behind <= np.float32(delta)) & both


def estimate_visib_mask_gt(d_test, d_gt, delta):
    return estimate_visib_mask(d_test, d_gt, delta)


def estimate_visib_mask_est(d_test, d_est, visib_gt, delta):
    """the estimate counts as visible also where the ground truth is visible and the estimate draws anything"""
    return estimate_visib_mask(d_test, d_est, delta) | (visib_gt & (d_est > 0))
