"""Pose-error functions with the reference's names (lib/utils/pose_error.py:55-147), numpy host code (evaluation is not on
the device path).  re() uses the closed form of ||logm(R_est^T R_gt)||_F / sqrt(2) = the rotation angle."""
from __future__ import print_function, division

import numpy as np
from scipy import spatial


def transform_pts_Rt(pts, R, t):
    assert pts.shape[1] == 3
    return (R.dot(pts.T) + t.reshape((3, 1))).T


def transform_pts_Rt_2d(pts, R, t, K):
    assert pts.shape[1] == 3
    pts_c_t = K.dot(R.dot(pts.T) + t.reshape((3, 1)))
    return (pts_c_t[:2] / pts_c_t[2:3]).T


def arp_2d(R_est, t_est, R_gt, t_gt, pts, K):
    """average re-projection error in 2d (pixels)"""
    return np.linalg.norm(transform_pts_Rt_2d(pts, R_est, t_est, K) - transform_pts_Rt_2d(pts, R_gt, t_gt, K), axis=1).mean()


def add(R_est, t_est, R_gt, t_gt, pts):
    """Average Distance of Model Points (Hinterstoisser et al., ACCV 2012)"""
    return np.linalg.norm(transform_pts_Rt(pts, R_est, t_est) - transform_pts_Rt(pts, R_gt, t_gt), axis=1).mean()


def adi(R_est, t_est, R_gt, t_gt, pts):
    """Average Distance of Model Points for objects with indistinguishable views (nearest neighbour)"""
    pts_est = transform_pts_Rt(pts, R_est, t_est)
    pts_gt = transform_pts_Rt(pts, R_gt, t_gt)
    nn_dists, _ = spatial.cKDTree(pts_est).query(pts_gt, k=1)
    return nn_dists.mean()


def _transform_pts_sym(pts, R, t, sym):
    """the model points moved by the symmetry [S_R | S_t], then by the pose"""
    sym = np.asarray(sym, dtype=np.float64)
    return transform_pts_Rt(transform_pts_Rt(pts, sym[:, :3], sym[:, 3]), R, t)


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance (Hodan et al., BOP 2019): the largest distance between a model point under the
    estimate and under the ground truth, minimised over the symmetries syms (S,3,4) of the model"""
    pts_est = transform_pts_Rt(pts, R_est, t_est)
    return min(np.linalg.norm(pts_est - _transform_pts_sym(pts, R_gt, t_gt, sym), axis=1).max() for sym in syms)


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance (BOP 2019), pixels: mssd on the projections K (R p + t) / z"""
    proj_est = transform_pts_Rt_2d(pts, R_est, t_est, K)
    es = []
    for sym in syms:
        sym = np.asarray(sym, dtype=np.float64)
        proj_gt = transform_pts_Rt_2d(transform_pts_Rt(pts, sym[:, :3], sym[:, 3]), R_gt, t_gt, K)
        es.append(np.linalg.norm(proj_est - proj_gt, axis=1).max())
    return min(es)


def re(R_est, R_gt):
    """rotation error in degrees"""
    assert R_est.shape == R_gt.shape == (3, 3)
    c = (np.trace(np.dot(np.transpose(R_est), R_gt)) - 1.0) / 2.0
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def te(t_est, t_gt):
    assert t_est.size == t_gt.size == 3
    return np.linalg.norm(np.asarray(t_gt).reshape(3) - np.asarray(t_est).reshape(3))


def calc_rt_dist_m(pose_src, pose_tgt):
    """lib/pair_matching/RT_transform.py:172-183: (rotation distance in degrees, translation distance)"""
    return re(pose_src[:, :3], pose_tgt[:, :3]), np.linalg.norm(pose_tgt[:, 3] - pose_src[:, 3])


VSD_COSTS = ("step", "tlinear")


def vsd(depth_est, depth_gt, depth_test, K, delta, tau, cost_type="step"):
    """Visible surface discrepancy (Hodan et al.) of one pose from three depth planes (metres, 0 = no surface): the model rendered
    at the estimate and at the ground truth, and the test image.  Only the surface visible in the test image is compared
    (lib/utils/visibility.py): on the pixels visible under both poses the cost of c = |S_gt - S_est| is 1 where c >= tau ("step") or
    min(c / tau, 1) ("tlinear"), a pixel visible under one pose only costs 1, and the error is the mean cost over the union.
    -> (e, (|visib_gt|, |union|, |inter|)); e = 1.0 when nothing is visible.  dim_vsd_errors (csrc/vsd.hip) is the device's."""
    from lib.utils.misc import depth_im_to_dist_im
    from lib.utils.visibility import estimate_visib_mask_est, estimate_visib_mask_gt

    if cost_type not in VSD_COSTS:
        raise ValueError("vsd cost_type must be one of {}, got {!r}".format(VSD_COSTS, cost_type))
    s_test, s_gt, s_est = (depth_im_to_dist_im(d, K) for d in (depth_test, depth_gt, depth_est))
    visib_gt = estimate_visib_mask_gt(s_test, s_gt, delta)
    visib_est = estimate_visib_mask_est(s_test, s_est, visib_gt, delta)
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    n_gt, n_union, n_inter = int(visib_gt.sum()), int(union.sum()), int(inter.sum())
    if n_union == 0:
        return 1.0, (n_gt, 0, 0)
    c = np.abs(s_gt[inter] - s_est[inter])
    costs = (c >= tau).astype(np.float64) if cost_type == "step" else np.minimum(c * (1.0 / tau), 1.0)
    return float((costs.sum() + (n_union - n_inter)) / float(n_union)), (n_gt, n_union, n_inter)
