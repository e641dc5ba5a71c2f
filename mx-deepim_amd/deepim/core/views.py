"""One object seen by several calibrated cameras (TEST.VIEWS = V > 1): a Refiner batch of B = G * V samples holds G groups of V views,
sample b = g * V + v, and cam_T_rig[b] = X_b = [R_b | t_b] maps the rig frame into the camera of sample b.  The network loop stays
per sample; after it ViewsConsensus picks the best-scoring view of each group and gives every view its pose from that one
(dim_views_consensus), and the post-loop stages of deepim.core.pose_stages run their joint (`_views`) entries from there: one
correction per group, so the stage poses of a group agree with the extrinsics by construction.
With TEST.VIEWS_CALIB_ITER > 0 ViewsCalib runs between the two: the rig's extrinsics are refined together with the rig poses
(dim_icp_refine_rig, camera 0 the gauge), and the joint stages then use the calibrated extrinsics and start from its poses.
Here: the checked settings, what the feature cannot be combined with, the checks of load()'s cam_T_rig, the consensus step and the
calibration stage."""
import numpy as np
import torch

from lib.hip import ops

VIEWS_SCORES = ("rgb", "depth")
# the bits that rule a view out of the consensus: the loop's empty boxes and what the rasteriser refused -- what the tracker's lost
# test treats as fatal (deepim.core.tracker.FATAL_MASK).  A stage's "too few points" bit is not among them
FATAL_MASK = 1 | 2 | ops.STATUS_BAD_CLASS | ops.STATUS_BAD_K
RIGID_TOL = 1e-4   # |R^T R - I| of a cam_T_rig row
F32, I32 = torch.float32, torch.int32


def views_settings(cfg, lit=False):
    """-> (VIEWS, VIEWS_SCORE, HYP_DEPTH_TAU) of cfg.TEST, checked; ValueError names the bad key(s).  VIEWS 1 = off: every sample on its
    own.  With VIEWS > 1 the features that own the sample axis or the start pose themselves are refused, naming both keys."""
    T = cfg.TEST
    v = T.get("VIEWS", 1)
    if isinstance(v, bool) or not float(v).is_integer() or not 1 <= int(v) <= ops.VIEWS_MAX:
        raise ValueError("TEST.VIEWS must be an integer in 1..{} (1 = off), got {!r}".format(ops.VIEWS_MAX, v))
    V = int(v)
    score = T.get("VIEWS_SCORE", "rgb")
    if score not in VIEWS_SCORES:
        raise ValueError("TEST.VIEWS_SCORE must be one of {}, got {!r}".format(VIEWS_SCORES, score))
    tau = float(T.get("HYP_DEPTH_TAU", 0.02))
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("TEST.HYP_DEPTH_TAU must be a finite distance > 0 (metres), got {!r}".format(T.get("HYP_DEPTH_TAU")))
    if V > 1:
        for key, off in (("HYP_NUM", 1), ("COARSE_VIEWS", 0), ("FLOW_PNP_ITER", 0)):
            if int(T.get(key, off) or off) > off:
                raise ValueError("TEST.VIEWS > 1 cannot be combined with TEST.{} > {}".format(key, off))
        if lit:
            raise ValueError("TEST.VIEWS > 1 is not supported with the lit ModelNet renderer")
    return V, str(score), tau


def calib_settings(cfg):
    """-> (VIEWS_CALIB_ITER, VIEWS_CALIB_MAX_DIST) of cfg.TEST, checked; ValueError names the bad key(s).  0 iterations = off; the gate
    in metres, ICP_MAX_DIST's value when not given.  On, it needs TEST.VIEWS > 1 (whose own refusals hold as they are)."""
    T = cfg.TEST
    n = T.get("VIEWS_CALIB_ITER", 0) or 0
    if isinstance(n, (bool, str)) or not float(n).is_integer() or int(n) < 0:
        raise ValueError("TEST.VIEWS_CALIB_ITER must be an integer >= 0 (0 = off), got {!r}".format(T.get("VIEWS_CALIB_ITER")))
    given = T.get("VIEWS_CALIB_MAX_DIST", None)
    gate = float(T.get("ICP_MAX_DIST", 0.02) if given is None else given)
    if not (np.isfinite(gate) and gate > 0):
        raise ValueError("TEST.VIEWS_CALIB_MAX_DIST must be a finite distance > 0 (metres), got {!r}".format(given))
    if int(n) > 0 and not views_on(cfg):
        raise ValueError("TEST.VIEWS_CALIB_ITER > 0 needs TEST.VIEWS > 1 (the extrinsics of one camera are not observable)")
    return int(n), gate


def views_on(cfg):
    return int(cfg.TEST.get("VIEWS", 1) or 1) > 1


def refuse_with_views(cfg, what):
    """`what` (load_staged, the Tracker, pred_eval) has no meaning for groups of views: a ValueError naming TEST.VIEWS and it"""
    if views_on(cfg):
        raise ValueError("TEST.VIEWS > 1 is not supported by {}".format(what))


def refuse_views_at_source_size(cfg, size, net_size):
    """the consensus renders and scores every view as the selection among hypotheses does, which exists at the network size only"""
    if views_on(cfg) and tuple(size) != tuple(net_size):
        raise ValueError("TEST.VIEWS > 1 is built for SCALES [[{}, {}]] only, got SCALES {}x{}: switch it off or shrink the images to the "
                         "network size".format(net_size[0], net_size[1], size[0], size[1]))


def check_cam_T_rig(cam_T_rig, B, V):
    """load()'s cam_T_rig, (V,3,4) (one rig, repeated for every group) or (B,3,4), any device -> (B,3,4) float32 host array; ValueError
    for another shape, a non-finite entry, or a row that is not rigid: |R^T R - I| <= RIGID_TOL and det R > 0"""
    if cam_T_rig is None:
        raise ValueError("TEST.VIEWS > 1: load() needs cam_T_rig, ({0},3,4) or ({1},3,4): p_cam = [R | t] p_rig per view".format(V, B))
    x = torch.as_tensor(cam_T_rig).detach().cpu().numpy().astype(np.float32)
    if x.shape not in ((V, 3, 4), (B, 3, 4)):
        raise ValueError("cam_T_rig must be ({},3,4) or ({},3,4), got {}".format(V, B, x.shape))
    if x.shape[0] != B:
        x = np.tile(x, (B // V, 1, 1))
    for b, row in enumerate(x.astype(np.float64)):
        R = row[:, :3]
        if not np.all(np.isfinite(row)) or np.abs(R.T @ R - np.eye(3)).max() > RIGID_TOL or not np.linalg.det(R) > 0:
            raise ValueError("cam_T_rig[{}] is not a rigid transform (|R^T R - I| <= {}, det R > 0): {}".format(b, RIGID_TOL, row.tolist()))
    return np.ascontiguousarray(x)


def check_one_rig(x, V):
    """TEST.VIEWS_CALIB_ITER > 0: the (B,3,4) host array check_cam_T_rig returned must repeat the V rows of one rig for every group,
    bit for bit (one correction per camera is sought); ValueError names the first row that does not"""
    x = np.ascontiguousarray(x, np.float32)
    for b in range(V, len(x)):
        if not np.array_equal(x[b].view(np.uint32), x[b % V].view(np.uint32)):
            raise ValueError("TEST.VIEWS_CALIB_ITER > 0: cam_T_rig[{}] differs from cam_T_rig[{}]: the groups of a batch must repeat one rig "
                             "of {} cameras".format(b, b % V, V))
    return x


class ViewsConsensus(object):
    """the step between the loop and the post-loop stages: the render of every sample's last pose and its score, as the selection among
    hypotheses takes them, then dim_views_consensus -> score (B,), choice (G,), pose_rig (G,3,4), pose_views (B,3,4) and status (B,) =
    the loop's last status row, the render's and the score's bits and DIM_STATUS_VIEWS_NO_CONSENSUS.  cam_T_rig (B,3,4) is resident:
    a captured graph reads what the latest load() put there.  cam_T_rig_used is what the joint stages read: cam_T_rig itself, or the
    calibration stage's output when that is on."""

    def __init__(self, r, H, W, V, mode, tau):
        B, d = r.B, r.net.device
        z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=d)  # noqa: E731
        self.V, self.G, self.mode, self.tau = V, B // V, mode, tau
        self.cam_T_rig = torch.eye(3, 4, dtype=F32, device=d).repeat(B, 1, 1).contiguous()
        self.cam_T_rig_used = self.cam_T_rig
        self.image, self.depth, self.bbox = z(F32, B, 3, H, W), z(F32, B, 1, H, W), z(I32, B, 4)
        self.work = ops.pose_score_workspace(B, H, W, d)
        self.score, self.choice, self.status = z(F32, B), z(I32, self.G), z(I32, B)
        self.pose_rig, self.pose_views = z(F32, self.G, 3, 4), z(F32, B, 3, 4)

    def run(self, r, pose):
        ops.copy(self.status, r.status_iter[r.test_iter - 1])
        r._render_at(pose, self.status, image=self.image, depth=self.depth, bbox=self.bbox, plane_means=r.net.plane_means)
        ops.pose_score(r.batch["image_observed"], self.image, self.depth, self.mode, self.tau,
                       depth_observed=r.depth_observed if self.mode == "depth" else None, bbox=self.bbox, score=self.score,
                       status=self.status, workspace=self.work)
        ops.views_consensus(self.score, pose, self.cam_T_rig, self.V, status=self.status, fatal_mask=FATAL_MASK, choice=self.choice,
                            pose_rig=self.pose_rig, pose_views=self.pose_views, status_out=self.status)


class ViewsCalib(object):
    """the step between the consensus and the post-loop stages (TEST.VIEWS_CALIB_ITER > 0): render depth and box at the consensus'
    per-sample poses, then dim_icp_refine_rig against the refiner's depth_observed -> cam_T_rig (B,3,4) = the calibrated rig repeated
    for every group (cam_T_rig_calib: its first V rows; camera 0's row is the loaded one), pose_rig (G,3,4), pose (B,3,4) =
    float32(X'_v pose_rig) (pose_step: the entry's own per-sample output), stats (B,n,2), stats_group (G,n,2), stats_view (V,n,2),
    status (B,) (render bits, DIM_STATUS_ICP_FEW_POINTS, DIM_STATUS_VIEWS_CALIB_HELD).  The loaded cam_T_rig is never written."""

    def __init__(self, r, H, W, settings):
        (self.iters, self.max_dist), B, V, d = settings, r.B, r.V, r.net.device
        z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=d)  # noqa: E731
        G, n = B // V, self.iters
        self.depth, self.bbox = z(F32, B, 1, H, W), z(I32, B, 4)
        self.pose, self.pose_step, self.pose_rig, self.cam_T_rig = z(F32, B, 3, 4), z(F32, B, 3, 4), z(F32, G, 3, 4), z(F32, B, 3, 4)
        self.cam_T_rig_calib = self.cam_T_rig[:V]
        self.stats, self.stats_group, self.stats_view, self.status = z(F32, B, n, 2), z(F32, G, n, 2), z(F32, V, n, 2), z(I32, B)
        self.work = ops.icp_rig_workspace(B, H, W, V, d)
        r.views.cam_T_rig_used = self.cam_T_rig

    def run(self, r, pose, pose_rig):
        ops.fill(self.status, 0)
        K_pair = r._render_at(pose, self.status, depth=self.depth, bbox=self.bbox)
        ops.icp_refine_rig(self.depth, r.depth_observed, pose, r.render_machine.K, self.iters, self.max_dist, r.views.cam_T_rig, r.V,
                           pose_rig, bbox=self.bbox, K_per_sample=K_pair, pose_out=self.pose_step, pose_rig_out=self.pose_rig,
                           cam_T_rig_out=self.cam_T_rig, stats=self.stats, stats_group=self.stats_group, stats_view=self.stats_view,
                           status=self.status, workspace=self.work)
        ops.views_from_rig(self.pose_rig, self.cam_T_rig, r.V, pose_views=self.pose)
