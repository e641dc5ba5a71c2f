"""The test-time pose stages of deepim.core.tester.Refiner: depth ICP, photometric polish and silhouette polish after the refinement
loop, each from its last pose, and pose from flow at every iteration of it; STAGE_KEY: stage -> the TEST key that switches it on (> 0).
A stage is one class, built only when it is on: its checked settings, its private buffers, its outputs, its run.
With TEST.VIEWS = V > 1 (deepim.core.views) a post-loop stage runs its joint entry: run() also takes the rig poses of the G = B / V
groups, and the stage leaves pose_rig (G,3,4) and stats_group next to its per-sample outputs; the extrinsics it reads are the
consensus' cam_T_rig_used: the loaded ones, or the calibrated ones with TEST.VIEWS_CALIB_ITER > 0."""
import numpy as np
import torch

from lib.hip import ops

STAGE_KEY = {"icp": "ICP_ITER", "flow_pnp": "FLOW_PNP_ITER", "photo": "PHOTO_ITER", "sil": "SIL_ITER"}
F32, I32 = torch.float32, torch.int32
_OFF = {"HYP_NUM": 1, "COARSE_VIEWS": 0}   # the value up to which a feature a stage cannot be combined with is off


def stages_on(cfg):
    """-> the names of the stages cfg.TEST switches on, in the order of STAGE_KEY: the one place that reads the raw keys for it"""
    return tuple(name for name, key in STAGE_KEY.items() if int(cfg.TEST.get(key, 0) or 0) > 0)


def int_setting(key, v, lo, hi, what):
    """v as an int in lo..hi (hi None: unbounded); ValueError "TEST.<key> must be <what>, got <v>" """
    if isinstance(v, bool) or not float(v).is_integer() or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError("TEST.{} must be {}, got {!r}".format(key, what, v))
    return int(v)


def _huber_gate(T, huber_key, huber_default, huber_what, gate_key, gate_default, gate_what, gate_max=np.inf):
    """-> (Huber knee, hard gate) of cfg.TEST: the knee finite and > 0, the gate finite and in knee..gate_max"""
    huber, gate = float(T.get(huber_key, huber_default)), float(T.get(gate_key, gate_default))
    if not (np.isfinite(huber) and huber > 0):
        raise ValueError("TEST.{} must be {}, got {!r}".format(huber_key, huber_what, T.get(huber_key)))
    if not (np.isfinite(gate) and huber <= gate <= gate_max):
        raise ValueError("TEST.{} must be {}, got {!r}".format(gate_key, gate_what, T.get(gate_key)))
    return huber, gate


def _refuse_with(T, key, *others):
    for other in others:
        if int(T.get(other, _OFF[other]) or _OFF[other]) > _OFF[other]:
            raise ValueError("TEST.{} > 0 cannot be combined with TEST.{} > {}".format(key, other, _OFF[other]))


def icp_settings(cfg):
    """-> (ICP_ITER, ICP_MAX_DIST) of cfg.TEST (0 iterations = off; the gate in metres)"""
    return int(cfg.TEST.get("ICP_ITER", 0) or 0), float(cfg.TEST.get("ICP_MAX_DIST", 0.02))


def flow_pnp_settings(cfg):
    """-> (FLOW_PNP_ITER, FLOW_PNP_WARM, FLOW_PNP_HUBER_PX, FLOW_PNP_MAX_PX) of cfg.TEST, checked; ValueError names the bad key(s).
    The stage reads the flow head's output of every loop iteration, so it needs PRED_FLOW and the full (not FAST_TEST) graph; choosing
    among per-hypothesis flow poses is not defined, so it is refused together with HYP_NUM > 1."""
    T = cfg.TEST
    n = int_setting("FLOW_PNP_ITER", T.get("FLOW_PNP_ITER", 0) or 0, 0, None, "an integer >= 0 (0 = off)")
    warm = int_setting("FLOW_PNP_WARM", T.get("FLOW_PNP_WARM", 2), 0, None, "an integer >= 0")
    huber, gate = _huber_gate(T, "FLOW_PNP_HUBER_PX", 2.0, "a finite number of pixels > 0",
                              "FLOW_PNP_MAX_PX", 8.0, "finite and >= TEST.FLOW_PNP_HUBER_PX")
    if n > 0:
        if not cfg.network.PRED_FLOW:
            raise ValueError("TEST.FLOW_PNP_ITER > 0 needs network.PRED_FLOW (the stage reads the flow head's output)")
        if T.FAST_TEST:
            raise ValueError("TEST.FLOW_PNP_ITER > 0 needs TEST.FAST_TEST off (the fast graph has no flow head)")
        _refuse_with(T, "FLOW_PNP_ITER", "HYP_NUM")
    return n, warm, huber, gate


def photo_settings(cfg):
    """-> (PHOTO_ITER, PHOTO_LEVELS, PHOTO_HUBER, PHOTO_MAX, PHOTO_GAIN) of cfg.TEST, checked; ValueError names the bad key(s).
    PHOTO_ITER counts Gauss-Newton iterations per pyramid level (0 = off); the two thresholds are in units of the channel sum.
    Selecting among polished hypotheses is not defined, so the stage is refused together with HYP_NUM > 1 and COARSE_VIEWS > 0."""
    T = cfg.TEST
    n = int_setting("PHOTO_ITER", T.get("PHOTO_ITER", 0) or 0, 0, None, "an integer >= 0 (iterations per level, 0 = off)")
    levels = int_setting("PHOTO_LEVELS", T.get("PHOTO_LEVELS", 3), 1, 5, "an integer in 1..5")
    huber, gate = _huber_gate(T, "PHOTO_HUBER", 30.0, "a finite number > 0 (units of the channel sum)",
                              "PHOTO_MAX", 180.0, "finite and >= TEST.PHOTO_HUBER")
    gain = T.get("PHOTO_GAIN", True)
    if not isinstance(gain, (bool, np.bool_)):
        raise ValueError("TEST.PHOTO_GAIN must be True or False, got {!r}".format(gain))
    if n > 0:
        _refuse_with(T, "PHOTO_ITER", "HYP_NUM", "COARSE_VIEWS")
    return n, levels, huber, gate, bool(gain)


def sil_settings(cfg):
    """-> (SIL_ITER, SIL_ROUNDS, SIL_HUBER_PX, SIL_MAX_PX, SIL_MASK) of cfg.TEST, checked; ValueError names the bad key(s).
    SIL_ITER counts Gauss-Newton iterations per round (0 = off); the two thresholds are in pixels, and the edge field reaches
    ceil(SIL_MAX_PX) <= 64 pixels.  Selecting among polished hypotheses is not defined, so the stage is refused together with
    HYP_NUM > 1 and COARSE_VIEWS > 0; SIL_MASK 'pred' needs the mask head's output, which only the full graph computes."""
    T = cfg.TEST
    n = int_setting("SIL_ITER", T.get("SIL_ITER", 0) or 0, 0, None, "an integer >= 0 (iterations per round, 0 = off)")
    rounds = int_setting("SIL_ROUNDS", T.get("SIL_ROUNDS", 2), 1, 8, "an integer in 1..8")
    huber, gate = _huber_gate(T, "SIL_HUBER_PX", 2.0, "a finite number > 0 (pixels)",
                              "SIL_MAX_PX", 12.0, "finite, >= TEST.SIL_HUBER_PX and <= 64 (pixels)", gate_max=64)
    which = T.get("SIL_MASK", "observed")
    if which not in ("observed", "pred"):
        raise ValueError("TEST.SIL_MASK must be 'observed' or 'pred', got {!r}".format(which))
    if n > 0:
        _refuse_with(T, "SIL_ITER", "HYP_NUM", "COARSE_VIEWS")
        if which == "pred" and not (cfg.network.PRED_MASK and not T.FAST_TEST):
            raise ValueError("TEST.SIL_ITER > 0 with TEST.SIL_MASK 'pred' needs the mask head of the full graph "
                             "(network.PRED_MASK, TEST.FAST_TEST off)")
    return n, rounds, huber, gate, str(which)


def stage_settings(cfg, lit=False):
    """-> {stage: its checked settings} for all four, on or off (entry 0: its iterations, 0 = off); lit: the lit ModelNet renderer"""
    s = {"flow_pnp": flow_pnp_settings(cfg)}
    for name, settings in (("photo", photo_settings), ("sil", sil_settings)):
        s[name] = settings(cfg)
        if s[name][0] > 0 and lit:
            raise ValueError("TEST.{} > 0 is not supported with the lit ModelNet renderer".format(STAGE_KEY[name]))
    return dict(s, icp=icp_settings(cfg))


def _zeros(r, dtype, *shape):
    return torch.zeros(shape, dtype=dtype, device=r.net.device)


def _views_outputs(stage, r, n_iters):
    """the joint outputs of a post-loop stage: pose_rig (G,3,4), stats_group (G,n_iters,2) and pose_step (B,3,4), the entry's own
    per-sample output; None with one view per group.  The stage's public pose is then X_b pose_rig (_publish)"""
    V = getattr(r, "V", 1)
    G = r.B // V
    stage.pose_rig, stage.stats_group, stage.pose_step = (
        _zeros(r, F32, G, 3, 4), _zeros(r, F32, G, n_iters, 2), _zeros(r, F32, r.B, 3, 4)) if V > 1 else (None, None, None)
    return V


def _publish(stage, r):
    """a joint stage's per-sample poses are its rig pose seen from every camera, rounded once: the views of a group then agree with
    the extrinsics to that one rounding.  (The entry's own pose_out, kept in pose_step, is the same pose up to the float32 rounding
    of the per-sample pose it started from.)"""
    ops.views_from_rig(stage.pose_rig, r.views.cam_T_rig_used, r.V, pose_views=stage.pose)


class IcpStage(object):
    """depth ICP from the loop's last pose: render its depth and box (the pair's K when loaded), then dim_icp_refine against the
    refiner's depth_observed -> pose (B,3,4), stats (B,ICP_ITER,2), status (B,) (render bits and DIM_STATUS_ICP_FEW_POINTS)"""

    def __init__(self, r, H, W, settings):
        (self.iters, self.max_dist), B = settings, r.B
        self.depth, self.bbox = _zeros(r, F32, B, 1, H, W), _zeros(r, I32, B, 4)
        self.pose, self.stats, self.status = _zeros(r, F32, B, 3, 4), _zeros(r, F32, B, self.iters, 2), _zeros(r, I32, B)
        V = _views_outputs(self, r, self.iters)
        self.work = ops.icp_workspace(B, H, W, r.net.device) if V == 1 else ops.icp_views_workspace(B, H, W, V, r.net.device)

    def run(self, r, pose, pose_rig=None):
        ops.fill(self.status, 0)
        K_pair = r._render_at(pose, self.status, depth=self.depth, bbox=self.bbox)
        if pose_rig is not None:
            ops.icp_refine_views(self.depth, r.depth_observed, pose, r.render_machine.K, self.iters, self.max_dist, r.views.cam_T_rig_used, r.V,
                                 pose_rig, bbox=self.bbox, K_per_sample=K_pair, pose_out=self.pose_step, pose_rig_out=self.pose_rig,
                                 stats=self.stats, stats_group=self.stats_group, status=self.status, workspace=self.work)
            return _publish(self, r)
        ops.icp_refine(self.depth, r.depth_observed, pose, r.render_machine.K, self.iters, self.max_dist, bbox=self.bbox,
                       K_per_sample=K_pair, pose_out=self.pose, stats=self.stats, status=self.status, workspace=self.work)


class PhotoStage(object):
    """photometric polish from the loop's last pose: render its image, depth and box (the pair's K when loaded), then dim_photo_refine
    against image_observed -> pose (B,3,4), stats (B,PHOTO_LEVELS*PHOTO_ITER,2), status (B,) (render bits, DIM_STATUS_PHOTO_FEW_POINTS)"""

    def __init__(self, r, H, W, settings):
        (self.iters, self.levels, self.huber, self.gate, self.gain), B = settings, r.B
        self.image, self.depth, self.bbox = _zeros(r, F32, B, 3, H, W), _zeros(r, F32, B, 1, H, W), _zeros(r, I32, B, 4)
        self.pose, self.stats, self.status = _zeros(r, F32, B, 3, 4), _zeros(r, F32, B, self.levels * self.iters, 2), _zeros(r, I32, B)
        V = _views_outputs(self, r, self.levels * self.iters)
        self.work = (ops.photo_workspace(B, H, W, self.levels, r.net.device) if V == 1 else
                     ops.photo_views_workspace(B, H, W, self.levels, V, r.net.device))

    def run(self, r, pose, pose_rig=None):
        ops.fill(self.status, 0)
        K_pair = r._render_at(pose, self.status, image=self.image, depth=self.depth, bbox=self.bbox, plane_means=r.net.plane_means)
        if pose_rig is not None:
            ops.photo_refine_views(r.batch["image_observed"], self.image, self.depth, pose, r.render_machine.K, self.levels, self.iters,
                                   self.huber, self.gate, r.views.cam_T_rig_used, r.V, pose_rig, gain=self.gain, bbox=self.bbox,
                                   K_per_sample=K_pair, pose_out=self.pose_step, pose_rig_out=self.pose_rig, stats=self.stats,
                                   stats_group=self.stats_group, status=self.status, workspace=self.work)
            return _publish(self, r)
        ops.photo_refine(r.batch["image_observed"], self.image, self.depth, pose, r.render_machine.K, self.levels, self.iters, self.huber,
                         self.gate, gain=self.gain, bbox=self.bbox, K_per_sample=K_pair, pose_out=self.pose, stats=self.stats,
                         status=self.status, workspace=self.work)


class SilStage(object):
    """silhouette polish from the loop's last pose: the edge field of the stage's mask once (radius ceil(SIL_MAX_PX)), then SIL_ROUNDS rounds,
    each rendering depth and box at the current pose and running dim_sil_refine from it -> pose, the last row of pose_round, stats
    (B,SIL_ROUNDS*SIL_ITER,2), status (B,).  mask: load()'s copy of the segmentation (SIL_MASK 'observed'; 'pred' reads the mask head's)"""

    def __init__(self, r, H, W, settings):
        (self.iters, self.rounds, self.huber, self.gate, self.which), B = settings, r.B
        if self.which == "pred" and r.mask_pred_iter is None:
            raise ValueError("TEST.SIL_ITER > 0 with TEST.SIL_MASK 'pred': the network has no mask head (network.PRED_MASK with a "
                             "decoder, TEST.FAST_TEST off)")
        self.mask = _zeros(r, F32, B, 1, H, W) if self.which == "observed" else None
        self.radius = int(np.ceil(self.gate))
        self.field, self.depth, self.bbox = _zeros(r, I32, B, H, W), _zeros(r, F32, B, 1, H, W), _zeros(r, I32, B, 4)
        self.pose_round, self.status = _zeros(r, F32, self.rounds, B, 3, 4), _zeros(r, I32, B)
        self.pose = self.pose_round[self.rounds - 1]
        self.stats_round, self.stats = _zeros(r, F32, B, self.iters, 2), _zeros(r, F32, B, self.rounds * self.iters, 2)
        V = _views_outputs(self, r, self.rounds * self.iters)
        self.work = ops.sil_workspace(B, H, W, r.net.device) if V == 1 else ops.sil_views_workspace(B, H, W, V, r.net.device)
        if V > 1:   # a round's rig pose and group stats, as pose_round and stats_round
            self.pose_rig_round, self.stats_group_round = _zeros(r, F32, self.rounds, B // V, 3, 4), _zeros(r, F32, B // V, self.iters, 2)
            self.pose_rig, self.pose = self.pose_rig_round[self.rounds - 1], self.pose_step   # (pose_round: the entry's own outputs)

    def _run_views(self, r, pose, pose_rig):
        """run() for groups of views: every round starts from the previous round's per-sample poses and rig pose"""
        n, G = 2 * self.iters, r.B // r.V
        flat, flat_group = self.stats.view(-1), self.stats_group.view(-1)
        for k in range(self.rounds):
            K_pair = r._render_at(pose, self.status, depth=self.depth, bbox=self.bbox)
            ops.sil_refine_views(self.depth, self.field, pose, r.render_machine.K, self.iters, self.huber, self.gate, r.views.cam_T_rig_used, r.V,
                                 pose_rig, bbox=self.bbox, K_per_sample=K_pair, pose_out=self.pose_round[k],
                                 pose_rig_out=self.pose_rig_round[k], stats=self.stats_round, stats_group=self.stats_group_round,
                                 status=self.status, workspace=self.work)
            ops.copy_rows(flat[k * n:], self.rounds * n, self.stats_round, n, r.B, n)
            ops.copy_rows(flat_group[k * n:], self.rounds * n, self.stats_group_round, n, G, n)
            pose, pose_rig = self.pose_round[k], self.pose_rig_round[k]
        _publish(self, r)

    def run(self, r, pose, pose_rig=None):
        ops.fill(self.status, 0)
        ops.sil_edge_field(self.mask if self.which == "observed" else r.mask_pred_iter[r.test_iter - 1], self.radius, field=self.field)
        if pose_rig is not None:
            return self._run_views(r, pose, pose_rig)
        n, flat = 2 * self.iters, self.stats.view(-1)   # n: floats per pair and round
        for k in range(self.rounds):
            K_pair = r._render_at(pose, self.status, depth=self.depth, bbox=self.bbox)
            ops.sil_refine(self.depth, self.field, pose, r.render_machine.K, self.iters, self.huber, self.gate, bbox=self.bbox,
                           K_per_sample=K_pair, pose_out=self.pose_round[k], stats=self.stats_round, status=self.status,
                           workspace=self.work)
            ops.copy_rows(flat[k * n:], self.rounds * n, self.stats_round, n, r.B, n)
            pose = self.pose_round[k]


class FlowPnpStage(object):
    """pose from the flow head's output at every loop iteration (dim_flow_pnp), recorded only: pose_iter (test_iter,B,3,4), se3_iter
    (test_iter,B,7), stats (test_iter,B,FLOW_PNP_ITER,2), status (test_iter,B).  depth: of the render each forward looked at (the loop's
    re-render writes it), bbox: of the initial render; both None in an INPUT_DEPTH graph, which holds the plane already"""

    def __init__(self, r, H, W, settings):
        (self.iters, self.warm, self.huber, self.gate), B, T = settings, r.B, r.test_iter
        if r.flow_est_iter is None:
            raise ValueError("TEST.FLOW_PNP_ITER > 0: the network has no flow head (network.PRED_FLOW with a decoder)")
        self.depth, self.bbox = (None, None) if r.input_depth else (_zeros(r, F32, B, 1, H, W), _zeros(r, I32, B, 4))
        self.pose_iter, self.se3_iter = _zeros(r, F32, T, B, 3, 4), _zeros(r, F32, T, B, 7)
        self.stats, self.status = _zeros(r, F32, T, B, self.iters, 2), _zeros(r, I32, T, B)
        self.work = ops.flow_pnp_workspace(B, H, W, r.net.device)

    def start(self, r, pose):
        """the first forward looks at the loaded render: its depth and box once more (INPUT_DEPTH: the plane is a blob, the box unknown)"""
        ops.fill(self.status, 0)
        if not r.input_depth:
            r._render_at(pose, self.status[0], depth=self.depth, bbox=self.bbox)

    def step(self, r, it, cur, pose, bbox_ren):
        """flow2se3 on what forward `it` saw: the render's depth and box, the flow it predicted, mask_observed as it read it"""
        ops.flow_pnp(cur["depth_rendered"] if r.input_depth else self.depth, r.flow_est_iter[it], pose, r.render_machine.K, self.iters,
                     self.warm, self.huber, self.gate, standard_rep=bool(r.cfg.network.STANDARD_FLOW_REP), valid=cur["mask_observed"],
                     bbox=bbox_ren if it > 0 else (None if r.input_depth else self.bbox),
                     K_per_sample=r.K_pair if (r.per_pair_K and not r.lit) else None, pose_out=self.pose_iter[it],
                     se3_q=self.se3_iter[it], stats=self.stats[it], status=self.status[it], workspace=self.work)


STAGES = (("icp", IcpStage), ("photo", PhotoStage), ("sil", SilStage), ("flow_pnp", FlowPnpStage))   # in the order the Refiner builds them
POST_LOOP = ("icp", "photo", "sil")   # the stages that run after the loop, in this order
