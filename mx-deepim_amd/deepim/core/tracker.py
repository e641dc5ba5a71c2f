"""Following objects through a video, device resident: the temporal layer around deepim.core.tester.Refiner.

P tracks share one camera.  Per frame one chain runs on one stream, with no host round trip:

    ingest (dim_track_ingest: the frame -> the P observed blobs)  ->  predict (dim_track_predict: the last two accepted poses ->
    refiner.pose_init)  ->  the start render and its box mask, as Refiner.load renders a starting pose  ->  Refiner._loop()  ->
    [render of the tracked poses]  ->  [dim_track_visibility]  ->  [dim_pose_score against the frame]  ->  update (dim_track_update
    or dim_track_update_occ: step ring, lost test, history, re-initialisation)

With TEST.TRACK_SEG "color" every frame is segmented from what the earlier frames showed: dim_track_seg_mask writes a mask per track
from the box of the start render and the track's foreground / background colour histograms before the loop runs (into
refiner.mask_sil when the silhouette stage is on: the stage then runs inside the chain and TRACK_POSE may be "sil"), and
dim_track_seg_learn updates the histograms after the update from the render of the tracked pose, skipping a track that was lost,
re-initialised or occluded on this frame (tests/track_seg_reference.py restates both).  learn_colors() gives the tracks a model
before the first frame.

The render runs when a score or TEST.TRACK_OCCLUSION is on.  With occlusion on, the tracks are judged together instead of each alone:
dim_track_visibility says which pixels of a track another track, or the frame's own depth, hides, the score is taken over the
visible pixels only (depth_visible in place of depth_sc), and the update is dim_track_update_occ, which lets a track of which too
little is visible coast on the motion model for a while instead of losing it (tests/track_occ_reference.py restates both).

With capture_graph the chain is one hipGraph, captured at the first step and replayed for every later frame.  The state (pose
history, age, step ring) lives in device tensors the chain reads and writes in place; a step copies the frame (and the offered
re-initialisation poses) into resident staging tensors and launches the chain.  tests/track_reference.py restates predict and update.
"""
from __future__ import print_function, division

import numpy as np
import torch

from lib.hip import ops
from deepim.core.pose_stages import int_setting, stages_on
from deepim.core.tester import Refiner, capture_graph
from deepim.core.views import refuse_with_views
from deepim.symbols.deepIM_flownet import source_size

TRACK_MOTIONS = ("hold", "velocity")
TRACK_SCORES = ("none", "rgb", "depth")
TRACK_POSES = ("loop", "icp", "photo", "sil")
TRACK_OCCLUSIONS = ("none", "tracks", "depth", "both")
TRACK_SEGS = ("none", "color")
# status bits that end a track's frame: nothing to zoom on (the object left the image or the render is empty), a class or camera
# the rasteriser refused.  The stages' own "too few points" bits are not fatal: their pose is then the loop's, unchanged
FATAL_MASK = 1 | 2 | ops.STATUS_BAD_CLASS | ops.STATUS_BAD_K   # DIM_STATUS_OBS_BOX_EMPTY | DIM_STATUS_REN_BOX_EMPTY | ...
# flags of a frame the colour model does not learn from: the pose is not one to trust, or too little of the object is seen
SEG_SKIP_MASK = FATAL_MASK | ops.STATUS_TRACK_LOST | ops.STATUS_TRACK_REINIT | ops.STATUS_TRACK_OCCLUDED


def _finite(T, key, what, ok, default=None):
    v = T.get(key, default)
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = np.nan
    if isinstance(v, bool) or not (np.isfinite(f) and ok(f)):
        raise ValueError("TEST.{} must be {}, got {!r}".format(key, what, v))
    return f


def occlusion_settings(cfg):
    """-> dict(mode, delta, min_visible, max_occluded) of cfg.TEST.TRACK_OCCLUSION, TRACK_OCC_DELTA, TRACK_MIN_VISIBLE and
    TRACK_MAX_OCCLUDED, checked; ValueError names the bad key"""
    T = cfg.TEST
    mode = T.get("TRACK_OCCLUSION")
    if mode not in TRACK_OCCLUSIONS:
        raise ValueError("TEST.TRACK_OCCLUSION must be one of {}, got {!r}".format(TRACK_OCCLUSIONS, mode))
    delta = _finite(T, "TRACK_OCC_DELTA", "a finite distance >= 0 (metres)", lambda f: f >= 0)
    min_visible = _finite(T, "TRACK_MIN_VISIBLE", "a number in [0, 1]", lambda f: 0.0 <= f <= 1.0)
    max_occluded = int_setting("TRACK_MAX_OCCLUDED", T.get("TRACK_MAX_OCCLUDED"), 0, 2 ** 31 - 1, "an integer >= 0")
    return dict(mode=mode, delta=delta, min_visible=min_visible, max_occluded=max_occluded)


def segmentation_settings(cfg):
    """-> dict(mode, bits, margin, radius, rate, min_pixels) of cfg.TEST.TRACK_SEG, TRACK_SEG_BITS, TRACK_SEG_MARGIN, TRACK_SEG_SMOOTH,
    TRACK_SEG_RATE and TRACK_SEG_MIN_PIXELS, checked; ValueError names the bad key.  With "color" a silhouette stage that is on must
    read the tracker's mask (SIL_MASK "observed") and the margin must reach the stage's gate: the region's border is an edge of the
    mask, and one nearer than ceil(SIL_MAX_PX) to the object would pull on its contour"""
    T = cfg.TEST
    mode = T.get("TRACK_SEG", "none")   # a configuration from before the keys existed: off, with the defaults
    if mode not in TRACK_SEGS:
        raise ValueError("TEST.TRACK_SEG must be one of {}, got {!r}".format(TRACK_SEGS, mode))
    bits = int_setting("TRACK_SEG_BITS", T.get("TRACK_SEG_BITS", 5), 1, 5, "an integer in 1..5")
    margin = int_setting("TRACK_SEG_MARGIN", T.get("TRACK_SEG_MARGIN", 16), 0, 2 ** 20, "an integer >= 0 (pixels)")
    radius = int_setting("TRACK_SEG_SMOOTH", T.get("TRACK_SEG_SMOOTH", 2), 0, 4, "an integer in 0..4 (pixels)")
    rate = _finite(T, "TRACK_SEG_RATE", "a number in [0, 1]", lambda f: 0.0 <= f <= 1.0, default=0.1)
    min_pixels = int_setting("TRACK_SEG_MIN_PIXELS", T.get("TRACK_SEG_MIN_PIXELS", 64), 1, 2 ** 31 - 1, "an integer >= 1")
    if mode == "color" and "sil" in stages_on(cfg):
        if T.get("SIL_MASK", "observed") != "observed":
            raise ValueError("TEST.SIL_MASK must be 'observed' in a Tracker with TEST.TRACK_SEG 'color' (the tracker writes the stage's "
                             "mask; the fast loop has no mask head), got {!r}".format(T.get("SIL_MASK")))
        gate = int(np.ceil(float(T.get("SIL_MAX_PX", 12.0))))
        if margin < gate:
            raise ValueError("TEST.TRACK_SEG_MARGIN = {} must be >= ceil(TEST.SIL_MAX_PX) = {}: the region's border would grow edges "
                             "inside the silhouette stage's gate".format(margin, gate))
    return dict(mode=mode, bits=bits, margin=margin, radius=radius, rate=rate, min_pixels=min_pixels)


def track_settings(cfg):
    """-> dict(motion, damping, window, lost_rot_deg, lost_trans, score, min_score, depth_tau, pose) of cfg.TEST.TRACK_*, checked;
    ValueError names the bad key.  The occlusion keys are checked here as well; their values come from occlusion_settings"""
    T = cfg.TEST
    motion = T.get("TRACK_MOTION")
    if motion not in TRACK_MOTIONS:
        raise ValueError("TEST.TRACK_MOTION must be one of {}, got {!r}".format(TRACK_MOTIONS, motion))
    damping = _finite(T, "TRACK_DAMPING", "a number in [0, 1]", lambda f: 0.0 <= f <= 1.0)
    window = int_setting("TRACK_WINDOW", T.get("TRACK_WINDOW"), 1, ops.TRACK_MAX_WINDOW, "an integer in 1..{}".format(ops.TRACK_MAX_WINDOW))
    rot = _finite(T, "TRACK_LOST_ROT_DEG", "a finite angle > 0 (degrees)", lambda f: f > 0)
    trans = _finite(T, "TRACK_LOST_TRANS", "a finite distance > 0 (metres)", lambda f: f > 0)
    score = T.get("TRACK_SCORE")
    if score not in TRACK_SCORES:
        raise ValueError("TEST.TRACK_SCORE must be one of {}, got {!r}".format(TRACK_SCORES, score))
    min_score = _finite(T, "TRACK_MIN_SCORE", "a finite number", lambda f: True)
    tau = _finite(T, "TRACK_DEPTH_TAU", "a finite distance > 0 (metres)", lambda f: f > 0)
    pose = T.get("TRACK_POSE")
    if pose not in TRACK_POSES:
        raise ValueError("TEST.TRACK_POSE must be one of {}, got {!r}".format(TRACK_POSES, pose))
    if pose != "loop" and pose not in stages_on(cfg):
        raise ValueError("TEST.TRACK_POSE {!r} needs its stage switched on (TEST.{}_ITER > 0)".format(pose, pose.upper()))
    occlusion_settings(cfg)
    return dict(motion=motion, damping=damping, window=window, lost_rot_deg=rot, lost_trans=trans, score=score, min_score=min_score,
                depth_tau=tau, pose=pose)


def refuse_for_tracking(cfg, lit=False):
    """what a Tracker cannot be combined with; every ValueError names its key.  Reads the configuration only: no device work"""
    T, stages = cfg.TEST, stages_on(cfg)
    refuse_with_views(cfg, "the Tracker (a track is one object in one camera)")
    if int(T.get("HYP_NUM", 1) or 1) > 1:
        raise ValueError("Tracker: TEST.HYP_NUM > 1 is not supported (a track has one pose per frame)")
    if int(T.get("COARSE_VIEWS", 0) or 0) > 0:
        raise ValueError("Tracker: TEST.COARSE_VIEWS > 0 is not supported (the starting pose of a frame comes from the track)")
    if lit:
        raise ValueError("Tracker: the lit ModelNet renderer is not supported (render machine with normals)")
    if "sil" in stages and T.get("TRACK_SEG", "none") != "color":
        raise ValueError("Tracker: TEST.SIL_ITER > 0 is not supported (a frame carries no segmentation)")
    if "flow_pnp" in stages:
        raise ValueError("Tracker: TEST.FLOW_PNP_ITER > 0 is not supported")
    if T.INIT_MASK != "box_rendered":
        raise ValueError("Tracker: TEST.INIT_MASK must be 'box_rendered' (the mask of a frame is the box of its start render), got {!r}".format(
            T.INIT_MASK))


class Tracker(object):
    """num_tracks = P objects followed through the frames of one camera.  reset() gives every track its class and first pose(s);
    step() takes one frame and returns device views of the frame's outputs; run() takes a sequence and reads everything back once."""

    def __init__(self, config, predictor, render_machine, num_tracks, capture_graph=True):
        cfg = config
        self.settings = s = track_settings(cfg)
        self.occlusion = occ = occlusion_settings(cfg)
        self.occ_on = occ["mode"] != "none"
        self.segmentation = seg = segmentation_settings(cfg)
        self.seg_on = seg["mode"] == "color"
        occ_depth = occ["mode"] in ("depth", "both")
        refuse_for_tracking(cfg, lit=hasattr(render_machine, "normals"))
        self.cfg, self.P = cfg, int(num_tracks)
        self.refiner = r = Refiner(cfg, predictor, render_machine, self.P, capture_graph=False)
        P, T, d = self.P, r.test_iter, r.net.device
        H, W = source_size(cfg)
        self.H, self.W, self.device = H, W, d
        self.depth_factor = float(cfg.dataset.DEPTH_FACTOR)
        self.pixel_means = np.asarray(cfg.network.PIXEL_MEANS, dtype=np.float32).reshape(3)
        self.znear, self.zfar = float(cfg.dataset.ZNEAR), float(cfg.dataset.ZFAR)
        # the observed depth plane of the frame: the refiner's where a stage or an INPUT_DEPTH graph reads one, else the score's own
        self.depth_observed = r.depth_observed if r.depth_observed is not None else r.batch.get("depth_observed")
        if self.depth_observed is None and (s["score"] == "depth" or occ_depth):
            self.depth_observed = torch.zeros((P, 1, H, W), dtype=torch.float32, device=d)
        self.needs_depth = self.depth_observed is not None
        zeros = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=d)  # noqa: E731
        f32, i32 = torch.float32, torch.int32
        # state
        self.hist, self.age = zeros(f32, P, 2, 3, 4), zeros(i32, P)
        self.ring, self.ring_n, self.ring_pos = zeros(f32, P, s["window"], 2), zeros(i32, P), zeros(i32, P)
        # (occlusion) occ_age: the frames a track has coasted in a row; occluder_ok: 0 for a track that was lost on the last frame and
        # not re-initialised -- its pose is stale, it hides nobody on the next one
        self.occ_age, self.occluder_ok = zeros(i32, P), torch.ones((P,), dtype=i32, device=d)
        # staging: what a step copies in before the chain runs
        self.frame_raw = zeros(torch.uint8, H, W, 3)
        # (torch has no uint16 fill or copy kernels: the plane is made and copied as int16, the same bytes)
        self.depth_raw = zeros(torch.int16, H, W).view(torch.uint16) if self.needs_depth else None
        self.reinit_pose, self.reinit_valid = zeros(f32, P, 3, 4), zeros(i32, P)
        # the start render's box; status rows of a frame: the loop's iterations, the start render, the tracked pose's stage and score
        self.bbox_start = zeros(i32, P, 4)
        self.status_rows = zeros(i32, T + 2, P)
        self.pose_before = r.poses_iter[T - 2] if T > 1 else r.pose_init
        self.pose_new = {"loop": r.poses_iter[T - 1], "icp": r.pose_icp, "photo": r.pose_photo, "sil": r.pose_sil}[s["pose"]]
        self.score = None
        if s["score"] != "none" or self.occ_on:   # the render of the tracked pose
            self.image_sc, self.depth_sc, self.bbox_sc = zeros(f32, P, 3, H, W), zeros(f32, P, 1, H, W), zeros(i32, P, 4)
        elif self.seg_on:   # the segmentation alone: depth and box suffice
            self.image_sc, self.depth_sc, self.bbox_sc = None, zeros(f32, P, 1, H, W), zeros(i32, P, 4)
        if s["score"] != "none":
            self.score_work = ops.pose_score_workspace(P, H, W, d)
            self.score = zeros(f32, P)
        self.flags, self.step_out, self.mean_out = zeros(i32, P), zeros(f32, P, 2), zeros(f32, P, 2)
        self.visible = self.counts = self.pose_track = None
        if self.occ_on:
            self.depth_visible, self.vis_work = zeros(f32, P, 1, H, W), ops.track_visibility_workspace(P, H, W, d)
            self.visible, self.counts, self.pose_track = zeros(f32, P), zeros(i32, P, 4), zeros(f32, P, 3, 4)
        # (segmentation) the colour model -- state --, the frame's mask (the silhouette stage's own when it is on) and pixel counts
        self.seg_hist = self.seg_age = self.mask = self.seg_counts = self.seg_learn_counts = None
        if self.seg_on:
            self.seg_hist, self.seg_age = zeros(f32, P, 2, 1 << (3 * seg["bits"])), zeros(i32, P)
            self.mask = r.mask_sil if "sil" in r.stages else zeros(f32, P, 1, H, W)
            self.seg_counts, self.seg_learn_counts = zeros(i32, P, 2), zeros(i32, P, 2)
            self.seg_work = ops.track_seg_workspace(P, H, W, seg["bits"], d)
        self.graph = None
        self._want_graph = bool(capture_graph)

    # ------------------------------------------------------------------------------------------
    def reset(self, class_index, pose, pose_prev=None):
        """start (again) from `pose` (P,3,4), the pose of the frame before the first one step() gets; with pose_prev, the pose one
        frame earlier, the first prediction already has a velocity (age 2, else 1).  The step ring is emptied, and so is the colour
        model of TEST.TRACK_SEG (learn_colors() fills it again)"""
        P = self.P
        self.refiner.batch["class_index"].copy_(torch.as_tensor(class_index).reshape(P).to(torch.int32))
        pose = torch.as_tensor(pose, dtype=torch.float32).reshape(P, 3, 4)
        self.hist[:, 1].copy_(pose)
        self.hist[:, 0].copy_(pose if pose_prev is None else torch.as_tensor(pose_prev, dtype=torch.float32).reshape(P, 3, 4))
        self.age.fill_(1 if pose_prev is None else 2)
        self.ring.zero_()
        self.ring_n.zero_()
        self.ring_pos.zero_()
        self.occ_age.zero_()
        self.occluder_ok.fill_(1)
        if self.seg_on:
            self.seg_hist.zero_()
            self.seg_age.zero_()

    def _state(self):
        state = (self.hist, self.age, self.ring, self.ring_n, self.ring_pos, self.occ_age, self.occluder_ok)
        return state + ((self.seg_hist, self.seg_age) if self.seg_on else ())

    def learn_colors(self, frame_bgr, pose=None):
        """one update of the colour model from `frame_bgr` (uint8 (H,W,3)) with the tracks at `pose` (P,3,4; default: the last accepted
        poses, after reset() the pose it was given), eagerly, outside the graph: with it the first frame is already segmented.
        -> (P,2) int32 device tensor {foreground, background pixels}; a track with too few of either keeps what it had"""
        if not self.seg_on:
            raise ValueError("Tracker.learn_colors: TEST.TRACK_SEG is 'none'")
        seg, r = self.segmentation, self.refiner
        frame_bgr = torch.as_tensor(frame_bgr)
        if tuple(frame_bgr.shape) != (self.H, self.W, 3) or frame_bgr.dtype != torch.uint8:
            raise ValueError("Tracker.learn_colors: frame_bgr must be uint8 ({},{},3), got {} {}".format(self.H, self.W, frame_bgr.dtype,
                                                                                                     tuple(frame_bgr.shape)))
        frame = frame_bgr.to(self.device).contiguous()
        pose = self.hist[:, 1] if pose is None else torch.as_tensor(pose, dtype=torch.float32).reshape(self.P, 3, 4).to(self.device)
        r.render_machine.render_batch(r.batch["class_index"], pose.contiguous(), depth=self.depth_sc, bbox=self.bbox_sc, mask_thr=0.0)
        return ops.track_seg_learn(frame, self.depth_sc, self.bbox_sc, self.seg_hist, self.seg_age, seg["bits"], seg["margin"], seg["rate"],
                                   seg["min_pixels"], workspace=self.seg_work)

    def _chain(self):
        """one frame, everything enqueued on the current stream from the resident tensors"""
        r, s, occ, T = self.refiner, self.settings, self.occlusion, self.refiner.test_iter
        b, init = r.batch, r.init
        ops.track_ingest(self.frame_raw, self.depth_factor, self.pixel_means, b["image_observed"], depth_raw=self.depth_raw,
                         depth_observed=self.depth_observed)
        ops.track_predict(self.hist, self.age, s["motion"], s["damping"], out=r.pose_init)
        r._render_start(bbox=self.bbox_start, status=self.status_rows[T])
        ops.box_mask(self.bbox_start, init["mask_observed"])
        seg = self.segmentation
        if self.seg_on:   # the frame's mask from the colour model, where the silhouette stage of the loop below reads it
            ops.track_seg_mask(self.frame_raw, self.bbox_start, self.seg_hist, self.seg_age, seg["bits"], seg["margin"], seg["radius"],
                               mask=self.mask, counts=self.seg_counts, status=self.status_rows[T], workspace=self.seg_work)
        r._loop()
        ops.copy(self.status_rows[:T], r.status_iter)
        last = self.status_rows[T + 1]
        if s["pose"] == "loop":
            ops.fill(last, 0)
        else:
            ops.copy(last, r.stages[s["pose"]].status)
        if self.score is not None or self.occ_on:   # the render of the tracked poses
            r.render_machine.render_batch(b["class_index"], self.pose_new, image=self.image_sc, depth=self.depth_sc, bbox=self.bbox_sc,
                                          plane_means=r.net.plane_means, mask_thr=0.0, status=last)
        elif self.seg_on:   # ... for the colour model alone
            r.render_machine.render_batch(b["class_index"], self.pose_new, depth=self.depth_sc, bbox=self.bbox_sc, mask_thr=0.0, status=last)
        if self.occ_on:   # which of its pixels are visible (every row of depth_observed is the frame's depth after the ingest)
            ops.track_visibility(self.depth_sc, occ["mode"], occ["delta"], depth_frame=self.depth_observed[0, 0] if occ["mode"] != "tracks" else None,
                                 occluder_ok=self.occluder_ok, depth_visible=self.depth_visible, counts=self.counts, workspace=self.vis_work)
        if self.score is not None:   # as Refiner._select scores a hypothesis: every drawn (with occlusion: and visible) pixel inside its box
            ops.pose_score(b["image_observed"], self.image_sc, self.depth_visible if self.occ_on else self.depth_sc, s["score"], s["depth_tau"],
                           depth_observed=self.depth_observed if s["score"] == "depth" else None, bbox=self.bbox_sc, score=self.score,
                           status=last, workspace=self.score_work)
        update, occ_in, occ_out = ops.track_update, (), {}
        if self.occ_on:   # the update with the occluded state
            update, occ_in = ops.track_update_occ, (self.occ_age, self.counts, occ["min_visible"], occ["max_occluded"], r.pose_init)
            occ_out = dict(visible=self.visible, pose_track=self.pose_track, occluder_ok=self.occluder_ok)
        update(self.pose_before, self.pose_new, self.hist, self.age, self.ring, self.ring_n, self.ring_pos, *occ_in, s["lost_rot_deg"],
               s["lost_trans"], self.znear, self.zfar, status_rows=self.status_rows, fatal_mask=FATAL_MASK, score=self.score,
               min_score=s["min_score"], reinit_pose=self.reinit_pose, reinit_valid=self.reinit_valid, flags=self.flags,
               step=self.step_out, mean=self.mean_out, **occ_out)
        if self.seg_on:   # the colour model learns from the accepted frames only
            ops.track_seg_learn(self.frame_raw, self.depth_sc, self.bbox_sc, self.seg_hist, self.seg_age, seg["bits"], seg["margin"],
                                seg["rate"], seg["min_pixels"], depth_fg=self.depth_visible if self.occ_on else None, flags=self.flags,
                                skip_mask=SEG_SKIP_MASK, counts=self.seg_learn_counts, workspace=self.seg_work)

    def _stage_inputs(self, frame_bgr, depth_raw, reinit_pose, reinit_valid):
        P = self.P
        frame_bgr = torch.as_tensor(frame_bgr)
        if tuple(frame_bgr.shape) != (self.H, self.W, 3) or frame_bgr.dtype != torch.uint8:
            raise ValueError("Tracker.step: frame_bgr must be uint8 ({},{},3), got {} {}".format(self.H, self.W, frame_bgr.dtype,
                                                                                             tuple(frame_bgr.shape)))
        self.frame_raw.copy_(frame_bgr, non_blocking=True)
        if self.needs_depth:
            if depth_raw is None:
                raise ValueError("Tracker.step: the configuration (INPUT_DEPTH, TEST.ICP_ITER > 0, TEST.TRACK_SCORE 'depth' or "
                                 "TEST.TRACK_OCCLUSION 'depth' / 'both') needs depth_raw")
            if isinstance(depth_raw, np.ndarray):
                depth_raw = torch.from_numpy(np.ascontiguousarray(depth_raw, dtype=np.uint16))
            if tuple(depth_raw.shape) != (self.H, self.W) or depth_raw.dtype != torch.uint16:
                raise ValueError("Tracker.step: depth_raw must be uint16 ({},{}), got {} {}".format(self.H, self.W, depth_raw.dtype,
                                                                                                tuple(depth_raw.shape)))
            self.depth_raw.view(torch.int16).copy_(depth_raw.contiguous().view(torch.int16), non_blocking=True)
        if reinit_pose is None:
            if reinit_valid is not None:
                raise ValueError("Tracker.step: reinit_valid without reinit_pose")
            self.reinit_valid.zero_()
            return
        self.reinit_pose.copy_(torch.as_tensor(reinit_pose, dtype=torch.float32).reshape(P, 3, 4), non_blocking=True)
        if reinit_valid is None:
            self.reinit_valid.fill_(1)
        else:
            self.reinit_valid.copy_(torch.as_tensor(reinit_valid).reshape(P).to(torch.int32), non_blocking=True)

    def step(self, frame_bgr, depth_raw=None, reinit_pose=None, reinit_valid=None):
        """one frame: uint8 BGR (H,W,3) [, uint16 depth (H,W) in 1 / dataset.DEPTH_FACTOR metres], any device.  reinit_pose (P,3,4):
        a pose offered to every track that is lost on this frame (reinit_valid (P,): to which of them; all when omitted).
        -> dict of device views, valid until the next step: pose (P,3,4) the tracked pose of the frame, flags (P,) int32 (the frame's
        status bits, DIM_STATUS_TRACK_LOST / _REINIT among them), step (P,2) the loop's last step (degrees, metres), mean (P,2) its
        window means, score (P,) or None; with TEST.TRACK_OCCLUSION on also visible (P,) the visible fraction of each track's render,
        counts (P,4) int32 its pixels {drawn, visible, hidden by a track, hidden by the frame's depth only} and pose_track (P,3,4)
        the best current estimate (the accepted pose, the coasted prediction of an occluded track -- DIM_STATUS_TRACK_OCCLUDED in
        flags --, the offered pose, or the last accepted pose of a lost track), else None for the three.  The predicted pose the loop
        started from stays in refiner.pose_init.  With TEST.TRACK_SEG "color" also mask (P,1,H,W) the frame's segmentation of 0 / 1
        (written before the loop), seg_counts (P,2) int32 {region pixels, mask pixels} and seg_age (P,) int32 the updates of each
        track's colour model after this frame (the three keys are absent when it is off: out.get("mask") is None); with the silhouette
        stage on, its pose is refiner.pose_sil"""
        self._stage_inputs(frame_bgr, depth_raw, reinit_pose, reinit_valid)
        if self._want_graph and self.graph is None:
            # the warm-up is a real frame: the state it advanced is put back before the captured chain runs for the first time
            self.graph = capture_graph(self._chain, self.device, self._state())
        if self.graph is not None:
            self.graph.replay()
        else:
            self._chain()
        out = {"pose": self.pose_new, "flags": self.flags, "step": self.step_out, "mean": self.mean_out, "score": self.score,
               "visible": self.visible, "counts": self.counts, "pose_track": self.pose_track}
        if self.seg_on:   # (absent, not None, when off: the dict of a tracker without a segmentation is the one it always was)
            out.update(mask=self.mask, seg_counts=self.seg_counts, seg_age=self.seg_age)
        return out

    def run(self, frames):
        """frames: an iterable of dicts with frame_bgr [, depth_raw, reinit_pose, reinit_valid] (the arguments of step).  Every
        frame's outputs are recorded on the device and read back once at the end -> dict of host arrays (T,P,...): pose, flags, step,
        mean [, score] [, visible, counts, pose_track] [, mask, seg_counts, seg_age]"""
        rec = {}
        for f in frames:
            out = self.step(f["frame_bgr"], f.get("depth_raw"), f.get("reinit_pose"), f.get("reinit_valid"))
            for k, v in out.items():
                if v is not None:
                    rec.setdefault(k, []).append(v.clone())
        return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}
