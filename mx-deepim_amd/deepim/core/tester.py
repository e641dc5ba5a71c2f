"""Test-time iterative refinement, device resident.

Mirror of /root/reference/deepim/core/tester.py: `Predictor` (:27-56) and the refinement loop of
`pred_eval` (:418-642).  The reference runs batch 1 per GPU and, per iteration, syncs the 7 floats to
the host, composes the pose in numpy (:525-532), renders with OpenGL + glReadPixels (:563-568),
rebuilds the blobs on the host (data_pair.update_data_batch) and uploads them (:590).  Here a batch of
pairs stays in HBM for all iterations:

    forward (zoom -> encoder -> heads)  ->  se3_compose  ->  rasterise (image_rendered, mask_rendered,
    bbox)  ->  box mask (mask_observed, UPDATE_MASK == "box_rendered")  ->  forward ...

and the whole loop can be captured into one hipGraph (`Refiner(capture_graph=True)`).  The blobs, the renders and the masks have the
size of the camera image, config.SCALES[0] (any 4:3 size, K the camera of that image); the network input stays 480x640.
"""
from __future__ import print_function, division
from collections import namedtuple

import numpy as np
import torch

from lib.hip import ops
from deepim.core.coarse import CoarseInit, boxes_from_int, coarse_settings
from deepim.core.pose_stages import (POST_LOOP, STAGE_KEY, STAGES, flow_pnp_settings, icp_settings, int_setting, photo_settings,  # noqa: F401
                                     sil_settings, stage_settings, stages_on)
from deepim.core.score_lists import PairLists, ScoreLists
from deepim.core.views import (ViewsCalib, ViewsConsensus, calib_settings, check_cam_T_rig, check_one_rig, refuse_views_at_source_size,
                               refuse_with_views, views_settings)
from deepim.symbols.deepIM_flownet import FlowNetHip, source_size, zoom_filter

HYP_SCORES = ("rgb", "depth")
ERR_KEYS = ("re", "te", "add", "arp_2d")   # the per-pose error lists lib.dataset.evaluation.PoseEvaluator takes as `errors=`
VSD_KEYS = ("vsd", "visib_gt", "union", "inter", "drawn_gt")   # per pose: the errors (one per tau) and dim_vsd_errors' four counts
BOP_KEYS = ("mssd", "mspd", "sym_mssd", "sym_mspd")             # per pose: dim_bop_errors' two errors and the symmetries that attain them
GRID_KEYS = ("vsd_grid",) + VSD_KEYS[1:]                       # per pose: dim_vsd_grid_errors' errors (one per tau of the class) and counts
RT_KEYS = ("rot_err", "trans_err", "poses_est", "poses_gt")    # per pose: the four lists of the reference's pred_eval (and of its result cache)
# the families of per-pose lists pred_eval keeps for a pose set, in the order their columns are packed for the host
FAMILY_KEYS = {"rt": RT_KEYS, "err": ERR_KEYS, "vsd": VSD_KEYS, "grid": GRID_KEYS, "bop": BOP_KEYS}
HYP_KEYS = ("score", "choice", "rot_err", "trans_err", "undetected")   # per pair with several hypotheses
COARSE_KEYS = ("idx", "score", "status", "pose")                       # per pair: the kept candidates of the coarse stage, best first
# the one-row pose sets of pred_eval, in the order of their tables.  pose: its attribute on the refiner; full: every family scores it, from
# _read_out's rows -- else the error code alone, from a copy of its own, and TEST.VSD / TEST.BOP refuse its `word` row; keys: (key, default)
OneRowSet = namedtuple("OneRowSet", "name pose full word headline keys")
ONE_ROW_SETS = (
    OneRowSet("icp", "pose_icp", True, None, "evaluate ICP ({} iterations, gate {} m):", (("ICP_ITER", 0), ("ICP_MAX_DIST", 0.02))),
    OneRowSet("photo", "pose_photo", False, "photometric", "evaluate photometric polish ({} levels x {} iterations, Huber {}, gate {}):",
     (("PHOTO_LEVELS", 3), ("PHOTO_ITER", 0), ("PHOTO_HUBER", 30.0), ("PHOTO_MAX", 180.0))),
    OneRowSet("sil", "pose_sil", False, "silhouette", "evaluate silhouette polish ({} rounds x {} iterations, Huber {} px, gate {} px, mask {}):",
     (("SIL_ROUNDS", 2), ("SIL_ITER", 0), ("SIL_HUBER_PX", 2.0), ("SIL_MAX_PX", 12.0), ("SIL_MASK", "observed"))))


def hyp_settings(cfg):
    """-> (HYP_NUM, HYP_ROT_DEG, HYP_SCORE, HYP_DEPTH_TAU) of cfg.TEST, checked; ValueError names the bad key"""
    T = cfg.TEST
    n = int_setting("HYP_NUM", T.get("HYP_NUM", 1), 1, None, "an integer >= 1 (1 = one hypothesis per pair, off)")
    deg = float(T.get("HYP_ROT_DEG", 30.0))
    if not np.isfinite(deg):
        raise ValueError("TEST.HYP_ROT_DEG must be finite, got {!r}".format(T.get("HYP_ROT_DEG")))
    score = T.get("HYP_SCORE", "rgb")
    if score not in HYP_SCORES:
        raise ValueError("TEST.HYP_SCORE must be one of {}, got {!r}".format(HYP_SCORES, score))
    tau = float(T.get("HYP_DEPTH_TAU", 0.02))
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("TEST.HYP_DEPTH_TAU must be a finite distance > 0 (metres), got {!r}".format(T.get("HYP_DEPTH_TAU")))
    return n, deg, score, tau


def bop_vsd_settings(cfg):
    """-> (BOP_VSD, BOP_VSD_DELTA, BOP_VSD_TAU as a list of fractions) of cfg.TEST, checked; ValueError names the bad key.  The grid
    only completes the BOP table (AR needs AR_MSSD and AR_MSPD next to AR_VSD), so it needs TEST.BOP."""
    T = cfg.TEST
    if not bool(T.get("BOP_VSD", False)):
        return False, None, None
    if not bool(T.get("BOP", False)):
        raise ValueError("TEST.BOP_VSD needs TEST.BOP (AR averages AR_VSD with the AR_MSSD and AR_MSPD of TEST.BOP)")
    delta = float(T.BOP_VSD_DELTA)
    if not np.isfinite(delta):
        raise ValueError("TEST.BOP_VSD_DELTA must be finite (metres), got {!r}".format(T.BOP_VSD_DELTA))
    fracs = [float(f) for f in np.asarray(T.BOP_VSD_TAU, dtype=np.float64).reshape(-1)]
    if not 1 <= len(fracs) <= ops.VSD_GRID_MAX_TAU or not all(np.isfinite(f) and f > 0 for f in fracs):
        raise ValueError("TEST.BOP_VSD_TAU must hold 1 to {} finite fractions > 0 of the diameter, got {!r}".format(
            ops.VSD_GRID_MAX_TAU, T.BOP_VSD_TAU))
    return True, delta, fracs


def hypothesis_rotations(N, rot_deg):
    """(N,3,3) float64: R_0 = I; R_h (h >= 1) = the Rodrigues rotation by rot_deg about axis h-1 of a Fibonacci sphere of N-1 points,
    z = 1 - (2k+1)/(N-1), r = sqrt(1-z^2), phi = k pi (3 - sqrt 5), axis = (r cos phi, r sin phi, z).  Hypothesis h starts the
    loop from [R_h R_p | t_p]: the pair's pose turned about the object origin in the camera frame."""
    R = np.tile(np.eye(3), (N, 1, 1))
    M, th = N - 1, np.radians(rot_deg)
    for k in range(M):
        z = 1.0 - (2.0 * k + 1.0) / M
        r, phi = np.sqrt(max(0.0, 1.0 - z * z)), k * np.pi * (3.0 - np.sqrt(5.0))
        a = np.array([r * np.cos(phi), r * np.sin(phi), z])
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        R[k + 1] = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    return R


def refuse_at_source_size(cfg, size, lit=False):
    """the stages that exist at the network size only: with SCALES of another size every one that is switched on raises a ValueError
    naming its key and SCALES (none may run at the wrong size).  What runs at any 4:3 size: the FAST_TEST loop (UPDATE_MASK
    'box_rendered' / 'init', per-pair K, graph capture, the INPUT_DEPTH graphs), TEST.DEVICE_EVAL and TEST.BOP without BOP_VSD.
    TEST.VIEWS > 1 is refused like the stages it needs: a joint stage raises under its own key here, and the consensus, which is on
    whatever the stages are, under TEST.VIEWS (deepim.core.views.refuse_views_at_source_size)."""
    if tuple(size) == (FlowNetHip.H, FlowNetHip.W):
        return
    T, stages = cfg.TEST, stages_on(cfg)
    on = [("TEST.ICP_ITER", "icp" in stages), ("TEST.HYP_NUM", int(T.get("HYP_NUM", 1) or 1) > 1),
          ("TEST.COARSE_VIEWS", int(T.get("COARSE_VIEWS", 0) or 0) > 0), ("TEST.VSD", bool(T.get("VSD", False))),
          ("TEST.BOP_VSD", bool(T.get("BOP_VSD", False))), ("TEST.FLOW_PNP_ITER", "flow_pnp" in stages),
          ("TEST.PHOTO_ITER", "photo" in stages), ("TEST.SIL_ITER", "sil" in stages),
          ("network.PRED_FLOW without TEST.FAST_TEST (the test-time flow error)", bool(cfg.network.PRED_FLOW and not T.FAST_TEST)),
          ("the lit ModelNet renderer", bool(lit))]
    for key, active in on:
        if active:
            raise ValueError("{} is built for SCALES [[{}, {}]] only, got SCALES {}x{}: switch it off or shrink the images to the network "
                             "size".format(key, FlowNetHip.H, FlowNetHip.W, size[0], size[1]))


class Predictor(object):
    """Reference: binds a MutableModule and calls forward (tester.py:27-56).  Here: owns a FlowNetHip."""

    def __init__(self, config, arg_params, batch_size, device="cuda:0", conv_plan=None, winograd=True):
        name, max_taps = zoom_filter(config)
        self.net = FlowNetHip(config, arg_params, batch_size, device=device, conv_plan=conv_plan, winograd=winograd,
                              source_size=source_size(config), zoom_filter=name, zoom_area_max_taps=max_taps)
        self.data_names = ["image_observed", "image_rendered", "src_pose", "class_index", "mask_observed", "mask_rendered"]

    def predict(self, data_batch):
        """data_batch: dict blob-name -> CUDA tensor (names/shapes as deepim/core/loader.py:35-41).
        Returns [dict(se3_output, zoom_factor)] -- one entry, since one process drives one GPU."""
        return [self.net.forward_test(data_batch)]


def capture_graph(chain, device, state=()):
    """-> a torch.cuda.CUDAGraph of chain() (kernels only, one stream), after a warm-up run on a side stream (lazy module loads, attribute
    sets).  The warm-up is a real run: the `state` tensors that chain() advances in place are put back before the capture"""
    keep = [t.clone() for t in state]
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, k in zip(state, keep):
        t.copy_(k)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    return g


class Refiner(object):
    """batch_size = P pairs per loaded batch.  With TEST.HYP_NUM = N > 1 every pair is refined from N starting poses, as the samples
    b = p * N + h of one batch (the Predictor is built for P * N samples); after the loop each sample's last pose is rendered and
    scored against the observed image (TEST.HYP_SCORE) and the best hypothesis of each pair is selected, all inside the same graph.
    With TEST.COARSE_VIEWS > 0 the starting poses come from a detection box per pair: load(..., det_boxes=) runs the coarse stage
    (deepim.core.coarse.CoarseInit, eagerly, outside the graph) and starts the loop from its HYP_NUM best candidates.  evaluator: the
    PoseEvaluator whose model points the box fit projects (None: the vertices of the render machine's meshes).
    With TEST.VIEWS = V > 1 the batch holds batch_size / V objects seen by V calibrated cameras each (sample b = g * V + v,
    load(..., cam_T_rig=)): the loop runs per sample, then a consensus among the views of a group and the post-loop stages as joint
    stages with one correction per group (deepim.core.views).  With TEST.VIEWS_CALIB_ITER > 0 the rig's extrinsics are refined with
    the rig poses in between (camera 0 fixed); the stages use them, and cam_T_rig_calib (V,3,4), pose_calib, pose_rig_calib,
    calib_stats, calib_stats_group, calib_stats_view and status_calib exist (only then).  The loaded cam_T_rig is never overwritten; a
    caller who trusts the result passes cam_T_rig_calib to the next load()."""

    def __init__(self, config, predictor, render_machine, batch_size, capture_graph=False, evaluator=None):
        cfg = config
        if cfg.network.INPUT_MASK and cfg.network.PRED_MASK and cfg.TEST.UPDATE_MASK not in ("box_rendered", "init"):
            # same restriction as the released loop (tester.py:579-587)
            raise Exception("Unknown UPDATE_MASK type: {}".format(cfg.TEST.UPDATE_MASK))
        # (Hs, Ws): the size of every image-like buffer here -- the camera image, the renders, the masks; the network input stays 480x640
        H, W = source_size(cfg)
        filter_cfg = zoom_filter(cfg)   # (refuses 'area' in the full graph)
        refuse_at_source_size(cfg, (H, W), lit=hasattr(render_machine, "normals"))
        refuse_views_at_source_size(cfg, (H, W), (FlowNetHip.H, FlowNetHip.W))
        self.hyp_num, self.hyp_rot_deg, self.hyp_score_mode, self.hyp_tau = hyp_settings(cfg)
        self.V, views_score, views_tau = views_settings(cfg, lit=hasattr(render_machine, "normals"))
        if batch_size % self.V:
            raise ValueError("Refiner: batch_size {} is not a multiple of TEST.VIEWS {}".format(batch_size, self.V))
        calib = calib_settings(cfg)
        settings = stage_settings(cfg, lit=hasattr(render_machine, "normals"))   # every key checked, whether its stage is on or not
        self.icp_iter, self.photo_iter, self.sil_iter, self.flow_pnp_iter = (settings[k][0] for k in ("icp", "photo", "sil", "flow_pnp"))
        N = self.hyp_num
        if N > 1 and predictor.net.B != batch_size * N:
            raise ValueError("Refiner: {} pairs x TEST.HYP_NUM {} = {} samples, but the Predictor was built for {} samples".format(
                batch_size, N, batch_size * N, predictor.net.B))
        if N > 1 and hasattr(render_machine, "normals"):
            raise ValueError("TEST.HYP_NUM > 1 is not supported with the lit ModelNet renderer")
        if (predictor.net.Hs, predictor.net.Ws) != (H, W):
            raise ValueError("Refiner: SCALES is {}x{} but the Predictor's network was built for a {}x{} source".format(
                H, W, predictor.net.Hs, predictor.net.Ws))
        if filter_cfg != (predictor.net.zoom_filter, predictor.net.zoom_area_max_taps):
            raise ValueError("Refiner: TEST.ZOOM_FILTER / TEST.ZOOM_AREA_MAX_TAPS are {} but the Predictor's network was built for {}".format(
                filter_cfg, (predictor.net.zoom_filter, predictor.net.zoom_area_max_taps)))
        if (int(render_machine.height), int(render_machine.width)) != (H, W):
            raise ValueError("Refiner: SCALES is {}x{} but the render machine draws {}x{}".format(H, W, render_machine.height,
                                                                                                   render_machine.width))
        self.cfg = cfg
        self.predictor = predictor
        self.net = predictor.net
        self.render_machine = render_machine
        self.P, self.N = batch_size, N
        self.B = batch_size * N   # samples
        self.test_iter = int(cfg.TEST.test_iter)
        d = self.net.device
        B = self.B
        self.batch = {
            "image_observed": torch.zeros((B, 3, H, W), dtype=torch.float32, device=d),
            "image_rendered": torch.zeros((B, 3, H, W), dtype=torch.float32, device=d),
            "mask_observed": torch.zeros((B, 1, H, W), dtype=torch.float32, device=d),
            "mask_rendered": torch.zeros((B, 1, H, W), dtype=torch.float32, device=d),
            "src_pose": torch.zeros((B, 3, 4), dtype=torch.float32, device=d),
            "class_index": torch.zeros((B,), dtype=torch.int32, device=d),
        }
        self.input_depth = bool(cfg.network.INPUT_DEPTH)
        if self.input_depth:   # the two depth planes of get_convs (:33-50); the rendered one is refreshed by every re-render (tester.py:573-574)
            self.batch["depth_observed"] = torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
            self.batch["depth_rendered"] = torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
        # pristine copies of the blobs the loop overwrites, so refine() can be replayed on the same batch
        self.init = {k: torch.zeros_like(self.batch[k]) for k in ("image_rendered", "mask_observed", "mask_rendered")
                     + (("depth_rendered",) if self.input_depth else ())}
        self.pose_init = torch.zeros((B, 3, 4), dtype=torch.float32, device=d)
        self.poses_iter = torch.zeros((self.test_iter, B, 3, 4), dtype=torch.float32, device=d)
        self.se3_iter = torch.zeros((self.test_iter, B, 7), dtype=torch.float32, device=d)
        self.bbox = torch.zeros((B, 4), dtype=torch.int32, device=d)
        self.bbox2 = torch.zeros((B, 4), dtype=torch.int32, device=d)   # consecutive renders alternate: one box is the next render's dirty-box hint
        self.bbox_obs = torch.zeros((B, 4), dtype=torch.int32, device=d)
        self.status_iter = torch.zeros((self.test_iter, B), dtype=torch.int32, device=d)
        # TEST.ZOOM_FILTER 'area', for diagnostics: the sub-samples (n_x, n_y) every iteration's zoom took per pair (dim_zoom_area_taps)
        self.taps_iter = torch.ones((self.test_iter, B, 2), dtype=torch.int32, device=d) if self.net.zoom_filter == "area" else None
        # the camera of each pair's re-render (reference tester.py:165, :560-562: a pair's own -K.txt replaces the config K there, and
        # only there -- ZoomMask and the flow error keep the config K).  Resident so that a captured graph reads whatever load() put in
        # it; `per_pair_K` False (no K loaded) keeps the uniform render with the config K, the launches of a loop without the feature.
        self.K_pair = torch.from_numpy(np.tile(np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(1, 9), (B, 1))).to(d)
        self.per_pair_K = False
        # per-iteration head outputs of the full (not FAST_TEST) graph, read by the reference at tester.py:485-491
        self.with_heads = bool(self.net.has_decoder and not cfg.TEST.FAST_TEST)
        self.mask_pred_iter = self.flow_est_iter = None
        if self.with_heads and cfg.network.PRED_MASK:
            self.mask_pred_iter = torch.zeros((self.test_iter, B, 1, H, W), dtype=torch.float32, device=d)
        if self.with_heads and cfg.network.PRED_FLOW:
            self.flow_est_iter = torch.zeros((self.test_iter, B, 2, H, W), dtype=torch.float32, device=d)
        self.T_means = np.asarray(cfg.dataset.trans_means, dtype=np.float32)
        self.T_stds = np.asarray(cfg.dataset.trans_stds, dtype=np.float32)
        self.depth_observed = None   # read by the ICP stage and the depth hypothesis score (an INPUT_DEPTH graph holds it as a blob)
        if self.icp_iter > 0 or (N > 1 and self.hyp_score_mode == "depth") or (self.V > 1 and views_score == "depth") or calib[0] > 0:
            self.depth_observed = self.batch["depth_observed"] if self.input_depth else torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
        # groups of views (TEST.VIEWS > 1): the consensus after the loop and its outputs; the joint outputs of the stages below
        self.views = ViewsConsensus(self, H, W, self.V, views_score, views_tau) if self.V > 1 else None
        vc = self.views
        self.views_score, self.views_choice, self.pose_rig, self.pose_views, self.status_views = (
            vc.score, vc.choice, vc.pose_rig, vc.pose_views, vc.status) if vc else (None,) * 5
        # the rig's extrinsics refined with the rig poses (TEST.VIEWS_CALIB_ITER > 0): built before the stages, which read its extrinsics.
        # Its outputs exist only when it is on
        self.calib = ViewsCalib(self, H, W, calib) if calib[0] > 0 else None
        if self.calib is not None:
            c = self.calib
            self.cam_T_rig_calib, self.pose_calib, self.pose_rig_calib, self.status_calib = c.cam_T_rig_calib, c.pose, c.pose_rig, c.status
            self.calib_stats, self.calib_stats_group, self.calib_stats_view = c.stats, c.stats_group, c.stats_view
        # the pose stages that are on, each with its own buffers, and their outputs under the Refiner's public names: None when off
        self.stages = {name: cls(self, H, W, settings[name]) for name, cls in STAGES if settings[name][0] > 0}
        icp, photo, sil, flow = (self.stages.get(k) for k in ("icp", "photo", "sil", "flow_pnp"))
        self.pose_icp, self.icp_stats, self.status_icp = (icp.pose, icp.stats, icp.status) if icp else (None, None, None)
        self.pose_photo, self.photo_stats, self.status_photo = (photo.pose, photo.stats, photo.status) if photo else (None, None, None)
        self.pose_sil, self.sil_stats, self.status_sil = (sil.pose, sil.stats, sil.status) if sil else (None, None, None)
        self.pose_rig_icp, self.icp_stats_group = (icp.pose_rig, icp.stats_group) if icp else (None, None)
        self.pose_rig_photo, self.photo_stats_group = (photo.pose_rig, photo.stats_group) if photo else (None, None)
        self.pose_rig_sil, self.sil_stats_group = (sil.pose_rig, sil.stats_group) if sil else (None, None)
        self.pose_flow_iter, self.se3_flow_iter, self.flow_pnp_stats, self.status_flow = (
            flow.pose_iter, flow.se3_iter, flow.stats, flow.status) if flow else (None, None, None, None)
        if sil and sil.mask is not None:   # SIL_MASK 'observed': load() fills it
            self.mask_sil = sil.mask
        # several hypotheses per pair (TEST.HYP_NUM > 1): the loaded pairs land in `pair` (P rows) and are expanded into the B = P*N
        # sample rows by load(); after the loop: the render at the last pose, the scores, the choice and the selected outputs
        self.pair = self.hyp_score = self.hyp_choice = self.poses_sel = self.status_sel = self.pose_icp_sel = None
        if N > 1:
            P = batch_size
            plane = lambda c: torch.zeros((P, c, H, W), dtype=torch.float32, device=d)  # noqa: E731
            self.pair = {"image_observed": plane(3), "image_rendered": plane(3), "mask_observed": plane(1), "mask_rendered": plane(1),
                         "src_pose": torch.zeros((P, 3, 4), dtype=torch.float32, device=d),
                         "class_index": torch.zeros((P,), dtype=torch.int32, device=d),
                         "K": torch.zeros((P, 9), dtype=torch.float32, device=d)}
            if self.depth_observed is not None or self.input_depth:
                self.pair["depth_observed"] = plane(1)
            if self.input_depth:
                self.pair["depth_rendered"] = plane(1)
            self.hyp_table = torch.from_numpy(hypothesis_rotations(N, self.hyp_rot_deg).astype(np.float32).reshape(N, 9)).to(d)
            self.bbox_hyp = torch.zeros((B, 4), dtype=torch.int32, device=d)
            self.status_hyp = torch.zeros((B,), dtype=torch.int32, device=d)   # render bits of the load-time hypothesis renders
            self.image_sc = torch.zeros((B, 3, H, W), dtype=torch.float32, device=d)
            self.depth_sc = torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
            self.bbox_sc = torch.zeros((B, 4), dtype=torch.int32, device=d)
            self.score_work = ops.pose_score_workspace(B, H, W, d)
            self.hyp_score = torch.zeros((B,), dtype=torch.float32, device=d)
            self.hyp_choice = torch.zeros((P,), dtype=torch.int32, device=d)
            self.poses_sel = torch.zeros((self.test_iter, P, 3, 4), dtype=torch.float32, device=d)
            self.status_sel = torch.zeros((self.test_iter, P), dtype=torch.int32, device=d)
            if self.icp_iter > 0:
                self.pose_icp_sel = torch.zeros((P, 3, 4), dtype=torch.float32, device=d)
        render_machine.reserve(B)
        # starting poses from detection boxes (TEST.COARSE_VIEWS > 0): the coarse stage, its outputs of the latest load, and for one
        # hypothesis per pair the box and the status of the initial render (several: _expand's bbox_hyp / status_hyp)
        self.coarse = self.coarse_out = None
        if coarse_settings(cfg)[0] > 0:
            self.coarse = CoarseInit(cfg, render_machine, evaluator, batch_size, N)   # (refuses the lit renderer)
            if N == 1:
                self.bbox_hyp = torch.zeros((B, 4), dtype=torch.int32, device=d)
                self.status_hyp = torch.zeros((B,), dtype=torch.int32, device=d)
        # ModelNet: the lit renderer takes a per-render light intensity drawn on the host (tester.py:227-230)
        self.lit = hasattr(render_machine, "normals")
        self.light_int = torch.ones((max(self.test_iter - 1, 1), B, 3), dtype=torch.float32, device=d) if self.lit else None
        self.graph = None
        self._graph_per_pair_K = None   # which render the captured graph holds (a different one is captured again)
        self._want_graph = capture_graph

    # ------------------------------------------------------------------------------------------
    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None, hyp_poses=None, det_boxes=None, cam_T_rig=None):
        """copy one batch of blobs (any device) into the resident buffers (the depth planes: INPUT_DEPTH graphs only; depth_observed
        also when TEST.ICP_ITER > 0 or the depth hypothesis score is on).
        K: None (every re-render uses the config K) or the camera of each pair, (B,3,3) or (B,9), any device: the unlit re-renders of
        this batch use it (the lit ModelNet render ignores K, as the reference's render() closure does)
        hyp_poses: TEST.HYP_NUM > 1 only: None (hypothesis 0 = the loaded pair, the others generated from it) or (P,N,3,4) starting
        poses given by the caller, all of them rendered
        det_boxes: TEST.COARSE_VIEWS > 0 only, and required then: (P,4) detection boxes {x0,x1,y0,y1}, continuous pixel extents (the
        inclusive int box {min_x,max_x,min_y,max_y} is {min_x-0.5, max_x+0.5, min_y-0.5, max_y+0.5}).  The coarse stage finds the
        starting poses; src_pose, image_rendered and mask_rendered (and depth_rendered) are ignored and may be None
        cam_T_rig: TEST.VIEWS > 1 only, and required then: (V,3,4) (one rig for every group) or (B,3,4), any device, the rigid
        [R | t] with p_cam = [R | t] p_rig of every view; each row is checked (|R^T R - I| <= 1e-4, det R > 0)"""
        if self.coarse is not None:
            return self._load_coarse(image_observed, mask_observed, class_index, depth_observed, K, hyp_poses, det_boxes)
        if det_boxes is not None:
            raise ValueError("det_boxes needs TEST.COARSE_VIEWS > 0")
        if self.views is not None:
            rig = check_cam_T_rig(cam_T_rig, self.B, self.V)
            self.views.cam_T_rig.copy_(torch.from_numpy(check_one_rig(rig, self.V) if self.calib is not None else rig))
        elif cam_T_rig is not None:
            raise ValueError("cam_T_rig needs TEST.VIEWS > 1")
        self._check_hyp_poses(hyp_poses)
        if "sil" in self.stages and self.stages["sil"].which == "observed":
            # taken from the caller's segmentation itself, before any INIT_MASK kind replaces the loop's mask by a box
            if mask_observed is None:
                raise ValueError("TEST.SIL_ITER > 0 with TEST.SIL_MASK 'observed': load() needs mask_observed, the segmentation whose "
                                 "edge the contour is pulled onto")
            self.mask_sil.copy_(torch.as_tensor(mask_observed).reshape(self.mask_sil.shape))
        self._load_K(K)
        b = self.batch
        dst = self._load_targets()
        if self.input_depth:
            assert depth_observed is not None and depth_rendered is not None, "INPUT_DEPTH: the loop needs depth_observed / depth_rendered"
            dst["depth_observed"].copy_(torch.as_tensor(depth_observed))
            dst["depth_rendered"].copy_(torch.as_tensor(depth_rendered))
        elif self.depth_observed is not None:
            if depth_observed is None:
                raise ValueError("TEST.ICP_ITER > 0: the ICP stage needs depth_observed" if self.icp_iter > 0 else
                                 "TEST.VIEWS_CALIB_ITER > 0: the calibration stage needs depth_observed" if self.calib is not None else
                                 "TEST.HYP_SCORE 'depth': the hypothesis score needs depth_observed")
            dst["depth_observed"].copy_(torch.as_tensor(depth_observed))
        dst["image_observed"].copy_(torch.as_tensor(image_observed))
        dst["image_rendered"].copy_(torch.as_tensor(image_rendered))
        dst["mask_observed"].copy_(torch.as_tensor(mask_observed))
        dst["mask_rendered"].copy_(torch.as_tensor(mask_rendered))
        dst["src_pose"].copy_(torch.as_tensor(src_pose))
        dst["class_index"].copy_(torch.as_tensor(class_index).to(torch.int32))
        if self.N > 1:
            self._expand(hyp_poses)
        if self.lit and self.test_iter > 1:
            # same draws, same order as the reference: sample by sample, one np.random.uniform(0.9,1.1,3) per re-render
            li = np.stack([[np.random.uniform(0.9, 1.1, size=(3,)) for _ in range(self.test_iter - 1)] for _ in range(self.B)])
            self.light_int.copy_(torch.from_numpy(li.transpose(1, 0, 2).astype(np.float32)))

    def _load_coarse(self, image_observed, mask_observed, class_index, depth_observed, K, hyp_poses, det_boxes):
        """load() with TEST.COARSE_VIEWS > 0: the observed blobs, then the coarse stage on them (eagerly, as _expand runs), whose
        HYP_NUM best candidates per pair become the starting poses, rendered by the render call of _expand.  One hypothesis per
        pair: the best candidate is pose_init, and mask_observed the box of its render under INIT_MASK 'box_rendered'."""
        if det_boxes is None:
            raise ValueError("TEST.COARSE_VIEWS > 0: load() needs det_boxes (P,4), the detection box of every pair")
        if hyp_poses is not None:
            raise ValueError("TEST.COARSE_VIEWS > 0: the starting poses come from det_boxes, hyp_poses must be None")
        self._load_K(K)
        dst = self._load_targets()
        if "depth_observed" in dst:
            if depth_observed is None:
                raise ValueError("the loop's configuration (INPUT_DEPTH, TEST.ICP_ITER > 0 or TEST.HYP_SCORE 'depth') needs depth_observed")
            dst["depth_observed"].copy_(torch.as_tensor(depth_observed))
        dst["image_observed"].copy_(torch.as_tensor(image_observed))
        dst["class_index"].copy_(torch.as_tensor(class_index).to(torch.int32))
        box_init = self.cfg.TEST.INIT_MASK == "box_rendered"
        mask_dst = dst["mask_observed"]
        if not box_init:
            if mask_observed is None:
                raise ValueError("TEST.INIT_MASK {!r}: load() needs mask_observed".format(self.cfg.TEST.INIT_MASK))
            mask_dst.copy_(torch.as_tensor(mask_observed))
        K_pair = (self.K_pair if self.N == 1 else self.pair["K"]) if self.per_pair_K else None
        poses, idx, score, status = self.coarse.run(dst["image_observed"], det_boxes, dst["class_index"],
                                                    depth_observed=dst.get("depth_observed", depth_observed), K=K_pair)
        self.coarse_out = {"pose": poses, "idx": idx, "score": score, "status": status}
        if self.N > 1:
            ops.copy(self.pair["src_pose"], poses[:, 0].contiguous())
            self._expand(poses)
            return
        ops.copy(self.pose_init, poses.reshape(self.B, 3, 4))
        self._render_start()
        if box_init:
            ops.box_mask(self.bbox_hyp, mask_dst)

    def _render_start(self, *, bbox=None, status=None):
        """the starting poses (pose_init) rendered as the loop re-renders: init image_rendered / mask_rendered [/ depth_rendered],
        their boxes in bbox_hyp and the render's status bits in status_hyp (or in the caller's bbox (B,4) / status (B,): the
        Tracker of deepim/core/tracker.py renders every frame's predicted poses with it)"""
        b, init = self.batch, self.init
        bbox = self.bbox_hyp if bbox is None else bbox
        status = self.status_hyp if status is None else status
        extra = {}
        if self.per_pair_K:
            extra["K"] = self.K_pair
        if self.input_depth:
            extra["depth"] = init["depth_rendered"]
        ops.fill(status, 0)
        self.render_machine.render_batch(b["class_index"], self.pose_init, image=init["image_rendered"], mask=init["mask_rendered"],
                                         bbox=bbox, plane_means=self.net.plane_means, mask_thr=0.2, status=status, **extra)

    def _load_K(self, K):
        if K is None:
            self.per_pair_K = False
            return
        K = torch.as_tensor(K)
        if tuple(K.shape) not in ((self.P, 3, 3), (self.P, 9)):
            raise ValueError("per-pair K must be ({0},3,3) or ({0},9), got {1}".format(self.P, tuple(K.shape)))
        (self.K_pair if self.N == 1 else self.pair["K"]).copy_(K.reshape(self.P, 9))
        self.per_pair_K = True

    def _load_targets(self):
        """where load() puts each blob: the resident loop buffers, or with several hypotheses the P pair rows that _expand reads"""
        if self.N > 1:
            return self.pair
        t = {"image_observed": self.batch["image_observed"], "image_rendered": self.init["image_rendered"],
             "mask_observed": self.init["mask_observed"], "mask_rendered": self.init["mask_rendered"], "src_pose": self.pose_init,
             "class_index": self.batch["class_index"]}
        if self.depth_observed is not None or self.input_depth:
            t["depth_observed"] = self.batch["depth_observed"] if self.input_depth else self.depth_observed
        if self.input_depth:
            t["depth_rendered"] = self.init["depth_rendered"]
        return t

    def _check_hyp_poses(self, hyp_poses):
        if hyp_poses is None:
            return
        if self.N == 1:
            raise ValueError("hyp_poses needs TEST.HYP_NUM > 1")
        if tuple(torch.as_tensor(hyp_poses).shape) != (self.P, self.N, 3, 4):
            raise ValueError("hyp_poses must be ({},{},3,4), got {}".format(self.P, self.N, tuple(torch.as_tensor(hyp_poses).shape)))

    def _expand(self, hyp_poses=None):
        """TEST.HYP_NUM > 1, eagerly once per batch: the P loaded pairs -> the B = P*N samples.  Starting poses (dim_hyp_expand, or the
        caller's), the observed blobs, class and K broadcast (dim_hyp_broadcast), and the hypotheses rendered as the loop re-renders
        (their mask_observed: the box of their own render under INIT_MASK 'box_rendered').  Without hyp_poses hypothesis 0 keeps the
        loaded planes.  Everything lands in the pristine buffers (`init`, pose_init) a replayed graph starts from.  The render's status
        bits stay in status_hyp; the selection ORs the winner's into its last status row (status_iter itself is rewritten by the loop)."""
        N, P, pr, b, init = self.N, self.P, self.pair, self.batch, self.init
        if hyp_poses is not None:
            self.pose_init.copy_(torch.as_tensor(hyp_poses).reshape(self.B, 3, 4))
        else:
            ops.hyp_expand(self.hyp_table, pr["src_pose"], N, out=self.pose_init)
        ops.hyp_broadcast(b["image_observed"], pr["image_observed"], N)
        ops.hyp_broadcast(b["class_index"], pr["class_index"], N)
        if "depth_observed" in pr:
            ops.hyp_broadcast(b["depth_observed"] if self.input_depth else self.depth_observed, pr["depth_observed"], N)
        if self.per_pair_K:
            ops.hyp_broadcast(self.K_pair, pr["K"], N)
        self._render_start()
        if self.cfg.TEST.INIT_MASK == "box_rendered":
            ops.box_mask(self.bbox_hyp, init["mask_observed"])
        else:
            ops.hyp_broadcast(init["mask_observed"], pr["mask_observed"], N)
        if hyp_poses is None:   # hypothesis 0: the loaded planes and masks
            for k in ("image_rendered", "mask_rendered", "mask_observed") + (("depth_rendered",) if self.input_depth else ()):
                row = pr[k].numel() // P
                ops.copy_rows(init[k], N * row, pr[k], row, P, row)

    def load_staged(self, loader, staged):
        """take the next batch straight from a deepim.core.loader.TestDataLoader staging set: the raw pixels it uploaded are turned
        into the resident blobs by dim_test_blobs_from_raw / dim_box_mask on the current stream -- no host blobs, no extra copies"""
        if self.V > 1:
            raise ValueError("TEST.VIEWS > 1 is not supported by load_staged (a staged batch carries no extrinsics, use load(..., cam_T_rig=))")
        if self.coarse is not None:
            raise ValueError("TEST.COARSE_VIEWS > 0: the staged batches carry no detection boxes, use load(..., det_boxes=)")
        if "sil" in self.stages and self.stages["sil"].which == "observed":
            raise ValueError("TEST.SIL_ITER > 0 with TEST.SIL_MASK 'observed': a staged batch carries the TEST.INIT_MASK mask of the loop, "
                             "not a segmentation; use load(..., mask_observed=)")
        dst = self._load_targets()
        out = {k: dst[k] for k in ("image_observed", "image_rendered", "mask_rendered", "mask_observed")}
        if self.depth_observed is not None:
            if not getattr(loader, "stage_depth_observed", False):
                raise ValueError(("TEST.ICP_ITER > 0" if self.icp_iter > 0 else "TEST.HYP_SCORE 'depth'") +
                                 ": the loader does not stage depth_observed")
            out["depth_observed"] = dst["depth_observed"]
        loader.build_blobs(staged, out=out)
        ops.copy(dst["src_pose"], staged.d_pose)
        ops.copy(dst["class_index"], staged.d_cls)
        self.per_pair_K = bool(getattr(loader, "per_pair_K", False))
        if self.per_pair_K:
            ops.copy(self.K_pair if self.N == 1 else self.pair["K"], staged.d_K)
        if self.N > 1:
            self._expand()
        loader.release(staged)   # the last read of the staging set's device mirrors is enqueued
        if self.lit and self.test_iter > 1:
            li = np.stack([[np.random.uniform(0.9, 1.1, size=(3,)) for _ in range(self.test_iter - 1)] for _ in range(self.B)])
            self.light_int.copy_(torch.from_numpy(li.transpose(1, 0, 2).astype(np.float32)))

    def _loop(self):
        """tester.py:476-598 for a whole batch; everything enqueued on the current stream, no host sync."""
        cfg, net, b = self.cfg, self.net, self.batch
        # The loaded blobs are read WHERE THEY LIE by the first forward; a working plane takes over once the loop has written it (the
        # first render writes image_rendered / mask_rendered [/ depth_rendered] in full, box_mask all of mask_observed).  Round 3
        # copied every pristine blob into its working plane at the start of each replay: 100 MB and ~40 us per step at 16 pairs.
        # A plane the loop never writes (one iteration only; UPDATE_MASK 'init': mask_observed) is still copied, so that `batch` ends
        # up as the reference leaves its data batch.  (ops.copy is a kernel: no memcpy / memset node may sit in the captured graph.)
        cur = dict(b)
        cur.update(self.init)
        box_update = cfg.network.INPUT_MASK and cfg.network.PRED_MASK and cfg.TEST.UPDATE_MASK == "box_rendered"
        for k, v in self.init.items():
            if self.test_iter < 2 or (k == "mask_observed" and not box_update):
                ops.copy(b[k], v)
                cur[k] = b[k]
        bbox_ren = bbox_obs = None
        pose = self.pose_init
        flow = self.stages.get("flow_pnp")
        if flow is not None:
            flow.start(self, pose)
        for it in range(self.test_iter):
            # se3 and status land directly in their per-iteration rows; the pose of the previous iteration is read where it lies
            out = net.forward_test(cur, bbox_ren=bbox_ren, bbox_obs=bbox_obs, src_pose=pose, se3_out=self.se3_iter[it],
                                   status_out=self.status_iter[it])
            if self.taps_iter is not None:
                net.zoom_area_taps(out=self.taps_iter[it])
            if self.mask_pred_iter is not None:
                ops.copy(self.mask_pred_iter[it], out["mask_observed_pred_output"])
            if self.flow_est_iter is not None:
                ops.copy(self.flow_est_iter[it], out["flow_est_crop_output"])
            if flow is not None:   # the result is recorded only: the next iteration starts from the head's pose
                flow.step(self, it, cur, pose, bbox_ren)
            # pose_rendered_update = RT_transform(pose_rendered, se3[:-3], se3[-3:], ...)   (:525-532)
            ops.se3_compose(pose, self.se3_iter[it], cfg.network.ROT_COORD, self.T_means, self.T_stds, out=self.poses_iter[it])
            if it < self.test_iter - 1:
                # render(render_machine, pose_rendered_update, cls_idx) + update_data_batch  (:563-590)
                extra = {"light_intensity": self.light_int[it]} if self.lit else {}
                if self.per_pair_K and not self.lit:
                    extra["K"] = self.K_pair   # read where it lies: a replayed graph renders with the K of the latest load
                # (the loop needs the depth only for mask_rendered = depth > 0.2, tester.py:575-577: the resolve pass writes the mask itself
                # and the depth plane is not materialised -- 1.2 MB per pair and render less to write)
                if self.input_depth:
                    extra["depth"] = b["depth_rendered"]   # INPUT_DEPTH: the rendered depth is a network input (tester.py:573-574)
                elif flow is not None:
                    extra["depth"] = flow.depth            # the next iteration's flow stage back-projects it
                # from the second render on the planes hold the previous render: background outside ITS box, which is not written again
                bb_new, bb_prev = (self.bbox, self.bbox2) if it % 2 == 0 else (self.bbox2, self.bbox)
                self.render_machine.render_batch(b["class_index"], self.poses_iter[it], image=b["image_rendered"],
                                                 mask=b["mask_rendered"], bbox=bb_new, plane_means=net.plane_means, mask_thr=0.2,
                                                 status=self.status_iter[it], clean_bbox=bb_prev if it > 0 else None, **extra)
                cur["image_rendered"], cur["mask_rendered"] = b["image_rendered"], b["mask_rendered"]
                if self.input_depth:
                    cur["depth_rendered"] = b["depth_rendered"]
                if box_update:
                    # data_pair.py:103-114; the rectangle's own bbox comes back with it, so ZoomMask does not scan the mask again
                    ops.box_mask(bb_new, b["mask_observed"], bbox_of_mask=self.bbox_obs)
                    bbox_obs = self.bbox_obs
                    cur["mask_observed"] = b["mask_observed"]
                pose = self.poses_iter[it]
                bbox_ren = bb_new
        ops.copy(b["src_pose"], pose)  # the blob ends up as the reference leaves it: the pose the last forward used
        if self.views is not None:   # one pose per group first; then every stage from it, with one correction per group
            self.views.run(self, self.poses_iter[self.test_iter - 1])
            pose, pose_rig = self.views.pose_views, self.views.pose_rig
            if self.calib is not None:   # the extrinsics first: the stages below read the calibrated ones and start from its poses
                self.calib.run(self, pose, pose_rig)
                pose, pose_rig = self.calib.pose, self.calib.pose_rig
            for name in [n for n in POST_LOOP if n in self.stages]:
                self.stages[name].run(self, pose, pose_rig)
            return
        for name in [n for n in POST_LOOP if n in self.stages]:   # independent of each other, all from the loop's last pose
            self.stages[name].run(self, self.poses_iter[self.test_iter - 1])
        if self.N > 1:
            self._select(self.poses_iter[self.test_iter - 1])

    def _select(self, pose):
        """several hypotheses: render the last pose of every sample (image, depth and the box of every drawn pixel; the pair's K when
        loaded), score it against the observed image (dim_pose_score) and keep the best hypothesis of each pair (dim_hyp_select)"""
        b, last = self.batch, self.status_iter[self.test_iter - 1]
        extra = {"K": self.K_pair} if self.per_pair_K else {}
        self.render_machine.render_batch(b["class_index"], pose, image=self.image_sc, depth=self.depth_sc, bbox=self.bbox_sc,
                                         plane_means=self.net.plane_means, mask_thr=0.0, status=last, **extra)
        depth_mode = self.hyp_score_mode == "depth"
        ops.pose_score(b["image_observed"], self.image_sc, self.depth_sc, self.hyp_score_mode, self.hyp_tau,
                       depth_observed=self.depth_observed if depth_mode else None, bbox=self.bbox_sc, score=self.hyp_score, status=last,
                       workspace=self.score_work)
        ops.hyp_select(self.hyp_score, self.N, self.poses_iter, status_iter=self.status_iter, status_load=self.status_hyp, pose_icp=self.pose_icp,
                       choice=self.hyp_choice, poses_sel=self.poses_sel, status_sel=self.status_sel, pose_icp_sel=self.pose_icp_sel)

    def _render_at(self, pose, status, **targets):
        """a stage's render of `pose` into `targets` (image / depth / bbox ..., every drawn pixel) -> the per-pair K it used, or None"""
        extra = {"light_intensity": self.light_int[0]} if self.lit else ({"K": self.K_pair} if self.per_pair_K else {})
        self.render_machine.render_batch(self.batch["class_index"], pose, mask_thr=0.0, status=status, **dict(targets, **extra))
        return extra.get("K")

    def refine(self):
        """run test_iter iterations on the loaded batch; returns poses_iter (test_iter,B,3,4) (device).  The stages of
        deepim.core.pose_stages that are on run inside the same graph: ICP, photometric and silhouette polish after the iterations, each
        from the same last pose, leave pose_icp / pose_photo / pose_sil (B,3,4); pose from flow at every iteration (dim_flow_pnp) leaves
        pose_flow_iter (test_iter,B,3,4), se3_flow_iter (test_iter,B,7), flow_pnp_stats (test_iter,B,FLOW_PNP_ITER,2) and status_flow
        (test_iter,B), which the loop itself never reads.  With TEST.HYP_NUM > 1 it returns the selected hypothesis of each pair, poses_sel
        (test_iter,P,3,4); poses_iter (P*N samples), hyp_score (P*N,), hyp_choice (P,), status_sel and pose_icp_sel stay readable."""
        if self.graph is not None and self._graph_per_pair_K != self.per_pair_K:
            self.graph = None   # captured with the other render (uniform / per-pair K): capture this one
        if self._want_graph and self.graph is None:
            self.graph = capture_graph(self._loop, self.net.device)
            self._graph_per_pair_K = self.per_pair_K
        if self.graph is not None:
            self.graph.replay()
        else:
            self._loop()
        return self.poses_iter if self.N == 1 else self.poses_sel


def _pair_view(refiner, cls=True, K=True, icp=False):
    """-> (class_index, K_pair, pose_icp) of the loaded batch, one row per pair: where a Refiner keeps them depends on its hypotheses
    (one per pair: the loop's own buffers; several: the pair rows, and the ICP pose of the selected hypothesis).  K_pair is None
    when no per-pair camera was loaded (the config K holds).  An entry that is not asked for is None and nothing is read for it."""
    one = int(getattr(refiner, "N", 1)) == 1
    return ((refiner.batch if one else refiner.pair)["class_index"] if cls else None,
            (refiner.K_pair if one else refiner.pair["K"]) if K and refiner.per_pair_K else None,
            (refiner.pose_icp if one else refiner.pose_icp_sel) if icp else None)


class VsdScorer(object):
    """TEST.VSD and TEST.BOP_VSD: the visible surface discrepancy of every pose pred_eval scores, against the batch's observed depth.
    Per batch the ground truth is rendered once (depth and box only, float32 pose, the pair's K when one was loaded) with the refiner's
    render machine; per scored pose set the estimate is rendered once into one reused plane, and from the same three planes
    TEST.VSD: dim_vsd_errors fills that set's row of `errors` (rows, P, n_tau) float64 and `counts` (rows, P, 4) int32 (absolute taus);
    TEST.BOP_VSD: dim_vsd_grid_errors fills its row of `grid_errors` (rows, P, len(BOP_VSD_TAU)) float64 and `grid_counts`
    (rows, P, 4) int32, at the taus of each pair's class (PoseEvaluator.device_vsd_tau_table).
    Nothing leaves the device here.  Either half is allocated only when its key is on."""

    def __init__(self, config, refiner, rows, evaluator=None):
        T = config.TEST
        self.absolute = bool(T.get("VSD", False))
        self.grid, self.grid_delta, fracs = bop_vsd_settings(config)
        who = "TEST.VSD" if self.absolute else "TEST.BOP_VSD"
        if getattr(refiner, "lit", False):
            raise ValueError("{} is not supported with the lit ModelNet renderer".format(who))
        self.refiner, self.rm = refiner, refiner.render_machine
        P, H, W, d = refiner.P, self.rm.height, self.rm.width, refiner.net.device
        if self.absolute:
            self.taus = [float(t) for t in np.asarray(T.VSD_TAU, dtype=np.float64).reshape(-1)]
            if not 1 <= len(self.taus) <= ops.VSD_MAX_TAU or not all(np.isfinite(t) and t > 0 for t in self.taus):
                raise ValueError("TEST.VSD_TAU must hold 1 to {} finite distances > 0 (metres), got {!r}".format(ops.VSD_MAX_TAU, T.VSD_TAU))
            self.delta, self.cost = float(T.VSD_DELTA), T.VSD_COST
            if self.cost not in ops.VSD_COST_ID:
                raise ValueError("TEST.VSD_COST must be 'step' or 'tlinear', got {!r}".format(self.cost))
            self.errors = torch.zeros((rows, P, len(self.taus)), dtype=torch.float64, device=d)
            self.counts = torch.zeros((rows, P, 4), dtype=torch.int32, device=d)
            self.work = ops.vsd_workspace(1, P, d)
        if self.grid:
            if evaluator is None:
                raise ValueError("TEST.BOP_VSD needs the evaluator (its class diameters give the taus)")
            self.tau_table = evaluator.device_vsd_tau_table(d, fracs)
            self.grid_errors = torch.zeros((rows, P, len(fracs)), dtype=torch.float64, device=d)
            self.grid_counts = torch.zeros((rows, P, 4), dtype=torch.int32, device=d)
            self.grid_n_ge = torch.zeros((rows, P, len(fracs)), dtype=torch.int32, device=d)
            self.grid_work = ops.vsd_grid_workspace(1, P, d)
        self.K = np.asarray(self.rm.K, dtype=np.float64)   # the camera the planes are rendered with
        self.depth_gt = torch.zeros((P, 1, H, W), dtype=torch.float32, device=d)
        self.depth_est = torch.zeros((P, 1, H, W), dtype=torch.float32, device=d)
        self.depth_obs = None   # allocated only when the refiner keeps no observed depth of its own
        self.bbox_gt = torch.zeros((P, 4), dtype=torch.int32, device=d)
        self.bbox_est = torch.zeros((P, 4), dtype=torch.int32, device=d)
        self.rm.reserve(P)

    @staticmethod
    def check(batch, who="TEST.VSD"):
        if batch.get("depth_observed") is None:
            raise KeyError("{} needs the blob 'depth_observed' (the test image's depth in metres)".format(who))

    def _observed(self, batch):
        """the pairs' observed depth where the refiner already holds it (ICP, the depth hypothesis score, INPUT_DEPTH), else a copy"""
        r = self.refiner
        if r.N > 1 and "depth_observed" in r.pair:
            return r.pair["depth_observed"]
        if r.N == 1 and (r.depth_observed is not None or r.input_depth):
            return r.batch["depth_observed"] if r.input_depth else r.depth_observed
        if self.depth_obs is None:
            self.depth_obs = torch.zeros_like(self.depth_gt)
        self.depth_obs.copy_(torch.as_tensor(batch["depth_observed"]).reshape(self.depth_gt.shape))
        return self.depth_obs

    def score(self, batch, pose_sets):
        """pose_sets: list of (P,3,4) float32 device poses, one per row of errors / counts (and of grid_errors / grid_counts)"""
        cls, K_pair, _ = _pair_view(self.refiner)
        extra = {"K": K_pair} if K_pair is not None else {}
        K64 = K_pair.to(torch.float64) if K_pair is not None else None
        obs = self._observed(batch)
        gt = torch.as_tensor(batch["pose_observed"]).to(self.depth_gt.device, torch.float32).contiguous()
        self.rm.render_batch(cls, gt, depth=self.depth_gt, bbox=self.bbox_gt, mask_thr=0.0, **extra)
        for row, pose in enumerate(pose_sets):
            self.rm.render_batch(cls, pose, depth=self.depth_est, bbox=self.bbox_est, mask_thr=0.0, **extra)
            if self.absolute:
                ops.vsd_errors(obs, self.depth_gt, self.depth_est, self.K, self.delta, self.taus, self.cost, K_per_sample=K64,
                               bbox_gt=self.bbox_gt, bbox_est=self.bbox_est, errors=self.errors[row], counts=self.counts[row],
                               workspace=self.work)
            if self.grid:
                ops.vsd_grid_errors(obs, self.depth_gt, self.depth_est, self.K, self.grid_delta, cls, self.tau_table, K_per_sample=K64,
                                    bbox_gt=self.bbox_gt, bbox_est=self.bbox_est, errors=self.grid_errors[row],
                                    counts=self.grid_counts[row], n_ge=self.grid_n_ge[row], workspace=self.grid_work)

    def packed(self):
        """(rows, P, n_tau + 4) float64: the errors and, behind them, the counts (exact in float64)"""
        return torch.cat([self.errors, self.counts.to(torch.float64)], dim=2)

    def packed_grid(self):
        """(rows, P, len(BOP_VSD_TAU) + 4) float64: the grid errors and, behind them, their counts"""
        return torch.cat([self.grid_errors, self.grid_counts.to(torch.float64)], dim=2)


class BopScorer(object):
    """TEST.BOP: the BOP symmetry-aware errors MSSD and MSPD of every pose pred_eval scores, under the evaluator's symmetry sets
    (PoseEvaluator.device_sym_tables at TEST.BOP_SYM_STEP).  One dim_bop_errors call per batch on the float32 poses where refine()
    left them (the ICP pose as one more row), with the pair's K when one was loaded and the config K otherwise: `errors`
    (rows, P, 2) float64 and `best_sym` (rows, P, 2) int32.  Nothing leaves the device here."""

    def __init__(self, config, refiner, evaluator, rows):
        step = float(config.TEST.BOP_SYM_STEP)
        if not (np.isfinite(step) and step > 0):
            raise ValueError("TEST.BOP_SYM_STEP must be a finite step > 0, got {!r}".format(config.TEST.BOP_SYM_STEP))
        self.refiner = refiner
        P, d = refiner.P, refiner.net.device
        self.points, self.table_off = evaluator.device_tables(d)[:2]
        self.sym, self.sym_off = evaluator.device_sym_tables(d, step)
        self.max_sym = evaluator.max_sym(step)
        self.K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float64)
        self.rows = rows
        self.poses = torch.zeros((rows, P, 3, 4), dtype=torch.float32, device=d)
        self.errors = torch.zeros((rows, P, 2), dtype=torch.float64, device=d)
        self.best_sym = torch.zeros((rows, P, 2), dtype=torch.int32, device=d)
        self.work = ops.bop_errors_workspace(rows, P, self.max_sym, d)

    def score(self, batch, poses, pose_icp=None):
        """poses (rows [- 1], P, 3, 4) float32 on the device, pose_icp (P,3,4) the last row when given"""
        if pose_icp is not None:   # one call needs the rows in one array
            self.poses[:-1].copy_(poses)
            self.poses[-1].copy_(pose_icp)
            poses = self.poses
        assert poses.shape[0] == self.rows
        cls, K_pair, _ = _pair_view(self.refiner)
        gt = torch.as_tensor(batch["pose_observed"]).to(self.errors.device, torch.float64).contiguous()
        ops.bop_errors(self.points, self.table_off, self.sym, self.sym_off, cls, poses.contiguous(), gt, self.K, self.max_sym,
                       K_per_sample=K_pair, errors=self.errors, best_sym=self.best_sym, workspace=self.work)

    def packed(self):
        """(rows, P, 4) float64: {mssd, mspd} and, behind them, the two symmetry indices (exact in float64)"""
        return torch.cat([self.errors, self.best_sym.to(torch.float64)], dim=2)


class FlowEPE(object):
    """Test-time flow error, reference deepim/core/tester.py:500-512 (accumulation), :675-716 (par_generate_gt) and :719-736
    (calc_EPE_one_pair), active when `PRED_FLOW and not FAST_TEST`: the flow head's output of the FIRST forward of every pair
    (`rst_iter` is built from predictor.predict before the refinement loop, :476-494) against calc_flow(depth_rendered,
    pose_rendered, pose_observed, K, depth_gt_observed) of the initial pair.  Labels (dim_calc_flow_labels) and the three masked
    error sums (dim_flow_epe_sums) stay on the device; ONE (5,) float64 read-out at the end."""

    def __init__(self, config, batch_size, device):
        self.cfg = config
        K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float64).reshape(3, 3)
        self.K = K
        self.Kinv64 = np.linalg.inv(K)
        H, W = source_size(config)
        refuse_at_source_size(config, (H, W))   # the flow head's output exists at the network size only
        B = batch_size
        self.flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=device)
        self.weights = torch.empty((B, 2, H, W), dtype=torch.float32, device=device)
        self.sums = torch.zeros((B, 5), dtype=torch.float64, device=device)
        self.work = torch.empty((ops.lib().dim_flow_epe_workspace_bytes(B) // 8,), dtype=torch.float64, device=device)
        self.P12 = torch.empty((B, 3, 4), dtype=torch.float64, device=device)
        self.num_all = 0

    def add(self, batch, flow_est, skip=None):
        """batch: depth_rendered (B,1,H,W) of the initial render, depth_gt_observed (B,1,H,W) (zero off the object: tester.py:700-704),
        src_pose, pose_observed; flow_est (B,2,H,W) = flow_est_crop_output of the first forward.  skip: (B,) bool, pairs that are not
        scored (undetected objects leave the loop before the flow error, :451-475)."""
        from lib.utils.projection import se3_inverse, se3_mul

        for k in ("depth_rendered", "depth_gt_observed", "pose_observed"):
            if k not in batch:
                raise KeyError("test-time flow error (PRED_FLOW and not FAST_TEST) needs the blob '{}' (par_generate_gt reads it from "
                               "the pair record, tester.py:681-704)".format(k))
        src = torch.as_tensor(batch["src_pose"]).cpu().numpy().astype(np.float64)
        tgt = torch.as_tensor(batch["pose_observed"]).cpu().numpy().astype(np.float64)
        P = np.stack([np.matmul(self.K, se3_mul(tgt[b], se3_inverse(src[b]))) for b in range(src.shape[0])])   # flow.py:31
        self.P12.copy_(torch.from_numpy(np.ascontiguousarray(P)))
        dr = torch.as_tensor(batch["depth_rendered"]).to(self.flow.device, torch.float32).contiguous()
        dg = torch.as_tensor(batch["depth_gt_observed"]).to(self.flow.device, torch.float32).contiguous()
        ops.calc_flow_labels(dr, dg, self.P12, self.Kinv64, self.flow, self.weights, standard_rep=bool(self.cfg.network.STANDARD_FLOW_REP),
                             weight_type="viz")
        per = ops.flow_epe_sums(flow_est, self.flow, self.weights[:, :1].contiguous(), dr, workspace=self.work)
        if skip is not None and bool(np.any(skip)):
            per = per * torch.from_numpy(~np.asarray(skip, dtype=bool)).to(per.device, torch.float64)[:, None]
        self.sums += per
        self.num_all += int(per.shape[0] - (0 if skip is None else int(np.sum(skip)))) * dr.shape[2] * dr.shape[3]

    def result(self, merge_ranks=True):
        """-> dict(epe_all, epe_vizbg, epe_viz: the three numbers the reference prints at :656-660; sums and counts next to them)"""
        import torch.distributed as dist

        t = torch.cat([self.sums.sum(0), torch.tensor([float(self.num_all)], dtype=torch.float64, device=self.sums.device)]).cpu()
        if merge_ranks and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, t.numpy())
            t = torch.from_numpy(np.sum(parts, axis=0))
        s_all, s_viz, s_vizbg, n_viz, n_vizbg, n_all = (float(v) for v in t)
        return {"epe_all": s_all / max(n_all, 1.0), "epe_vizbg": s_vizbg / max(n_vizbg, 1.0), "epe_viz": s_viz / max(n_viz, 1.0),
                "sum_EPE_all": s_all, "sum_EPE_viz": s_viz, "sum_EPE_vizbg": s_vizbg, "num_inst_all": n_all, "num_inst_viz": n_viz,
                "num_inst_vizbg": n_vizbg}


def pred_eval(config, refiner, batches, evaluator, result_file=None, logger=None, merge_ranks=True):
    """The outer loop of the reference's pred_eval (deepim/core/tester.py:418-676) on device-resident batches.

    batches: iterable of dicts with the blobs Refiner.load takes plus "pose_observed" (B,3,4) ground truth.
    Collects all_poses_est[cls][iter] / all_poses_gt[cls][iter] and the rotation / translation errors per iteration exactly as
    the reference does (:497-560), writes the result cache [all_rot_err, all_trans_err, all_poses_est, all_poses_gt] with
    pickle protocol 2 (:650-654) and runs evaluate_pose / evaluate_pose_add / evaluate_pose_arp_2d (:664-673).
    evaluator: lib.dataset.evaluation.PoseEvaluator.  Returns the three result dicts.
    With TEST.ICP_ITER > 0 the refiner's ICP poses are scored too, as the one-row table of the reference's PRECOMPUTED_ICP branch
    (tester.py:253-330), under out["icp"] = {pose, add, arp_2d}; every other output and the result cache are those of ICP off.
    With TEST.PHOTO_ITER > 0 the refiner's photometrically polished poses (pose_photo) are scored the same way, as a one-row table
    under out["photo"] = {pose, add, arp_2d} (the host error functions, or dim_pose_errors under TEST.DEVICE_EVAL; one more copy per
    batch); every other output and the result cache are those of the stage off.  Scoring that row by TEST.VSD / TEST.BOP is left out:
    the combination raises a ValueError.
    With TEST.SIL_ITER > 0 the silhouette-polished poses (pose_sil) are scored exactly so under out["sil"], with the same refusals.
    With TEST.HYP_NUM = N > 1 every table, the result cache and out["icp"] score the selected hypothesis of each pair, and out["hyp"]
    holds per pair the N scores, the choice and the last-iteration rotation / translation error of every hypothesis, plus the rate
    at which the chosen hypothesis is also the one with the least rotation error.  A batch may carry "hyp_poses" (P,N,3,4).
    With TEST.DEVICE_EVAL the errors behind the three tables (and out["icp"]) come from dim_pose_errors on the poses where refine()
    left them, and reach the host in the batch's one copy next to the poses; pairs that were not refined (undetected) are scored on the
    host as before.  Every output keeps its meaning; out["device_eval"] = True is added.
    With TEST.VSD every scored pose (and the ICP pose) also gets its visible surface discrepancy against the batch's "depth_observed"
    (VsdScorer, dim_vsd_errors): out["vsd"] = the table of PoseEvaluator.evaluate_pose_vsd plus "errors", the per-pose lists
    {vsd, visib_gt, union, inter, drawn_gt}[cls][iter] in the order of all_poses_est; out["icp"]["vsd"] the same for the ICP row.  A
    pair that was not refined scores 1.0.  The numbers ride in the device-to-host copy of TEST.DEVICE_EVAL, or come in one copy of
    their own per batch.  Every other output and the result cache are those of VSD off.
    With TEST.BOP every scored pose (and the ICP pose) also gets the BOP symmetry-aware errors MSSD and MSPD under the evaluator's
    symmetry sets (BopScorer, one dim_bop_errors call per batch): out["bop"] = the table of PoseEvaluator.evaluate_pose_bop plus
    "errors", the per-pose lists {mssd, mspd, sym_mssd, sym_mspd}[cls][iter] in the order of all_poses_est; out["icp"]["bop"] the same
    for the ICP row.  A pair that was not refined scores inf for both (symmetry -1).  The numbers travel like the VSD ones.  Every
    other output and the result cache are those of BOP off.
    With TEST.BOP_VSD (needs TEST.BOP and "depth_observed") every scored pose also gets the step-cost VSD at the fractions
    TEST.BOP_VSD_TAU of its class's diameter (VsdScorer, dim_vsd_grid_errors on the renders TEST.VSD uses when both are on):
    out["bop"]["bop19"] = the table of PoseEvaluator.evaluate_pose_bop19 (AR_VSD, AR_MSSD, AR_MSPD, AR per class, over the classes and
    pooled) plus "errors", the per-pose lists {vsd_grid, visib_gt, union, inter, drawn_gt, mssd, mspd}[cls][iter]; out["icp"]["bop19"]
    the same for the ICP row.  A pair that was not refined scores 1.0 with zero counts, so it is no target.  Every other output and
    the result cache are those of BOP_VSD off.
    With TEST.FLOW_PNP_ITER > 0 the refiner's poses from flow (pose_flow_iter, one per loop iteration) are scored next to the head's,
    by the same error code (the host functions, or dim_pose_errors under TEST.DEVICE_EVAL): out["flow_pnp"] = {pose, add: the tables
    of evaluate_pose / evaluate_pose_add; all_rot_err, all_trans_err; inliers, rms: per loop iteration the mean over the refined pairs
    of the stage's last weighted point count and pixel rms; flagged: per loop iteration the number of pairs with
    DIM_STATUS_FLOW_PNP_FEW_POINTS}.  Every other output and the result cache are those of the stage off.
    With TEST.COARSE_VIEWS > 0 (a Refiner with a coarse stage) every pair starts from its detection box: the batch's "det_bbox" (P,4)
    {x0,x1,y0,y1} continuous pixel extents when it carries one, otherwise the box of its "mask_observed" (dim_mask_bbox, widened by
    half a pixel to each side).  "src_pose", "image_rendered" and "mask_rendered" are not read (the pair's best coarse pose stands for
    src_pose).  out["coarse"] = {idx, score, status, pose}: per pair the HYP_NUM kept candidates of the coarse stage, best first.
    With TEST.VISUALIZE every refined batch is also drawn (deepim.core.visualize.PoseVisualizer: contour overlays of the ground truth,
    the initial and the refined poses under TEST.VIS_DIR); every output is that of the switch off."""
    refuse_with_views(config, "pred_eval (its score tables are per pair, not per rig pose)")
    st = _eval_setup(config, refiner, evaluator, logger)
    for batch in batches:
        _collect_batch(st, refiner, batch)
    # several ranks refine disjoint shards (one process per GPU): the metrics are over ALL pairs, so the lists are merged in rank
    # order on every rank before scoring (the reference scores one list in one process)
    import torch.distributed as dist

    merged = bool(merge_ranks) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if merged:
        st.store = _merge_over_ranks(st.store)
        if dist.get_rank() != 0:
            result_file = None   # one result cache, written by rank 0
    return _tables(st, result_file, merge_ranks, merged)


def _eval_setup(config, refiner, evaluator, logger):
    """what one pred_eval call holds: the switches, the device scorers and `store`, every list it collects under its name --
    (pose set, family) -> ScoreLists for the sets "loop", "icp", "flow_pnp", "photo" and "sil" and the families of FAMILY_KEYS, and the per-pair
    "hyp", "flow_rows" and "coarse" -> PairLists.  A name is there only when its feature is on."""
    from types import SimpleNamespace

    bop_vsd = bop_vsd_settings(config)[0]   # before anything is allocated: BOP_VSD without BOP raises here
    T = config.TEST
    st = SimpleNamespace(config=config, evaluator=evaluator, logger=logger, n_cls=len(evaluator.classes), n_it=int(T.test_iter),
                         on=stages_on(config), n_hyp=int(getattr(refiner, "N", 1)), device_eval=bool(T.get("DEVICE_EVAL", False)),
                         with_coarse=getattr(refiner, "coarse", None) is not None, vsd=None, bop=None,
                         vsd_who="TEST.VSD" if bool(T.get("VSD", False)) else "TEST.BOP_VSD")
    st.with_icp, st.with_flow = "icp" in st.on, "flow_pnp" in st.on
    for s in ONE_ROW_SETS:
        if s.name in st.on and not s.full and (bool(T.get("VSD", False)) or bool(T.get("BOP", False))):
            raise ValueError("TEST.{} > 0 cannot be combined with TEST.VSD or TEST.BOP (the {} row is not scored there)".format(
                STAGE_KEY[s.name], s.word))
    if st.device_eval:
        from lib.dataset.evaluation import SYM_CLASSES

        st.dev = refiner.net.device
        st.tables = evaluator.device_tables(st.dev)
        st.K_eval = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float64)
        st.uses_adi = [c in SYM_CLASSES for c in evaluator.classes]
    rows = st.n_it + (1 if st.with_icp else 0)   # the device scorers take the ICP pose as one more row
    if bool(T.get("VSD", False)) or bop_vsd:     # one scorer renders for TEST.VSD and the grid of TEST.BOP_VSD
        st.vsd = VsdScorer(config, refiner, rows, evaluator)
    if bool(T.get("BOP", False)):
        st.bop = BopScorer(config, refiner, evaluator, rows)
    on = {"rt": True, "err": st.device_eval, "vsd": st.vsd is not None and st.vsd.absolute, "grid": bop_vsd, "bop": st.bop is not None}
    families = [f for f in FAMILY_KEYS if on[f]]
    error_code = [f for f in families if f in ("rt", "err")]
    sets = [("loop", st.n_it, families)]
    sets += [(s.name, 1, families if s.full else error_code) for s in ONE_ROW_SETS if s.name in st.on]
    if st.with_flow:   # pose from flow at every iteration: scored by the error code alone
        sets.append(("flow_pnp", st.n_it, error_code))
    st.store = {(name, f): ScoreLists(FAMILY_KEYS[f], st.n_cls, iters) for name, iters, fams in sets for f in fams}
    st.scored = list(st.store)
    if st.n_hyp > 1:
        st.store["hyp"] = PairLists(HYP_KEYS)
    if st.with_flow:   # per refined pair (iter, 3) = (weighted points, rms, flagged) of the stage's last Gauss-Newton iteration
        st.store["flow_rows"] = PairLists(("stats",))
    if st.with_coarse:
        st.store["coarse"] = PairLists(COARSE_KEYS)
    # flow error of the first forward (:500-512): only the full test graph emits the flow head's output
    st.epe = FlowEPE(config, getattr(refiner, "P", refiner.B), refiner.net.device) if (config.network.PRED_FLOW and not T.FAST_TEST) else None
    st.vis = None   # TEST.VISUALIZE: the overlays of every refined batch (deepim/core/visualize.py); off: nothing is imported or allocated
    if bool(T.get("VISUALIZE", False)):
        from deepim.core.visualize import PoseVisualizer

        st.vis = PoseVisualizer(config, refiner, evaluator)
    return st


def _cat(tensors, dim):
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=dim)


def _to_host(columns):
    """columns: [(name, width, (rows, P, ...) device tensor)] -> {name: its (rows, P, width) float64 of the ONE device->host copy
    of the columns side by side, in the order given}"""
    host = _cat([t.reshape(t.shape[0], -1, w) for _, w, t in columns], 2).cpu().numpy().astype(np.float64, copy=False)
    out, at = {}, 0
    for name, w, _ in columns:
        out[name], at = host[:, :, at:at + w], at + w
    assert at == host.shape[2]
    return out


def _read_out(st, batch, poses_dev, p_icp, cls_dev, gt_dev):
    """score the refined batch on the device and bring it to the host -> {column: (rows, P, width) float64}, rows = the loop's
    iterations and behind them the ICP pose when there is one; "pose" is (rows, P, 3, 4).  TEST.DEVICE_EVAL: the errors of every
    pose from dim_pose_errors, packed behind the poses (float32 -> float64 is exact) with the scorers' columns: ONE copy per batch.
    Otherwise one copy per column: the poses, the scorers' in the same order, then the ICP pose."""
    f64 = torch.float64
    columns = []
    if st.vsd is not None:
        st.vsd.score(batch, list(poses_dev) + ([p_icp] if p_icp is not None else []))
        if st.vsd.absolute:
            columns.append(("vsd", len(st.vsd.taus) + 4, st.vsd.packed()))
        if st.vsd.grid:
            columns.append(("grid", st.vsd.grid_errors.shape[2] + 4, st.vsd.packed_grid()))
    if st.bop is not None:
        st.bop.score(batch, poses_dev, p_icp)
        columns.append(("bop", 4, st.bop.packed()))
    if st.device_eval:
        P, t = gt_dev.shape[0], st.tables
        sets = [poses_dev] + ([p_icp] if p_icp is not None else [])
        errs = [ops.pose_errors(t[0], t[1], t[2], cls_dev, p, gt_dev, st.K_eval).reshape(-1, P, 5) for p in sets]
        host = _to_host([("pose", 12, _cat([p.to(f64).reshape(-1, P, 12) for p in sets], 0)), ("err", 5, _cat(errs, 0))] + columns)
    else:
        host = {}
        for column in [("pose", 12, poses_dev)] + columns + ([("pose_icp", 12, p_icp[None])] if p_icp is not None else []):
            host.update(_to_host([column]))
        if p_icp is not None:
            host["pose"] = np.concatenate([host["pose"], host.pop("pose_icp")])
    host["pose"] = host["pose"].reshape(len(host["pose"]), -1, 3, 4)
    return host


def _read_out_flow(st, refiner, cls_dev, gt_dev):
    """one more copy per batch with TEST.FLOW_PNP_ITER > 0: the flow poses [and their device errors], and the stage's last stats
    and flag -> {pose (iter, P, 3, 4), [err (iter, P, 5)], stats (iter, P, 3)}"""
    f64, n_it, t = torch.float64, st.n_it, st.tables if st.device_eval else None
    columns = [("pose", 12, refiner.pose_flow_iter.to(f64))]
    if st.device_eval:
        columns.append(("err", 5, ops.pose_errors(t[0], t[1], t[2], cls_dev, refiner.pose_flow_iter, gt_dev, st.K_eval)))
    columns += [("stats", 2, refiner.flow_pnp_stats[:, :, -1].to(f64)),
                ("flagged", 1, (refiner.status_flow & ops.STATUS_FLOW_PNP_FEW_POINTS).ne(0).to(f64))]
    host = _to_host(columns)
    host["pose"] = host["pose"].reshape(n_it, -1, 3, 4)
    host["stats"] = np.concatenate([host["stats"], host.pop("flagged")], axis=2)
    return host


def _read_out_pose(st, pose, cls_dev, gt_dev):
    """one more copy per batch for a one-row pose set outside _read_out's rows: (P,3,4) [and its device errors] -> {pose (1,P,3,4), [err (1,P,5)]}"""
    columns = [("pose", 12, pose.to(torch.float64)[None])]
    if st.device_eval:
        columns.append(("err", 5, ops.pose_errors(*st.tables[:3], cls_dev, pose, gt_dev, st.K_eval).reshape(1, -1, 5)))
    host = _to_host(columns)
    host["pose"] = host["pose"].reshape(1, -1, 3, 4)
    return host


def _pair_values(st, family, rows, b, undetected, src, gt, cls_b):
    """What pair b adds to the lists of one family for one pose set: one tuple of FAMILY_KEYS[family] values per row of `rows`
    (iterations, ...), the pair's rows of the family's column.  This is the one place of the rule for a pair that was not refined,
    "NO POINT VALID IN INIT POSE" (:419-445): an undetected object comes with pose_rendered = -1 everywhere (sum -12) and is scored
    with its initial pose and 1000 deg / 1000 m at every iteration instead of its rows; under TEST.DEVICE_EVAL by the host error
    functions on that pose; its VSD is 1.0 with no counts, whatever its -1 pose rendered; its BOP errors are inf, attained by no
    symmetry."""
    from lib.utils.pose_error import calc_rt_dist_m

    if family == "err" and undetected:
        host = tuple(float(v) for v in st.evaluator.host_pose_errors(st.config, st.evaluator.classes[cls_b], src[b], gt[b]))
    for row in rows:
        if family == "rt":
            est = src[b] if undetected else row
            yield ((1000, 1000) if undetected else tuple(calc_rt_dist_m(est, gt[b]))) + (est, gt[b])
        elif family == "err":   # {re, te, add, adi, arp_2d} -> ERR_KEYS: a symmetric class is scored by ADD-S
            yield host if undetected else tuple(float(v) for v in (row[0], row[1], row[3] if st.uses_adi[cls_b] else row[2], row[4]))
        elif family in ("vsd", "grid"):   # the errors, one per tau, and the four counts behind them
            n = len(row) - 4
            yield ([1.0] * n, 0, 0, 0, 0) if undetected else (row[:n].tolist(),) + tuple(int(v) for v in row[n:])
        else:
            yield (float("inf"), float("inf"), -1, -1) if undetected else (float(row[0]), float(row[1]), int(row[2]), int(row[3]))


def _collect_batch(st, refiner, batch):
    """load, refine and score one batch; its pairs go behind what `st.store` holds"""
    n_it, n_hyp, store = st.n_it, st.n_hyp, st.store
    extra = {"hyp_poses": batch["hyp_poses"]} if batch.get("hyp_poses") is not None else {}
    if st.with_coarse:
        det = batch.get("det_bbox")
        if det is None:
            mask = torch.as_tensor(batch["mask_observed"]).to(refiner.net.device, torch.float32).contiguous()
            det = boxes_from_int(ops.mask_bbox(mask, 0.5))
        extra["det_boxes"] = det
    if st.vsd is not None:
        st.vsd.check(batch, st.vsd_who)
    if st.with_flow and "pose_observed" not in batch:
        raise KeyError("pose from flow (TEST.FLOW_PNP_ITER > 0) needs the blob 'pose_observed' to be scored")
    if st.with_coarse:
        refiner.load(batch["image_observed"], None, batch.get("mask_observed"), None, None, batch["class_index"],
                     depth_observed=batch.get("depth_observed"), K=batch.get("K"), **extra)
        # one more copy per batch; the best candidate stands for the batch's src_pose
        co = {k: v.cpu().numpy() for k, v in refiner.coarse_out.items()}
        pose64 = co["pose"].astype(np.float64)
        for p in range(len(pose64)):
            store["coarse"].append([pose64[p] if k == "pose" else co[k][p].tolist() for k in COARSE_KEYS])
        batch = dict(batch, src_pose=co["pose"][:, 0].copy())
    else:
        refiner.load(batch["image_observed"], batch["image_rendered"], batch["mask_observed"], batch["mask_rendered"], batch["src_pose"],
                     batch["class_index"], depth_observed=batch.get("depth_observed"), K=batch.get("K"), **extra)
    poses_dev = refiner.refine()
    if st.vis is not None:
        st.vis.draw(batch)
    cls_dev, _, p_icp = _pair_view(refiner, cls=st.device_eval, K=False, icp=st.with_icp)
    gt_dev = torch.as_tensor(batch["pose_observed"]).to(st.dev, torch.float64).contiguous() if st.device_eval else None
    host = _read_out(st, batch, poses_dev, p_icp, cls_dev, gt_dev)
    by_set = {"loop": {k: v[:n_it] for k, v in host.items()}, "icp": {k: v[n_it:] for k, v in host.items()}}
    if st.with_flow:
        by_set["flow_pnp"] = _read_out_flow(st, refiner, cls_dev, gt_dev)
    for s in ONE_ROW_SETS:
        if s.name in st.on and not s.full:
            by_set[s.name] = _read_out_pose(st, getattr(refiner, s.pose), cls_dev, gt_dev)
    cls = torch.as_tensor(batch["class_index"]).cpu().numpy().astype(int)
    gt = torch.as_tensor(batch["pose_observed"]).cpu().numpy().astype(np.float64)
    src = torch.as_tensor(batch["src_pose"]).cpu().numpy().astype(np.float64)
    undetected = [bool(np.sum(src[b]) == -12) for b in range(len(src))]
    if st.epe is not None:   # defined on hypothesis 0, the loaded render
        flow0 = refiner.flow_est_iter[0] if n_hyp == 1 else refiner.flow_est_iter[0][::n_hyp].contiguous()
        st.epe.add(batch, flow0, skip=np.sum(src.reshape(src.shape[0], -1), axis=1) == -12)
    if n_hyp > 1:   # per pair the N scores, the choice and the last-iteration errors of every hypothesis
        scores = refiner.hyp_score.cpu().numpy().reshape(-1, n_hyp).astype(np.float64)
        choice = refiner.hyp_choice.cpu().numpy().astype(int)
        last = refiner.poses_iter[-1].cpu().numpy().astype(np.float64).reshape(-1, n_hyp, 3, 4)
    for b in range(host["pose"].shape[1]):
        if n_hyp > 1:
            errs = list(_pair_values(st, "rt", last[b], b, undetected[b], src, gt, cls[b]))
            store["hyp"].append((scores[b].tolist(), int(choice[b]), [e[0] for e in errs], [e[1] for e in errs], undetected[b]))
        for name, family in st.scored:
            rows = by_set[name]["pose" if family == "rt" else family][:, b]
            for it, values in enumerate(_pair_values(st, family, rows, b, undetected[b], src, gt, cls[b])):
                store[name, family].append(cls[b], it, values)
        if st.with_flow and not undetected[b]:   # the stage's statistics count refined pairs only
            store["flow_rows"].append((by_set["flow_pnp"]["stats"][:, b].tolist(),))


def _merge_over_ranks(store):
    """-> what every rank collected, rank after rank under every name: one all_gather_object of the whole store"""
    import torch.distributed as dist

    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, store)
    for part in parts[1:]:
        for name, lists in parts[0].items():
            lists.extend(part[name])
    return parts[0]


def _say(logger, line):
    print(line)
    if logger:
        logger.info(line)


def _pose_tables(st, config, name, arp_2d=True):
    """-> {pose, add [, arp_2d], all_rot_err, all_trans_err} of one pose set: the evaluator's tables on its lists (with
    TEST.DEVICE_EVAL on the device's errors; flag off: the evaluator is called as before)"""
    ev, rt = st.evaluator, st.store[name, "rt"]
    est, gt = rt["poses_est"], rt["poses_gt"]
    given = {"errors": st.store[name, "err"].lists} if st.device_eval else {}
    out = {"pose": ev.evaluate_pose(config, est, gt, st.logger, **given),
           "add": ev.evaluate_pose_add(config, est, gt, output_dir=None, logger=st.logger, **given)}
    if arp_2d:
        out["arp_2d"] = ev.evaluate_pose_arp_2d(config, est, gt, output_dir=None, logger=st.logger, **given)
    return dict(out, all_rot_err=rt["rot_err"], all_trans_err=rt["trans_err"])


def _scorer_tables(st, name):
    """-> {[vsd], [bop], [bop19]} of one pose set: each scorer's table plus "errors", its per-pose lists"""
    ev, config, store, out = st.evaluator, st.config, st.store, {}
    if (name, "vsd") in store:
        out["vsd"] = dict(ev.evaluate_pose_vsd(config, store[name, "vsd"].lists, st.logger), errors=store[name, "vsd"].lists)
    if (name, "bop") in store:
        bop = store[name, "bop"]
        out["bop"] = dict(ev.evaluate_pose_bop(config, bop.lists, st.logger), errors=bop.lists)
        if (name, "grid") in store:   # AR_VSD on the grid, and AR with the two errors above
            errs = dict(store[name, "grid"].lists, mssd=bop["mssd"], mspd=bop["mspd"])
            out["bop19"] = dict(ev.evaluate_pose_bop19(config, errs, st.logger), errors=errs)
    return out


def _tables(st, result_file, merge_ranks, merged):
    """the result cache, then every table of `out`, printed and logged in the order of the keys"""
    import copy
    import pickle

    config, store, logger, n_it = st.config, st.store, st.logger, st.n_it
    rt = store["loop", "rt"]
    if result_file:
        with open(result_file, "wb") as f:
            pickle.dump([np.array(rt["rot_err"], dtype=object), np.array(rt["trans_err"], dtype=object), rt["poses_est"], rt["poses_gt"]], f,
                        protocol=2)
    out = {}
    if st.epe is not None:   # :656-660, before the pose tables like the reference
        out["epe"] = st.epe.result(merge_ranks=merge_ranks)
        for line in ("evaluate flow:", "EPE all: {}".format(out["epe"]["epe_all"]), "EPE ignore unvisible: {}".format(out["epe"]["epe_vizbg"]),
                     "EPE visible: {}".format(out["epe"]["epe_viz"])):
            _say(logger, line)
    tables = _pose_tables(st, config, "loop")
    out.update((k, tables[k]) for k in ("pose", "add", "arp_2d"))
    if st.device_eval:
        out["device_eval"] = True
    out.update(_scorer_tables(st, "loop"))
    if "bop19" in out:   # the loop's completes its BOP table; the ICP row's stays next to it
        out["bop"]["bop19"] = out.pop("bop19")
    out["all_rot_err"], out["all_trans_err"] = tables["all_rot_err"], tables["all_trans_err"]
    out["merged_over_ranks"] = merged
    for s in [s for s in ONE_ROW_SETS if s.name in st.on]:
        # one row, as the reference's PRECOMPUTED_ICP branch scores it (tester.py:253-330), which sets config.TEST.test_iter = 1: a copy
        cfg1 = copy.deepcopy(config)
        cfg1.TEST.test_iter = 1
        _say(logger, s.headline.format(*[type(default)(config.TEST.get(key, default)) for key, default in s.keys]))
        out[s.name] = dict(_pose_tables(st, cfg1, s.name), **_scorer_tables(st, s.name))
    if st.with_flow:
        _say(logger, "evaluate pose from flow ({} iterations, {} unweighted, Huber {} px, gate {} px):".format(
            int(config.TEST.FLOW_PNP_ITER), int(config.TEST.FLOW_PNP_WARM), float(config.TEST.FLOW_PNP_HUBER_PX), float(config.TEST.FLOW_PNP_MAX_PX)))
        rows = np.asarray(store["flow_rows"]["stats"], dtype=np.float64).reshape(-1, n_it, 3)
        mean = rows.mean(axis=0) if len(rows) else np.full((n_it, 3), np.nan)
        out["flow_pnp"] = dict(_pose_tables(st, config, "flow_pnp", arp_2d=False), inliers=mean[:, 0].tolist(), rms=mean[:, 1].tolist(),
                               flagged=[int(v) for v in rows[:, :, 2].sum(axis=0)])
        for it in range(n_it):
            _say(logger, "iter {}: {:.1f} weighted points, rms {:.3f} px, {} of {} pairs flagged".format(
                it + 1, mean[it, 0], mean[it, 1], out["flow_pnp"]["flagged"][it], len(rows)))
    if st.n_hyp > 1:
        hyp = store["hyp"]
        best = [c == int(np.argmin(r)) for c, r, u in zip(hyp["choice"], hyp["rot_err"], hyp["undetected"]) if not u]
        out["hyp"] = dict({"num": st.n_hyp}, **hyp.lists)
        out["hyp"]["chosen_is_least_rot_err"] = float(np.mean(best)) if best else float("nan")
        _say(logger, "hypotheses: {} per pair, the chosen one has the least rotation error in {:.1f} % of {} pairs".format(
            st.n_hyp, 100.0 * out["hyp"]["chosen_is_least_rot_err"], len(best)))
    if st.with_coarse:
        out["coarse"] = dict(store["coarse"].lists)
    return out
