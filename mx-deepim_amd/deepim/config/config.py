"""Config / flag system with the reference's schema (/root/reference/deepim/config/config.py:11-171).

`config` is a global attribute-dict with the same defaults; `update_config(yaml)` merges an
experiments/deepim/cfgs/*.yaml exactly like the reference: unknown TOP-LEVEL keys raise ValueError
(:170-171), nested keys are merged blindly (:163-164), PIXEL_MEANS / INTRINSIC_MATRIX / trans_means /
trans_stds become numpy arrays (:138-162), SCALES becomes a tuple (:166-167).
"""
from __future__ import print_function, division

import copy

import numpy as np
import yaml


class edict(dict):
    """attribute-access dict (stand-in for easydict.EasyDict, which is not installed here)."""

    def __init__(self, d=None, **kwargs):
        super(edict, self).__init__()
        d = dict(d or {}, **kwargs)
        for k, v in d.items():
            self[k] = v

    def __setitem__(self, k, v):
        if isinstance(v, dict) and not isinstance(v, edict):
            v = edict(v)
        super(edict, self).__setitem__(k, v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __deepcopy__(self, memo):
        return edict({k: copy.deepcopy(v, memo) for k, v in self.items()})


def _defaults():
    c = edict()
    c.ModelNet = False
    c.modelnet_root = "./data/ModelNet/"
    c.MXNET_VERSION = ""
    c.output_path = ""
    c.symbol = ""
    c.SCALES = [(480, 640)]
    c.default = edict(frequent=1000, kvstore="device")
    c.network = edict(
        FIXED_PARAMS=[], PIXEL_MEANS=np.array([0, 0, 0]), pretrained="../model/pretrained_model/flownet", pretrained_epoch=0,
        init_from_flownet=False, skip_initialize=False, INPUT_DEPTH=False, INPUT_MASK=False, PRED_MASK=False, PRED_FLOW=False,
        STANDARD_FLOW_REP=False, TRAIN_ITER=False, TRAIN_ITER_SIZE=1, REGRESSOR_NUM=1, ROT_TYPE="QUAT", ROT_COORD="CAMERA",
        TRANS_LOSS_TYPE="L2")
    c.dataset = edict(
        dataset="LINEMOD_REFINE", dataset_path="./data/LINEMOD_6D/LINEMOD_converted/LINEMOD_refine", image_set="train_ape",
        root_path="./data", test_image_set="val_ape", model_dir="", model_file="./data/ModelNet/render_v1/models.txt",
        pose_file="./data/ModelNet/render_v1/poses.txt", DEPTH_FACTOR=1000, NORMALIZE_FLOW=1.0, NORMALIZE_3D_POINT=0.1,
        INTRINSIC_MATRIX=np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]]), ZNEAR=0.25, ZFAR=6.0,
        class_name_file="", class_name=[], trans_means=np.array([0.0, 0.0, 0.0]), trans_stds=np.array([1.0, 1.0, 1.0]),
        # class name -> its BOP model_info dict (symmetries_discrete / symmetries_continuous, lib/utils/symmetry.py), translations and
        # offsets in the unit of the model points; read by train_iter.SE3_PM_SYM
        SYMMETRIES={},
        # synthetic training pairs (lib/dataset/synthetic_pairs.py): occluding objects per pair, the share of the target that may be
        # hidden (toolkit/LM6d_occ_dsm_3_remove_low_visible.py), LINEMOD light model (toolkit/LM6d_occ_dsm_1_gen_observed_light.py)
        SYN_OCC_OBJECTS=0, SYN_OCC_MAX_RATE=0.85, SYN_LIGHT=False)
    c.TRAIN = edict(
        optimizer="sgd", warmup=False, warmup_lr=0, warmup_step=0, begin_epoch=0, end_epoch=0, lr=0.0001, lr_step="4, 6",
        momentum=0.975, wd=0.0005, model_prefix="deepim", RESUME=False, SHUFFLE=True, BATCH_PAIRS=1, FLOW_WEIGHT_TYPE="all",
        TENSORBOARD_LOG=False, INIT_MASK="box_gt", UPDATE_MASK="box_gt", MASK_DILATE=False, REPLACE_OBSERVED_BG_RATIO=0.0,
        # photometric augmentation of image_observed on the device (dim_augment_observed, lib/utils/augment.py; off = the batches of
        # before): the seed of its own generator (with the epoch and the pair's key), the share of pairs that are touched at all and
        # of those that are blurred, and [lo, hi] ranges ([a, a] pins): Gaussian blur sigma in pixels (radius ceil(3 sigma) <= 7),
        # saturation and contrast factors, brightness shift in grey levels, gain per colour plane (white balance), sensor noise sigma
        # in grey levels; AUG_QUANTIZE rounds the result to whole grey levels, as a camera delivers them
        AUG_OBSERVED=False, AUG_SEED=0, AUG_PROB=0.8, AUG_BLUR_PROB=0.4, AUG_BLUR_SIGMA=[0.5, 2.0], AUG_SATURATION=[0.6, 1.4],
        AUG_CONTRAST=[0.7, 1.3], AUG_BRIGHTNESS=[-30.0, 30.0], AUG_GAIN=[0.9, 1.1], AUG_NOISE_SIGMA=[0.0, 8.0], AUG_QUANTIZE=True)
    c.TEST = edict(BATCH_PAIRS=1, test_epoch=0, VISUALIZE=False, test_iter=1, INIT_MASK="box_rendered", UPDATE_MASK="box_rendered",
                   FAST_TEST=False, PRECOMPUTED_ICP=False, BEFORE_ICP=False,
                   # how the zoom window is sampled into the network input (FAST_TEST loop): "bilinear" = one sample per network pixel,
                   # "area" = where the window shrinks the image, the mean of up to ZOOM_AREA_MAX_TAPS (1..8) sub-samples per axis
                   ZOOM_FILTER="bilinear", ZOOM_AREA_MAX_TAPS=4,
                   ICP_ITER=0, ICP_MAX_DIST=0.02,   # depth ICP after the loop: iterations (0 = off), gate in metres
                   # photometric polish after the loop (dim_photo_refine; a polish of a pose within a few degrees, not a tracker):
                   # Gauss-Newton iterations per pyramid level (0 = off), pyramid levels (1..5), the Huber knee and the hard gate in
                   # units of the channel sum (three times a gray level), one gain and bias per pair
                   PHOTO_ITER=0, PHOTO_LEVELS=3, PHOTO_HUBER=30.0, PHOTO_MAX=180.0, PHOTO_GAIN=True,
                   # silhouette polish after the loop (dim_sil_refine; for textureless objects, a polish of a pose within a few degrees and
                   # pixels): Gauss-Newton iterations per round (0 = off), rounds (1..8; each renders the contour again at its pose), the
                   # Huber knee and the hard gate in pixels (the edge field reaches ceil(SIL_MAX_PX) <= 64 pixels), and the mask whose
                   # edge the contour is pulled onto: "observed" = the mask_observed handed to load(), "pred" = the mask head's last output
                   SIL_ITER=0, SIL_ROUNDS=2, SIL_HUBER_PX=2.0, SIL_MAX_PX=12.0, SIL_MASK="observed",
                   # pose from the flow head's output at every loop iteration (dim_flow_pnp; needs PRED_FLOW and the full graph):
                   # Gauss-Newton iterations (0 = off), how many of them are unweighted, the Huber knee and the hard gate (pixels)
                   FLOW_PNP_ITER=0, FLOW_PNP_WARM=2, FLOW_PNP_HUBER_PX=2.0, FLOW_PNP_MAX_PX=8.0,
                   # several starting poses per pair, scored after the loop (1 = off): rotation of the generated ones (degrees), the
                   # score ("rgb" ZNCC or "depth" inlier fraction) and the depth score's inlier gate (metres)
                   HYP_NUM=1, HYP_ROT_DEG=30.0, HYP_SCORE="rgb", HYP_DEPTH_TAU=0.02,
                   # starting poses from a detection box per pair (Refiner.load(..., det_boxes=); 0 views = off): a grid of COARSE_VIEWS
                   # viewpoints x COARSE_INPLANE in-plane turns, the iterations and the starting distance (metres) of the box fit, the
                   # score of the candidates ("rgb" / "depth" and its gate, as HYP_SCORE) and how many are rendered at a time; the
                   # HYP_NUM best of every pair start the loop
                   COARSE_VIEWS=0, COARSE_INPLANE=1, COARSE_BOX_ITER=8, COARSE_Z_INIT=1.0, COARSE_SCORE="rgb", COARSE_DEPTH_TAU=0.02,
                   COARSE_CHUNK=256,
                   # one object seen by several calibrated cameras (deepim/core/views.py, deepim/multiview.py): VIEWS = V > 1 makes a
                   # batch hold batch / V groups of V views (Refiner.load(..., cam_T_rig=)); after the per-sample loop the best view
                   # of a group by VIEWS_SCORE ("rgb" ZNCC or "depth" inlier fraction with HYP_DEPTH_TAU's gate) gives the group's pose
                   # and the post-loop stages refine ONE pose per group from all its views.  1 = off
                   VIEWS=1, VIEWS_SCORE="rgb",
                   # the rig's extrinsics refined with the object poses after the consensus (depth ICP terms, needs VIEWS > 1 and
                   # depth_observed; camera 0 is the gauge): VIEWS_CALIB_ITER iterations (0 = off), gate in metres (None = ICP_MAX_DIST).
                   # The later joint stages use the calibrated extrinsics; Refiner.cam_T_rig_calib holds them
                   VIEWS_CALIB_ITER=0, VIEWS_CALIB_MAX_DIST=None,
                   # following objects through a video (deepim/core/tracker.py Tracker, deepim/track.py): the motion model that
                   # predicts a frame's starting pose from the last two accepted ones ("hold" or "velocity") and its damping in
                   # [0, 1]; the lost test -- the window length in frames (1..64) and the window means of the loop's last step
                   # (degrees, metres) above which a track counts as lost; an optional score of the tracked pose against the frame
                   # ("none", "rgb" ZNCC or "depth" inlier fraction with its gate in metres, as HYP_SCORE) and the score below which
                   # the track is lost; and the pose a track keeps ("loop", "icp" or "photo": the named stage must be on).  The
                   # three thresholds TRACK_LOST_ROT_DEG, TRACK_LOST_TRANS and TRACK_MIN_SCORE are starting values that nobody has
                   # tuned on real video
                   TRACK_MOTION="velocity", TRACK_DAMPING=1.0, TRACK_WINDOW=10, TRACK_LOST_ROT_DEG=10.0, TRACK_LOST_TRANS=0.01,
                   TRACK_SCORE="none", TRACK_MIN_SCORE=0.5, TRACK_DEPTH_TAU=0.02, TRACK_POSE="loop",
                   # occlusion reasoning of the tracker ("none" = off): what may hide a track's render -- the other "tracks", the
                   # frame's own "depth" (needs depth frames) or "both" -- by more than TRACK_OCC_DELTA metres (VSD_DELTA's default);
                   # the score then counts the visible pixels only, and a track of which less than TRACK_MIN_VISIBLE of the drawn
                   # pixels are visible is occluded, not lost: it coasts on the motion model for at most TRACK_MAX_OCCLUDED frames in
                   # a row.  These two are starting values that nobody has tuned on real video either
                   TRACK_OCCLUSION="none", TRACK_OCC_DELTA=0.015, TRACK_MIN_VISIBLE=0.3, TRACK_MAX_OCCLUDED=30,
                   # a segmentation of every frame for the tracker ("none" = off, "color": per-track foreground / background colour
                   # histograms carried from frame to frame, dim_track_seg_mask / dim_track_seg_learn): colour bits per channel
                   # (1..5), the margin in pixels by which a render's box is grown into the region that is segmented and learnt
                   # from, the radius of the majority filter (0..4), the rate at which a frame's histograms are blended into the
                   # model, and the fewest pixels of either class for an update.  With it TEST.SIL_ITER > 0 works in a Tracker
                   # (SIL_MASK "observed": the tracker writes the mask) and TRACK_POSE may be "sil".  Rate, margin and radius are
                   # starting values that nobody has tuned on real video
                   TRACK_SEG="none", TRACK_SEG_BITS=5, TRACK_SEG_MARGIN=16, TRACK_SEG_SMOOTH=2, TRACK_SEG_RATE=0.1,
                   TRACK_SEG_MIN_PIXELS=64,
                   # pred_eval: the pose errors (re, te, ADD, ADD-S, arp_2d) from dim_pose_errors on the device instead of
                   # lib/utils/pose_error.py on the host, one pose at a time
                   DEVICE_EVAL=False,
                   # pred_eval: the visible surface discrepancy of every scored pose against depth_observed (dim_vsd_errors): the
                   # visibility tolerance and the misalignment tolerances (metres; up to 8, scored together), the cost ("step" or
                   # "tlinear") and the error below which a pose counts as correct
                   VSD=False, VSD_DELTA=0.015, VSD_TAU=[0.02], VSD_COST="step", VSD_THRESH=0.3,
                   # pred_eval: the BOP symmetry-aware errors MSSD and MSPD of every scored pose (dim_bop_errors) under the symmetry
                   # sets of the evaluator: the discretisation step of continuous symmetries (radians of arc, BOP's
                   # max_sym_disc_step), and the thresholds of correctness -- fractions of the class diameter for MSSD, pixels at a
                   # 640-pixel-wide image (scaled by W / 640) for MSPD
                   BOP=False, BOP_SYM_STEP=0.01, BOP_MSSD_THRESH=[round(0.05 * k, 2) for k in range(1, 11)],
                   BOP_MSPD_THRESH=[5 * k for k in range(1, 11)],
                   # pred_eval with BOP: also the step-cost VSD on BOP's grid (dim_vsd_grid_errors) and with it AR_VSD and
                   # AR = (AR_VSD + AR_MSSD + AR_MSPD) / 3: the visibility tolerance (metres), the misalignment tolerances as
                   # fractions of the class diameter (up to 16), the errors below which a pose counts as correct, and the least
                   # visible fraction of the ground truth at which a pose is a target at all
                   BOP_VSD=False, BOP_VSD_DELTA=0.015, BOP_VSD_TAU=[round(0.05 * k, 2) for k in range(1, 11)],
                   BOP_VSD_THRESH=[round(0.05 * k, 2) for k in range(1, 11)], BOP_MIN_VISIB_FRACT=0.1,
                   # with VISUALIZE (test.py --vis): contour overlays of the ground truth, the initial and the refined pose of every
                   # iteration (deepim/core/visualize.py, dim_vis_overlay): the directory ("" = <output path>/vis), how many of the
                   # first pairs are drawn (0 = all), the outline's radius (0..3: 2 radius + 1 pixels wide), its alpha (0..256), the
                   # alpha of a fill under the refined outline (0 = none), and whether the frames zoomed to the object are written too
                   # (VIS_ZOOM), and whether each pair's frames / zoomed frames are also assembled into a GIF (--vis_video[_zoom])
                   VIS_DIR="", VIS_MAX_PAIRS=64, VIS_RADIUS=1, VIS_EDGE_ALPHA=256, VIS_FILL_ALPHA=0, VIS_ZOOM=True, VIS_VIDEO=False,
                   VIS_VIDEO_ZOOM=False)
    c.train_iter = edict(SE3_DIST_LOSS=False, LW_ROT=0.0, LW_TRANS=0.0, TRANS_LOSS_TYPE="L2", TRANS_SMOOTH_L1_SCALAR=3.0,
                         SE3_PM_LOSS=False, LW_PM=0.0, SE3_PM_LOSS_TYPE="L1", SE3_PM_SL1_SCALAR=1.0, NUM_3D_SAMPLE=-1, LW_FLOW=0.0,
                         LW_MASK=0.0,
                         # the point-matching loss against the closest of the class's symmetric ground truths (dim_pm_sym_loss_grad;
                         # needs SE3_PM_LOSS) and the discretisation step of continuous symmetries in radians: ceil(pi / 0.1) = 32
                         # rotations per axis (BOP's evaluation step of 0.01 gives 315)
                         SE3_PM_SYM=False, SE3_PM_SYM_STEP=0.1)
    return c


config = _defaults()


def reset_config():
    """restore defaults in place (the reference has no such call; tests need it because `config` is global)."""
    config.clear()
    for k, v in _defaults().items():
        config[k] = v
    return config


def update_config(config_file):
    with open(config_file) as f:
        # reference: yaml.load(f) without a Loader (config.py:131) -- fails on PyYAML >= 6, safe_load is equivalent here
        exp_config = edict(yaml.safe_load(f))
    for k, v in exp_config.items():
        if k not in config:
            raise ValueError("key: {} does not exist in config.py".format(k))
        if isinstance(v, dict):
            if k == "TRAIN":
                if "BBOX_WEIGHTS" in v:
                    v["BBOX_WEIGHTS"] = np.array(v["BBOX_WEIGHTS"])
            elif k == "network":
                if "PIXEL_MEANS" in v:
                    v["PIXEL_MEANS"] = np.array(v["PIXEL_MEANS"])
            elif k == "dataset":
                if "INTRINSIC_MATRIX" in v:
                    v["INTRINSIC_MATRIX"] = np.array(v["INTRINSIC_MATRIX"]).reshape([3, 3]).astype(np.float32)
                if "trans_means" in v:
                    v["trans_means"] = np.array(v["trans_means"]).flatten().astype(np.float32)
                if "trans_stds" in v:
                    v["trans_stds"] = np.array(v["trans_stds"]).flatten().astype(np.float32)
                if "class_name_file" in v and v["class_name_file"] != "":
                    with open(v["class_name_file"]) as cf:
                        v["class_name"] = [line.strip() for line in cf.readlines()]
            for vk, vv in v.items():
                config[k][vk] = vv
        else:
            if k == "SCALES":
                config[k][0] = tuple(v)
            else:
                config[k] = v
    return config
