"""Tracking entry point:
    python deepim/track.py --cfg experiments/deepim/cfgs/deepim_hip_LM_ape_track.yaml --gpus 0 --num_frames 60 --num_objects 3 [--reinit_from_gt]
        [--occluder] [--seg] [--object_colors LO HI] [--background_colors LO HI]
Follows the objects of a seeded synthetic video (lib/dataset/synthetic_sequences.py) with deepim.core.tracker.Tracker and prints, per
object, the frames tracked and lost, the re-initialisations, the mean ADD over the tracked frames and the frames it was occluded
(TEST.TRACK_OCCLUSION on: deepim_hip_LM_ape_track_occ.yaml), and the frames per second.  --occluder puts an untracked object in
front of object 0 for the middle third of the video.  --seg switches the colour-histogram segmentation on (TEST.TRACK_SEG color, and
the silhouette stage with 2 iterations per round when the YAML leaves it off: deepim_hip_LM_ape_track_seg.yaml has both), learns the
colours on frame 0 at its true pose, and adds two columns: the mean IoU of the frame's mask against the silhouette of the ground-truth
render, and the mean ADD of the silhouette stage's pose next to the loop's.  --object_colors / --background_colors restrict the colour
range of the textures and the background (the default world, textures in 40..255 over a background in 0..255, is the hard case).
The weights are found as deepim/test.py finds them: `<prefix>-<test_epoch>.params` of the training run, else the seeded
initialisation (stated in the log).  --reinit_from_gt offers the ground-truth pose to every lost track (stands in for a detector)."""
from __future__ import print_function, division

import _init_paths  # noqa: F401

import argparse
import os
import time

import numpy as np

from deepim.config.config import config, update_config


def parse_args():
    parser = argparse.ArgumentParser(description="Track objects through a synthetic video with a DeepIM network")
    parser.add_argument("--cfg", help="experiment configure file name", required=True, type=str)
    args, rest = parser.parse_known_args()
    update_config(args.cfg)
    parser.add_argument("--gpus", help="specify the gpu to be use", required=True, type=str)
    parser.add_argument("--num_frames", help="frames of the synthetic video", default=60, type=int)
    parser.add_argument("--num_objects", help="objects followed through it", default=3, type=int)
    parser.add_argument("--subdiv", help="icosphere subdivisions of the synthetic meshes (4 = 5120 triangles)", default=4, type=int)
    parser.add_argument("--reinit_from_gt", help="offer the ground-truth pose to every lost track", action="store_true")
    parser.add_argument("--occluder", help="an untracked object 0.35 m in front of object 0 for the middle third of the frames",
                        action="store_true")
    parser.add_argument("--seg", help="colour-histogram segmentation of every frame (TEST.TRACK_SEG color) and the silhouette stage on it",
                        action="store_true")
    parser.add_argument("--object_colors", help="colour range of the object textures, every channel", nargs=2, type=int, metavar=("LO", "HI"))
    parser.add_argument("--background_colors", help="colour range of the background, every channel", nargs=2, type=int, metavar=("LO", "HI"))
    return parser.parse_args()


def mean_add(pose, pose_gt, keep, pts):
    """mean ADD of pose (T,3,4) against pose_gt over the frames in `keep` (nan for none)"""
    from lib.utils import pose_error

    pose, pose_gt = pose.astype(np.float64), pose_gt.astype(np.float64)
    adds = [pose_error.add(pose[t, :, :3], pose[t, :, 3], pose_gt[t, :, :3], pose_gt[t, :, 3], pts) for t in range(len(pose)) if keep[t]]
    return float(np.mean(adds)) if adds else float("nan")


def run_frames(tracker, frames):
    """Tracker.run, recording with a segmentation also the loop's last pose and the silhouette stage's (pose_loop, pose_sil)"""
    import torch

    r, rec = tracker.refiner, {}
    for f in frames:
        out = dict(tracker.step(f["frame_bgr"], f.get("depth_raw"), f.get("reinit_pose"), f.get("reinit_valid")))
        if tracker.seg_on:
            out["pose_loop"], out["pose_sil"] = r.poses_iter[r.test_iter - 1], r.pose_sil
        for k, v in out.items():
            if v is not None:
                rec.setdefault(k, []).append(v.clone())
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


def track_table(out, pose_gt, class_index, models, class_names):
    """-> [dict(object, cls, tracked, lost, reinit, add, occluded)] from Tracker.run's host arrays and the ground truth (T,P,3,4);
    occluded: the frames with DIM_STATUS_TRACK_OCCLUDED (coasting ones count as tracked, with the coasted pose's ADD)"""
    from lib.hip import ops
    from lib.utils import pose_error

    rows = []
    flags, pose = out["flags"], out.get("pose_track", out["pose"]).astype(np.float64)   # the best estimate where there is one
    for p in range(flags.shape[1]):
        lost = (flags[:, p] & ops.STATUS_TRACK_LOST) != 0
        pts = models[int(class_index[p])][0].astype(np.float64)
        adds = [pose_error.add(pose[t, p, :, :3], pose[t, p, :, 3], pose_gt[t, p, :, :3].astype(np.float64), pose_gt[t, p, :, 3].astype(np.float64),
                               pts) for t in range(flags.shape[0]) if not lost[t]]
        rows.append(dict(object=p, cls=class_names[int(class_index[p])], tracked=int((~lost).sum()), lost=int(lost.sum()),
                         reinit=int(((flags[:, p] & ops.STATUS_TRACK_REINIT) != 0).sum()), add=float(np.mean(adds)) if adds else float("nan"),
                         occluded=int(((flags[:, p] & ops.STATUS_TRACK_OCCLUDED) != 0).sum())))
        if "pose_sil" in out:   # the segmentation is on: the loop's pose and the silhouette stage's over the same frames
            rows[-1].update(add_loop=mean_add(out["pose_loop"][:, p], pose_gt[:, p], ~lost, pts),
                            add_sil=mean_add(out["pose_sil"][:, p], pose_gt[:, p], ~lost, pts))
    return rows


def mask_iou(masks, seq):
    """mean over the frames of the IoU of masks (T,P,1,H,W) against the silhouettes of the ground-truth renders -> (P,)"""
    import torch

    rm, d = seq.render_machine, torch.device(seq.device)
    depth = torch.empty((seq.P, 1, seq.height, seq.width), device=d)
    cls = torch.from_numpy(seq.class_index).to(d)
    ious = np.zeros((len(masks), seq.P))
    for t in range(len(masks)):
        rm.render_batch(cls, torch.from_numpy(np.ascontiguousarray(seq.pose_gt[t])).to(d), depth=depth)
        truth, got = depth.cpu().numpy()[:, 0] > 0, masks[t][:, 0] > 0
        union = (truth | got).sum(axis=(1, 2))
        ious[t] = np.where(union > 0, (truth & got).sum(axis=(1, 2)) / np.maximum(union, 1), 1.0)
    return ious.mean(axis=0)


def track_deepim(args):
    import torch

    from deepim.core.tester import Predictor
    from deepim.core.tracker import Tracker
    from deepim.symbols import deepIM_flownet as symbols
    from lib.dataset.synthetic_sequences import SyntheticSequence, sequence_poses
    from lib.utils.create_logger import create_logger
    from lib.utils.load_model import load_param

    dev_id = int(args.gpus.split(",")[0])
    torch.cuda.set_device(dev_id)
    device = "cuda:{}".format(dev_id)
    epoch = config.TEST.test_epoch
    logger, final_output_path = create_logger(config.output_path, args.cfg, config.dataset.test_image_set)
    prefix = os.path.join(final_output_path, "..", "_".join([iset for iset in config.dataset.image_set.split("+")]), config.TRAIN.model_prefix)
    sym_instance = getattr(symbols, config.symbol)()
    sym_instance.get_symbol(config, is_train=False)
    param_file = "%s-%04d.params" % (prefix, epoch)
    if os.path.exists(param_file):
        arg_params, aux_params = load_param(prefix, epoch, process=True)
        print("loaded {}".format(param_file))
    else:
        arg_params = {}
        msg = "{} not found: running with the seeded initialisation (throughput / plumbing run, poses will not converge)".format(param_file)
        print(msg)
        logger.info(msg)
    arg_params = sym_instance.init_weights(config, arg_params, {}, seed=0)

    if args.seg:
        config.TEST.TRACK_SEG = "color"
        if int(config.TEST.get("SIL_ITER", 0) or 0) == 0:
            config.TEST.SIL_ITER = 2
    P, T = args.num_objects, args.num_frames
    events = []
    if args.occluder:   # of object 0's class, centred on it
        cls0 = int(sequence_poses(T, P, 2333, n_classes=len(config.dataset.class_name))[0][0])
        events.append(("occluder", T // 3, 2 * T // 3, 0, 0.35, 0.0, cls0))
    seq = SyntheticSequence(config, T, P, 2333, device=device, events=events, subdiv=args.subdiv, object_colors=args.object_colors,
                            background_colors=args.background_colors)
    predictor = Predictor(config, arg_params, P, device=device)
    tracker = Tracker(config, predictor, seq.render_machine, P, capture_graph=True)
    tracker.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    frames = list(seq.frames(reinit_from_gt=args.reinit_from_gt))   # rendered before the clock starts
    if tracker.seg_on:   # the colour model from frame 0 at its true pose: frame 0 is already segmented
        tracker.learn_colors(frames[0]["frame_bgr"], pose=frames[0]["pose_gt"])
    # the first frame captures the graph: it is tracked, but timed apart
    torch.cuda.synchronize()
    t0 = time.time()
    first = run_frames(tracker, frames[:1])
    t1 = time.time()
    rest = run_frames(tracker, frames[1:]) if T > 1 else None
    t2 = time.time()
    out = first if rest is None else {k: np.concatenate([first[k], rest[k]]) for k in first}
    rows = track_table(out, seq.pose_gt, seq.class_index, seq.models, seq.classes)
    seg_head = seg_row = ""
    if tracker.seg_on:
        for r, iou in zip(rows, mask_iou(out["mask"], seq)):
            r["iou"] = float(iou)
        seg_head, seg_row = "  mask IoU  loop ADD (m)  sil ADD (m)", "  {iou:8.4f}  {add_loop:12.5f}  {add_sil:11.5f}"
    print("object  class  tracked  lost  reinit  mean ADD (m)  occluded" + seg_head)
    for r in rows:
        print(("{object:6d}  {cls:>5s}  {tracked:7d}  {lost:4d}  {reinit:6d}  {add:12.5f}  {occluded:8d}" + seg_row).format(**r))
    fps = (T - 1) / (t2 - t1) if T > 1 else float("nan")
    print("tracked {} objects through {} frames x {} iterations on {}: {:.1f} frames/s after the first frame ({:.2f} s, with the graph "
          "capture)".format(P, T, config.TEST.test_iter, device, fps, t1 - t0))
    return rows, fps


def main():
    args = parse_args()
    print(args)
    track_deepim(args)


if __name__ == "__main__":
    main()
