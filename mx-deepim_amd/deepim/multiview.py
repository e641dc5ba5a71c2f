"""Multi-view entry point:
    python deepim/multiview.py --cfg experiments/deepim/cfgs/deepim_hip_LM_ape_views.yaml --gpus 0 --num_views 3 --num_objects 4
        [--hold_loop] [--axis_shift_mm 15] [--extrinsic_noise_deg 0.3 --extrinsic_noise_mm 3 --calib_iter 10]
Refines the objects of a seeded synthetic camera rig (lib/dataset/synthetic_views.py: --num_views calibrated cameras on a ring around
--num_objects objects) twice on the same samples -- every camera on its own (a Refiner with TEST.VIEWS 1) and jointly (TEST.VIEWS =
--num_views, deepim/core/views.py) -- and prints, for the consensus and for every post-loop stage that is on, the mean ADD, rotation
and translation error of both, the error along camera 0's optical axis, and the largest disagreement of the views of an object with
the extrinsics, max_b |pose_b - X_b pose_rig| (for the independent result: with the rig pose that view 0 implies); then the time per
batch of both and of the loop alone.
The weights are found as deepim/test.py finds them: `<prefix>-<test_epoch>.params` of the training run, else the seeded
initialisation (stated in the log).  --hold_loop replaces the pose head by one that predicts no motion, so the loop keeps the
starting poses and the table shows the stages alone; --axis_shift_mm starts every view from the ground truth displaced by that many
millimetres along camera 0's optical axis and three pixels sideways (the direction a single camera sees worst), instead of the rig's
own seeded perturbations.
--extrinsic_noise_deg / --extrinsic_noise_mm load the extrinsics of cameras 1 .. V-1 off by a seeded rotation and shift of that size
(camera 0 stays exact); --calib_iter (replaces TEST.VIEWS_CALIB_ITER) adds a third Refiner that refines the rig's extrinsics with the
object poses before the joint stages.  Then the extrinsic error of every camera before and after is printed -- rotation angle,
translation, and the mean displacement of the objects' model points -- and the table and the time per batch with and without the
calibration, timed alternately."""
from __future__ import print_function, division

import _init_paths  # noqa: F401

import argparse
import os
import time

import numpy as np

from deepim.config.config import config, update_config


def parse_args():
    parser = argparse.ArgumentParser(description="Refine objects seen by several calibrated cameras with a DeepIM network")
    parser.add_argument("--cfg", help="experiment configure file name", required=True, type=str)
    args, rest = parser.parse_known_args()
    update_config(args.cfg)
    parser.add_argument("--gpus", help="specify the gpu to be use", required=True, type=str)
    parser.add_argument("--num_views", help="cameras of the rig (replaces TEST.VIEWS)", default=int(config.TEST.VIEWS), type=int)
    parser.add_argument("--num_objects", help="objects in front of it", default=4, type=int)
    parser.add_argument("--subdiv", help="icosphere subdivisions of the synthetic meshes (4 = 5120 triangles)", default=4, type=int)
    parser.add_argument("--hold_loop", help="a pose head that predicts no motion: the stages alone", action="store_true")
    parser.add_argument("--axis_shift_mm", help="start from the ground truth moved along camera 0's axis (mm) and 3 pixels sideways",
                        default=None, type=float)
    parser.add_argument("--extrinsic_noise_deg", help="load cameras 1.. with their extrinsic rotated by this angle (seeded axis)", default=0.0,
                        type=float)
    parser.add_argument("--extrinsic_noise_mm", help="... and shifted by this distance (seeded direction)", default=0.0, type=float)
    parser.add_argument("--calib_iter", help="iterations of the extrinsic calibration (replaces TEST.VIEWS_CALIB_ITER; 0 = off)",
                        default=int(config.TEST.get("VIEWS_CALIB_ITER", 0) or 0), type=int)
    parser.add_argument("--steps", help="timed refine() calls per Refiner", default=10, type=int)
    return parser.parse_args()


def axis_shift_poses(samples, V, shift_m, pixels=3.0):
    """-> (B,3,4) float32: every sample's ground truth displaced, in the rig frame, by shift_m along camera 0's optical axis and by
    `pixels` pixels at the object's distance along camera 0's image x"""
    X, gt = samples["cam_T_rig"].astype(np.float64), samples["pose_gt"].astype(np.float64)
    R0 = X[0][:, :3]
    out = gt.copy()
    for b in range(len(gt)):
        g0 = (b // V) * V
        side = pixels * gt[g0][2, 3] / float(samples["K"][0][0, 0])
        d_rig = R0.T @ np.array([side, 0.0, shift_m])               # the displacement in the rig frame
        out[b][:, 3] += X[b][:, :3] @ d_rig
    return out.astype(np.float32)


def perturb_extrinsics(X, deg, mm, seed=2333):
    """X (V,3,4) -> float32 copy with cameras 1 .. V-1 moved, in their own frame, by a rotation of `deg` degrees about a seeded axis and
    a shift of `mm` millimetres in a seeded direction; camera 0 is kept"""
    def rotation(axis, angle):
        Wx = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        return np.eye(3) + np.sin(angle) * Wx + (1.0 - np.cos(angle)) * (Wx @ Wx)

    rng = np.random.default_rng([int(seed), 97])
    out = np.asarray(X, np.float32).copy()
    for v in range(1, len(out)):
        axis, d = rng.normal(size=3), rng.normal(size=3)
        R = rotation(axis / np.linalg.norm(axis), np.radians(deg))
        Xv = out[v].astype(np.float64)
        out[v] = np.concatenate([R @ Xv[:, :3], (R @ Xv[:, 3] + 1e-3 * mm * d / np.linalg.norm(d))[:, None]], axis=1).astype(np.float32)
    return out


def extrinsic_table(X, X_true, samples, V, models):
    """-> [dict(view, rot_deg, trans, disp)]: per camera the rotation angle and translation of X_v X*_v^-1 and the mean displacement of
    the objects' model points, |X_v T_g m - X*_v T_g m| over the true rig poses T_g"""
    from lib.utils import pose_error

    X, X_true = np.asarray(X, np.float64), np.asarray(X_true, np.float64)
    rig, cls = samples["pose_rig_gt"].astype(np.float64), samples["class_index"]
    rows = []
    for v in range(V):
        disp = []
        for g in range(len(rig)):
            m = models[int(cls[g * V])][0].astype(np.float64) @ rig[g][:, :3].T + rig[g][:, 3]
            disp.append(np.mean(np.linalg.norm((m @ X[v][:, :3].T + X[v][:, 3]) - (m @ X_true[v][:, :3].T + X_true[v][:, 3]), axis=1)))
        chord = np.linalg.norm(X[v][:, :3] - X_true[v][:, :3]) / (2.0 * np.sqrt(2.0))   # sin(angle / 2): exact for small angles too
        rows.append(dict(view=v, rot_deg=float(np.degrees(2.0 * np.arcsin(min(chord, 1.0)))),
                         trans=float(pose_error.te(X[v][:, 3], X_true[v][:, 3])), disp=float(np.mean(disp))))
    return rows


def views_table(names, poses_alone, poses_joint, rigs_joint, samples, V, models):
    """-> [dict(stage, which, add, rot_deg, trans, axis, axis_view, gap)], two rows per pose set; poses_* : {name: (B,3,4)}, rigs_joint:
    {name: (G,3,4)}; axis_view: the error along camera 0's axis per view, the mean over the objects"""
    from lib.utils import pose_error

    X, gt, cls = samples["cam_T_rig"].astype(np.float64), samples["pose_gt"].astype(np.float64), samples["class_index"]
    B = len(gt)
    axis0 = X[0][2, :3]                                              # camera 0's optical axis in the rig frame

    def seen(Xb, T):
        return np.concatenate([Xb[:, :3] @ T[:, :3], (Xb[:, :3] @ T[:, 3] + Xb[:, 3])[:, None]], axis=1)

    def implied_rig(Xb, T):
        return np.concatenate([Xb[:, :3].T @ T[:, :3], (Xb[:, :3].T @ (T[:, 3] - Xb[:, 3]))[:, None]], axis=1)

    rows = []
    for name in names:
        for which, poses in (("independent", poses_alone.get(name)), ("joint", poses_joint[name])):
            if poses is None:
                continue
            p = poses.astype(np.float64)
            adds, res, tes, axs, gaps = [], [], [], [], []
            for b in range(B):
                pts = models[int(cls[b])][0].astype(np.float64)
                adds.append(pose_error.add(p[b][:, :3], p[b][:, 3], gt[b][:, :3], gt[b][:, 3], pts))
                res.append(pose_error.re(p[b][:, :3], gt[b][:, :3]))
                tes.append(pose_error.te(p[b][:, 3], gt[b][:, 3]))
                axs.append(abs(float(axis0 @ (X[b][:, :3].T @ (p[b][:, 3] - gt[b][:, 3])))))
                rig = rigs_joint[name][b // V].astype(np.float64) if which == "joint" else implied_rig(X[(b // V) * V], p[(b // V) * V])
                gaps.append(np.abs(p[b] - seen(X[b], rig)).max())
            rows.append(dict(stage=name, which=which, add=float(np.mean(adds)), rot_deg=float(np.mean(res)), trans=float(np.mean(tes)),
                             axis=float(np.mean(axs)), axis_view=np.asarray(axs).reshape(-1, V).mean(axis=0).tolist(), gap=float(np.max(gaps))))
    return rows


def multiview_deepim(args):
    import torch

    from deepim.core.tester import Predictor, Refiner
    from deepim.symbols import deepIM_flownet as symbols
    from lib.dataset.synthetic_views import SyntheticViews
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
        msg = "{} not found: running with the seeded initialisation (throughput / plumbing run, the loop will not converge)".format(param_file)
        print(msg)
        logger.info(msg)
    arg_params = sym_instance.init_weights(config, arg_params, {}, seed=0)
    if args.hold_loop:
        for k in ("rot_weight", "trans_weight", "trans_bias"):
            arg_params[k] = np.zeros_like(arg_params[k])
        arg_params["rot_bias"] = np.array([1.0, 0.0, 0.0, 0.0] * (arg_params["rot_bias"].size // 4), np.float32).reshape(arg_params["rot_bias"].shape)

    G, V = int(args.num_objects), int(args.num_views)
    B = G * V
    data = SyntheticViews(config, G, V, seed=2333, subdiv=args.subdiv, device=device)
    s = data.samples
    batch = data.batch(pose_init=None if args.axis_shift_mm is None else axis_shift_poses(s, V, 1e-3 * args.axis_shift_mm))
    X_true = s["cam_T_rig"][:V]
    noisy = args.extrinsic_noise_deg > 0 or args.extrinsic_noise_mm > 0
    X_load = perturb_extrinsics(X_true, args.extrinsic_noise_deg, args.extrinsic_noise_mm) if noisy else X_true
    if noisy:   # what load() is given: the ground truth and the observations keep the true rig
        batch["cam_T_rig"] = torch.from_numpy(np.tile(X_load, (G, 1, 1))).to(device)
    predictor = Predictor(config, arg_params, B, device=device)
    stage_keys = {"icp": "ICP_ITER", "photo": "PHOTO_ITER", "sil": "SIL_ITER"}
    on = {k: int(config.TEST.get(v, 0) or 0) for k, v in stage_keys.items()}

    def refiner(views, stages=True, calib_iter=0):
        keep = {v: config.TEST[v] for v in list(stage_keys.values()) + ["VIEWS", "VIEWS_CALIB_ITER"]}
        config.TEST.VIEWS, config.TEST.VIEWS_CALIB_ITER = views, calib_iter
        if not stages:
            for v in stage_keys.values():
                config.TEST[v] = 0
        try:
            return Refiner(config, predictor, data.render_machine, B, capture_graph=True)
        finally:
            config.TEST.update(keep)

    def run(r):
        extra = {"cam_T_rig": batch["cam_T_rig"]} if r.V > 1 else {}
        r.load(batch["image_observed"], batch["image_rendered"], batch["mask_segmentation"], batch["mask_rendered"], batch["src_pose"],
               batch["class_index"], depth_observed=batch["depth_observed"] if r.depth_observed is not None else None, K=batch["K"], **extra)
        r.refine()   # captures the graph
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.steps):
            r.refine()
        torch.cuda.synchronize()
        return (time.time() - t0) / max(args.steps, 1)

    joint, alone, loop = refiner(V), refiner(1), refiner(1, stages=False)
    t_joint, t_alone, t_loop = run(joint), run(alone), run(loop)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    calib = refiner(V, calib_iter=args.calib_iter) if args.calib_iter > 0 else None
    if calib is not None:   # timed alternately with the joint Refiner: two rounds each, the second kept
        for _ in range(2):
            t_calib, t_joint = run(calib), run(joint)
    names = ["loop"] + [k for k in ("icp", "photo", "sil") if on[k] > 0]
    poses_alone = {"loop": host(alone.poses_iter[-1])}
    poses_joint, rigs_joint = {"loop": host(joint.pose_views)}, {"loop": host(joint.pose_rig)}
    for k in names[1:]:
        poses_alone[k] = host(getattr(alone, "pose_" + k))
        poses_joint[k], rigs_joint[k] = host(getattr(joint, "pose_" + k)), host(getattr(joint, "pose_rig_" + k))
    loaded = dict(s, cam_T_rig=np.tile(X_load, (G, 1, 1)))   # the extrinsics the poses of a joint stage agree with
    rows = views_table(names, poses_alone, poses_joint, rigs_joint, loaded, V, data.models)
    print("views chosen by the consensus ({}): {}; status {}".format(joint.views.mode, host(joint.views_choice).tolist(),
                                                                     sorted(set(host(joint.status_views).tolist()))))
    print("stage  result       mean ADD (m)  rot err (deg)  trans err (m)  along cam 0 axis (m)  max |pose - X pose_rig|")
    for r in rows:
        print("{stage:5s}  {which:11s}  {add:12.6f}  {rot_deg:13.4f}  {trans:13.6f}  {axis:20.6f}  {gap:24.3e}".format(**r))
    if args.axis_shift_mm is not None:
        print("error along camera 0's axis per view (mm), the mean over the objects:")
        for r in rows:
            print("{:5s}  {:11s}  {}".format(r["stage"], r["which"], "  ".join("{:8.3f}".format(1e3 * a) for a in r["axis_view"])))
    if noisy or calib is not None:
        print("extrinsics against the true rig: rotation (deg), translation (mm), mean displacement of the objects' model points (mm)")
        tables = [("loaded", extrinsic_table(X_load, X_true, s, V, data.models))]
        if calib is not None:
            tables.append(("calibrated", extrinsic_table(host(calib.cam_T_rig_calib), X_true, s, V, data.models)))
        for what, table in tables:
            for e in table:
                print("{:10s}  camera {:2d}  {:8.4f}  {:8.3f}  {:8.3f}".format(what, e["view"], e["rot_deg"], 1e3 * e["trans"], 1e3 * e["disp"]))
    if calib is not None:
        used = dict(s, cam_T_rig=np.tile(host(calib.cam_T_rig_calib), (G, 1, 1)))
        poses_c, rigs_c = {"loop": host(calib.pose_calib)}, {"loop": host(calib.pose_rig_calib)}
        for k in names[1:]:
            poses_c[k], rigs_c[k] = host(getattr(calib, "pose_" + k)), host(getattr(calib, "pose_rig_" + k))
        print("with the calibration ({} iterations; row 'loop' is the calibration's own poses): status {}".format(
            args.calib_iter, sorted(set(host(calib.status_calib).tolist()))))
        for r in views_table(names, {}, poses_c, rigs_c, used, V, data.models):
            print("{stage:5s}  {which:11s}  {add:12.6f}  {rot_deg:13.4f}  {trans:13.6f}  {axis:20.6f}  {gap:24.3e}".format(**r))
        print("{:.2f} ms per batch with the calibration, {:.2f} ms without (alternating runs)".format(1e3 * t_calib, 1e3 * t_joint))
    print("{} objects x {} views, {} loop iterations on {}: {:.2f} ms per batch jointly, {:.2f} ms independently, {:.2f} ms the loop alone "
          "(graph replays; the stages: {:.2f} ms jointly with the consensus, {:.2f} ms independently)".format(
              G, V, config.TEST.test_iter, device, 1e3 * t_joint, 1e3 * t_alone, 1e3 * t_loop, 1e3 * (t_joint - t_loop), 1e3 * (t_alone - t_loop)))
    return rows, (t_joint, t_alone, t_loop)


def main():
    args = parse_args()
    print(args)
    multiview_deepim(args)


if __name__ == "__main__":
    main()
