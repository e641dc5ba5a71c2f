"""Time of the device-side visible surface discrepancy (csrc/vsd.hip, TEST.VSD).
(1) The VSD stage of one batch at the shipped test size: 16 pairs x 4 iterations at 480 x 640 on the synthetic meshes -- its renders
    (the ground truth once, depth and box only; one estimate per iteration into one plane) and dim_vsd_errors (all 4 sets in one call:
    the three planes read once per set), with the render boxes and without.  Device events, alternating rounds, medians; the bytes
    the kernel reads (whole planes, and the rows of the box union) against the time.  Next to it lib/utils/pose_error.py vsd on the
    same planes, per pose on this host, and whether the two agree.
(2) pred_eval wall time (perf_counter around the call, device synchronised) of a fixed synthetic run -- classes ape + glue, 32 pairs in
    batches of 16, the shipped 4-iteration test config, captured graph -- with TEST.VSD off and on in the same process, alternating,
    after one warm-up of each.
Prints one JSON line.  usage: vsd_time.py [rounds] [launches per round] [pred_eval rounds]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deepim.config.config import config as cfg, update_config  # noqa: E402
from deepim.core.tester import Predictor, Refiner, pred_eval  # noqa: E402
from deepim.symbols.deepIM_flownet import deepIM_flownet  # noqa: E402
from lib.dataset.synthetic_pairs import SyntheticPairs  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.utils import pose_error as pe  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
EVAL_ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
d = "cuda:0"
T, B, H, W = 4, 16, 480, 640
HOST_POSES = 4
DELTA, TAUS = 0.015, [0.02]

update_config(os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test.yaml"))
cfg.dataset.class_name = ["ape", "glue"]
cfg.TEST.VSD = True   # the synthetic batches carry depth_observed
data = SyntheticPairs(cfg, 32, B, subdiv=5)
rm = data.render_machine
K = np.asarray(rm.K, np.float64)

# ------------------------------------------------------------------------------------------------------------------ (1) the stage
cls, gt, init = syn.sample_pairs(7, B, n_classes=2)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
cls_d, gt_d = dev(np.asarray(cls, np.int32)), dev(gt.astype(np.float32))
est_d = dev(np.stack([syn.perturb_pose(np.random.default_rng(100 * t + b), gt[b], angle_std=4.0 / (t + 1), xy_std=0.004, z_std=0.01)
                      for t in range(T) for b in range(B)]).reshape(T, B, 3, 4).astype(np.float32))
depth_gt = torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
depth_est = torch.zeros((T, B, 1, H, W), dtype=torch.float32, device=d)
box_gt = torch.zeros((B, 4), dtype=torch.int32, device=d)
box_est = torch.zeros((T, B, 4), dtype=torch.int32, device=d)
errors = torch.zeros((T, B, len(TAUS)), dtype=torch.float64, device=d)
counts = torch.zeros((T, B, 4), dtype=torch.int32, device=d)
work = ops.vsd_workspace(T, B, d)


def renders():
    rm.render_batch(cls_d, gt_d, depth=depth_gt, bbox=box_gt, mask_thr=0.0)
    for t in range(T):
        rm.render_batch(cls_d, est_d[t], depth=depth_est[t], bbox=box_est[t], mask_thr=0.0)


renders()
depth_obs = torch.where(depth_gt > 0, depth_gt, torch.full_like(depth_gt, 2.0))   # the object in front of a wall


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def kernel(boxes):
    extra = {"bbox_gt": box_gt, "bbox_est": box_est} if boxes else {}
    return lambda: ops.vsd_errors(depth_obs, depth_gt, depth_est, K, DELTA, TAUS, "step", errors=errors, counts=counts, workspace=work,
                                  **extra)


stages = {"renders": renders, "kernel_boxes": kernel(True), "kernel_whole": kernel(False)}
res = {k: [] for k in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for k, fn in (order if rd % 2 == 0 else order[::-1]):
        res[k].append(timed(fn))
med = {k: float(np.median(v)) for k, v in res.items()}
stages["kernel_boxes"]()
got_e, got_n = errors.cpu().numpy(), counts.cpu().numpy()
bg, be = box_gt.cpu().numpy(), box_est.cpu().numpy()
rows = sum(int(x) for x in (max(0, min(max(bg[b, 3], be[t, b, 3]), H - 1) - max(min(bg[b, 2], be[t, b, 2]), 0) + 1) for t in range(T) for b in range(B)))
bytes_whole, bytes_rows = 3 * 4 * T * B * H * W, 3 * 4 * rows * W

host_ms, agree = [], True
obs_h, gt_h, est_h = depth_obs.cpu().numpy(), depth_gt.cpu().numpy(), depth_est.cpu().numpy()
for b in range(HOST_POSES):
    t0 = time.perf_counter()
    e, n = pe.vsd(est_h[0, b, 0], gt_h[b, 0], obs_h[b, 0], K, DELTA, TAUS[0], "step")
    host_ms.append((time.perf_counter() - t0) * 1e3)
    agree = agree and e == got_e[0, b, 0] and list(n) == got_n[0, b, :3].tolist()

# ------------------------------------------------------------------------------------------------------------------ (2) pred_eval
P = B
sym = deepIM_flownet()
sym.get_symbol(cfg, is_train=False)
params = sym.init_weights(cfg, {}, {}, seed=0)
ev = data.evaluator()
ref = Refiner(cfg, Predictor(cfg, params, P), rm, P, capture_graph=True)
batches = list(data.test_batches())
devnull = open(os.devnull, "w")


def eval_wall(flag):
    cfg.TEST.VSD = flag
    torch.cuda.synchronize()
    stdout, sys.stdout = sys.stdout, devnull
    try:
        t0 = time.perf_counter()
        out = pred_eval(cfg, ref, batches, ev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    finally:
        sys.stdout = stdout


wall = {False: [], True: []}
for flag in (False, True):
    eval_wall(flag)   # warm-up: graph capture, allocator
for rd in range(EVAL_ROUNDS):
    for flag in ((False, True) if rd % 2 == 0 else (True, False)):
        wall[flag].append(eval_wall(flag)[0])
cfg.TEST.VSD = False
print(json.dumps({
    "pairs": B, "iterations": T, "image": [H, W], "rounds": ROUNDS, "launches_per_round": REPS,
    "renders_us": round(med["renders"], 1), "kernel_boxes_us": round(med["kernel_boxes"], 1), "kernel_whole_us": round(med["kernel_whole"], 1),
    "stage_us": round(med["renders"] + med["kernel_boxes"], 1),
    "bytes_whole": bytes_whole, "bytes_box_rows": bytes_rows,
    "whole_GBps": round(bytes_whole / med["kernel_whole"] * 1e-3, 1), "box_rows_GBps": round(bytes_rows / med["kernel_boxes"] * 1e-3, 1),
    "host_vsd_ms_per_pose": round(float(np.median(host_ms)), 2), "host_poses_timed": HOST_POSES,
    "host_over_device_per_pose": round(float(np.median(host_ms)) * 1e3 / (med["kernel_boxes"] / (T * B)), 1),
    "host_equals_device": bool(agree),
    "pred_eval": {"pairs": 32, "batch": P, "test_iter": int(cfg.TEST.test_iter),
                  "wall_off_ms": round(float(np.median(wall[False])), 1), "wall_on_ms": round(float(np.median(wall[True])), 1),
                  "rounds_off_ms": [round(x, 1) for x in wall[False]], "rounds_on_ms": [round(x, 1) for x in wall[True]]},
    "rounds_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))
