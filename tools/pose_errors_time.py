"""Time of the device-side pose errors (csrc/metrics.hip, TEST.DEVICE_EVAL).
(1) dim_pose_errors at the LINEMOD size: one class of 5841 points, T x B = 4 x 16 = 64 poses (float32, as the loop leaves them), once
    with the ADD-S flag (symmetric class: 64 x 5841^2 = 2.2e9 distance evaluations) and once without (ADD, arp_2d, re, te only).
    Device events, alternating rounds, medians.  Next to it lib/utils/pose_error.py's adi / add / arp_2d on the same points, per pose
    on this host (the numbers the device path replaces), and the largest difference between the two on the timed poses.
(2) pred_eval wall time (perf_counter around the call, device synchronised) of a fixed synthetic run -- classes ape + glue, 32 pairs
    in batches of 16, the shipped 4-iteration test config, captured graph -- with TEST.DEVICE_EVAL off and on in the same process,
    alternating, after one warm-up of each.
Prints one JSON line.  usage: pose_errors_time.py [rounds] [launches per round] [pred_eval rounds]"""
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
NPTS, T, B = 5841, 4, 16
HOST_POSES = 8

# ------------------------------------------------------------------------------------------------------------------ (1) the kernel
rng = np.random.default_rng(0)
pts = rng.uniform(-0.05, 0.05, size=(NPTS, 3)) * np.array([1.0, 0.8, 0.6])
_, gt, init = syn.sample_pairs(7, B)
gt = gt.astype(np.float64)
est = np.stack([syn.sample_pairs(8 + t, B)[2] for t in range(T)]).astype(np.float32)
est[..., 3] = gt[None, :, :, 3] + rng.normal(size=(T, B, 3)) * 0.01   # near the ground truth's place, any rotation
K = np.asarray(syn.LINEMOD_K, np.float64)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
points_d, off_d = dev(pts), dev(np.array([0, NPTS], np.int32))
flags_d = {"adi": dev(np.array([ops.POSE_ERR_ADI], np.int32)), "add": dev(np.array([0], np.int32))}
cls_d, est_d, gt_d = torch.zeros((B,), dtype=torch.int32, device=d), dev(est), dev(gt)
work = ops.pose_errors_workspace(T, B, NPTS, d)
errors = torch.zeros((T, B, 5), dtype=torch.float64, device=d)


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


stages = {k: (lambda f=f: ops.pose_errors(points_d, off_d, f, cls_d, est_d, gt_d, K, errors=errors, workspace=work))
          for k, f in flags_d.items()}
res = {k: [] for k in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for k, fn in (order if rd % 2 == 0 else order[::-1]):
        res[k].append(timed(fn))
med = {k: float(np.median(v)) for k, v in res.items()}
stages["adi"]()
got = errors.cpu().numpy()

host = {"adi": [], "add": [], "arp_2d": []}
diff = {"adi": 0.0, "add": 0.0, "arp_2d": 0.0}
for b in range(HOST_POSES):
    e, g = est[0, b].astype(np.float64), gt[b]
    for name, col, fn in (("adi", 3, lambda: pe.adi(e[:, :3], e[:, 3], g[:, :3], g[:, 3], pts)),
                          ("add", 2, lambda: pe.add(e[:, :3], e[:, 3], g[:, :3], g[:, 3], pts)),
                          ("arp_2d", 4, lambda: pe.arp_2d(e[:, :3], e[:, 3], g[:, :3], g[:, 3], pts, K))):
        t0 = time.perf_counter()
        v = fn()
        host[name].append((time.perf_counter() - t0) * 1e3)
        diff[name] = max(diff[name], abs(v - got[0, b, col]))
host_ms = {k: float(np.median(v)) for k, v in host.items()}

# ------------------------------------------------------------------------------------------------------------------ (2) pred_eval
update_config(os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test.yaml"))
cfg.dataset.class_name = ["ape", "glue"]
P, PAIRS = 16, 32
sym = deepIM_flownet()
sym.get_symbol(cfg, is_train=False)
params = sym.init_weights(cfg, {}, {}, seed=0)
data = SyntheticPairs(cfg, PAIRS, P, subdiv=5)
ev = data.evaluator()
ref = Refiner(cfg, Predictor(cfg, params, P), data.render_machine, P, capture_graph=True)
batches = list(data.test_batches())
devnull = open(os.devnull, "w")


def eval_wall(flag):
    cfg.TEST.DEVICE_EVAL = flag
    torch.cuda.synchronize()
    stdout, sys.stdout = sys.stdout, devnull   # the tables' printed lines are the same either way
    try:
        t0 = time.perf_counter()
        out = pred_eval(cfg, ref, batches, ev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    finally:
        sys.stdout = stdout


wall = {False: [], True: []}
outs = {}
for flag in (False, True):
    eval_wall(flag)   # warm-up: graph capture, the resident tables, allocator
for rd in range(EVAL_ROUNDS):
    for flag in ((False, True) if rd % 2 == 0 else (True, False)):
        ms, outs[flag] = eval_wall(flag)
        wall[flag].append(ms)
cfg.TEST.DEVICE_EVAL = False
t0 = time.perf_counter()
for b in batches:
    ref.load(*[b[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
    ref.refine()
torch.cuda.synchronize()
refine_ms = (time.perf_counter() - t0) * 1e3
same_counts = all(np.array_equal(outs[False][k]["count_correct"][c], outs[True][k]["count_correct"][c])
                  for k in ("add", "arp_2d") for c in outs[False][k]["count_correct"])
err_diff = max(float(np.abs(outs[False][k]["errors"][c] - outs[True][k]["errors"][c]).max())
               for k in ("add", "arp_2d") for c in outs[False][k]["errors"])
n_sym = int(sum(int((b["class_index"] == 1).sum()) for b in batches))
evals = T * B * NPTS * NPTS
print(json.dumps({
    "points": NPTS, "poses": T * B, "rounds": ROUNDS, "launches_per_round": REPS,
    "pose_errors_adi_us": round(med["adi"], 1), "pose_errors_no_adi_us": round(med["add"], 1),
    "adi_us_per_pose": round(med["adi"] / (T * B), 2), "adi_distance_evals": evals,
    "adi_evals_per_s": round(evals / (med["adi"] * 1e-6), -9),
    "host_adi_ms_per_pose": round(host_ms["adi"], 3), "host_add_ms_per_pose": round(host_ms["add"], 4),
    "host_arp_2d_ms_per_pose": round(host_ms["arp_2d"], 4), "host_poses_timed": HOST_POSES,
    "host_adi_over_device_per_pose": round(host_ms["adi"] * 1e3 / (med["adi"] / (T * B)), 1),
    "max_abs_diff_vs_host": {k: float(v) for k, v in diff.items()},
    "pred_eval": {"pairs": PAIRS, "batch": P, "test_iter": int(cfg.TEST.test_iter), "classes": list(cfg.dataset.class_name),
                  "points_per_class": [int(len(ev._points[c])) for c in ev.classes], "symmetric_pairs": n_sym,
                  "wall_off_ms": round(float(np.median(wall[False])), 1), "wall_on_ms": round(float(np.median(wall[True])), 1),
                  "off_over_on": round(float(np.median(wall[False]) / np.median(wall[True])), 2),
                  "load_and_refine_only_ms": round(refine_ms, 1),
                  "rounds_off_ms": [round(x, 1) for x in wall[False]], "rounds_on_ms": [round(x, 1) for x in wall[True]],
                  "count_correct_equal": bool(same_counts), "max_abs_error_diff": err_diff},
    "rounds_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))
