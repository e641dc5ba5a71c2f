"""Time of the scene composition kernel (csrc/scene.hip) and of the training-batch builder with and without occluders.
One dim_scene_compose for N = 16 scenes of S = 4 layers at 480x640 (rendered synthetic objects, ~5 % coverage each), every output
asked for; device events, medians of rounds of launches.  Bytes it must move: N*H*W*(4*S + 12 + 20) (S depths and the winner's colour
read; colour, depth and label written) -- the S visibility masks add N*H*W*4*S, reported separately.  Next to it one
build_device_train_batch of 16 pairs with 0 and with 3 occluders (wall clock around a synchronize: it is host-driven).
Prints one JSON line.  usage: scene_time.py [rounds] [launches per round]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
d = "cuda:0"
N, S, H, W = 16, 4, 480, 640

models = syn.make_models(seed=2333, n_models=4, subdiv=4)
rm = Render_Py(None, ["c{}".format(i) for i in range(4)], syn.LINEMOD_K, meshes=models)
cls, gt, _ = syn.sample_pairs(1000, N, n_classes=4)
dc, dp = syn.sample_distractors(1029, cls, gt, models, S - 1, n_classes=4)
lc = np.concatenate([cls.reshape(N, 1), dc], axis=1).reshape(N * S).astype(np.int32)
lp = np.concatenate([gt.reshape(N, 1, 3, 4), dp], axis=1).reshape(N * S, 3, 4).astype(np.float32)
cls_l, pose_l = torch.from_numpy(lc).to(d), torch.from_numpy(lp).to(d)
layer_bgr = torch.empty((N * S, H, W, 3), device=d)
layer_depth = torch.empty((N * S, 1, H, W), device=d)
rm.render_batch(cls_l, pose_l, bgr=layer_bgr, depth=layer_depth)
label = cls_l + 1
out = dict(scene_bgr=torch.empty((N, H, W, 3), device=d), scene_depth=torch.empty((N, 1, H, W), device=d),
           scene_label=torch.empty((N, 1, H, W), device=d), vis_mask=torch.empty((N * S, 1, H, W), device=d),
           counts=torch.empty((N * S, 2), dtype=torch.int32, device=d), vis_bbox=torch.empty((N * S, 4), dtype=torch.int32, device=d))
ws = ops.scene_compose_workspace(N, S, H, W, d)
no_mask = {k: v for k, v in out.items() if k != "vis_mask"}


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


stages = {"all_outputs": lambda: ops.scene_compose(layer_bgr, layer_depth, label, S, workspace=ws, **out),
          "no_vis_mask": lambda: ops.scene_compose(layer_bgr, layer_depth, label, S, workspace=ws, **no_mask)}
res = {k: [] for k in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for k, fn in (order if rd % 2 == 0 else order[::-1]):
        res[k].append(timed(fn))
med = {k: float(np.median(v)) for k, v in res.items()}
cnt = out["counts"].cpu().numpy().reshape(N, S, 2)


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


build = {str(k): wall(lambda k=k: syn.build_device_train_batch(rm, N, 7, models, n_classes=4, occluders=k)) for k in (0, 3)}
base = N * H * W * (4 * S + 12 + 20)
masks = N * H * W * 4 * S
print(json.dumps({
    "N": N, "S": S, "H": H, "W": W, "rounds": ROUNDS, "launches_per_round": REPS,
    "compose_us": {k: round(v, 1) for k, v in med.items()}, "rounds_us": {k: [round(x, 1) for x in v] for k, v in res.items()},
    "bytes_must_move": base, "bytes_vis_masks": masks,
    "TBps_no_vis_mask": round(base / (med["no_vis_mask"] * 1e-6) / 1e12, 3),
    "TBps_all_outputs": round((base + masks) / (med["all_outputs"] * 1e-6) / 1e12, 3),
    "target_visible_share_median": round(float(np.median(cnt[:, 0, 1] / np.maximum(cnt[:, 0, 0], 1))), 3),
    "build_device_train_batch_ms": {k: round(v, 2) for k, v in build.items()}}))
