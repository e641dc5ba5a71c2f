"""Time of the BOP symmetry-aware pose errors on the device (csrc/bop.hip, TEST.BOP).
One dim_bop_errors call at the LINEMOD size: one class of 5841 points, T x B = 4 x 16 = 64 poses (float32, as the loop leaves them),
with symmetry sets of 1, 2 and 630 transformations (the identity; one discrete symmetry; one discrete times one continuous symmetry
at BOP's step of 0.01).  Device events, alternating rounds, medians.  Next to it lib/utils/pose_error.py's mssd + mspd on the same
points and poses on this host, and the largest difference between the two on the timed poses.
Prints one JSON line.  usage: bop_time.py [rounds] [launches per round] [host poses at 630 symmetries]"""
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
from lib.utils import pose_error as pe  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402
from lib.utils.symmetry import get_symmetry_transformations  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
HOST_POSES = int(sys.argv[3]) if len(sys.argv) > 3 else 4
d = "cuda:0"
NPTS, T, B = 5841, 4, 16
FLIP_X = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]
INFO = {1: {}, 2: {"symmetries_discrete": [FLIP_X]},
        630: {"symmetries_discrete": [FLIP_X], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}

rng = np.random.default_rng(0)
pts = rng.uniform(-0.05, 0.05, size=(NPTS, 3)) * np.array([1.0, 0.8, 0.6])
_, gt, init = syn.sample_pairs(7, B)
gt = gt.astype(np.float64)
est = np.stack([syn.sample_pairs(8 + t, B)[2] for t in range(T)]).astype(np.float32)
est[..., 3] = gt[None, :, :, 3] + rng.normal(size=(T, B, 3)) * 0.01   # near the ground truth's place, any rotation
K = np.asarray(syn.LINEMOD_K, np.float64)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
points_d, off_d = dev(pts), dev(np.array([0, NPTS], np.int32))
cls_d, est_d, gt_d = torch.zeros((B,), dtype=torch.int32, device=d), dev(est), dev(gt)
sets = {n: get_symmetry_transformations(info, 0.01) for n, info in INFO.items()}
assert all(len(s) == n for n, s in sets.items())
sym_d = {n: (dev(s), dev(np.array([0, n], np.int32))) for n, s in sets.items()}
work = {n: ops.bop_errors_workspace(T, B, n, d) for n in sets}
errors = torch.zeros((T, B, 2), dtype=torch.float64, device=d)
best = torch.zeros((T, B, 2), dtype=torch.int32, device=d)


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


stages = {n: (lambda n=n: ops.bop_errors(points_d, off_d, sym_d[n][0], sym_d[n][1], cls_d, est_d, gt_d, K, n, errors=errors,
                                         best_sym=best, workspace=work[n])) for n in sets}
res = {n: [] for n in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for n, fn in (order if rd % 2 == 0 else order[::-1]):
        res[n].append(timed(fn))
med = {n: float(np.median(v)) for n, v in res.items()}

host_ms, diff = {}, {}
for n, s in sets.items():
    stages[n]()
    got = errors.cpu().numpy()
    ms, worst = [], [0.0, 0.0]
    for b in range(HOST_POSES if n == 630 else min(B, 8)):
        e, g = est[0, b].astype(np.float64), gt[b]
        t0 = time.perf_counter()
        v = (pe.mssd(e[:, :3], e[:, 3], g[:, :3], g[:, 3], pts, s), pe.mspd(e[:, :3], e[:, 3], g[:, :3], g[:, 3], K, pts, s))
        ms.append((time.perf_counter() - t0) * 1e3)
        worst = [max(w, abs(a - c)) for w, a, c in zip(worst, v, got[0, b])]
    host_ms[n], diff[n] = float(np.median(ms)), worst

pairs630 = T * B * 630 * NPTS
print(json.dumps({
    "points": NPTS, "poses": T * B, "rounds": ROUNDS, "launches_per_round": REPS,
    "bop_errors_us": {str(n): round(v, 1) for n, v in med.items()},
    "us_per_pose": {str(n): round(v / (T * B), 2) for n, v in med.items()},
    "point_pairs_630": pairs630, "point_pairs_per_s_630": round(pairs630 / (med[630] * 1e-6), -9),
    "host_mssd_mspd_ms_per_pose": {str(n): round(v, 3) for n, v in host_ms.items()},
    "host_ms_per_batch_of_64_poses": {str(n): round(v * T * B, 1) for n, v in host_ms.items()},
    "host_over_device_per_pose": {str(n): round(host_ms[n] * 1e3 / (med[n] / (T * B)), 1) for n in med},
    "max_abs_diff_vs_host_mssd_mspd": {str(n): [float(x) for x in v] for n, v in diff.items()},
    "rounds_us": {str(n): [round(x, 1) for x in v] for n, v in res.items()}}))
