"""Cost of per-pair camera intrinsics in the rasteriser: a 16-pair render in the refinement loop's shape (image + mask + bbox, no depth
plane) with one K for the batch (dim_raster_render_dirty) against a (B,9) device K with a different camera per pair (dim_raster_render_k).
The two are timed in alternating rounds; prints one JSON line with the median of each and their ratio.
usage: raster_k_time.py [rounds] [renders per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mx-deepim_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
d = "cuda:0"
B = 16
models = syn.make_models(seed=2333, n_models=1, subdiv=5)
rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
cls, gt, init = syn.sample_pairs(5, B, n_classes=1)
ci = torch.from_numpy(cls.astype(np.int32)).to(d)
poses = torch.from_numpy(gt.astype(np.float32)).to(d)
img = torch.empty((B, 3, 480, 640), device=d)
msk = torch.empty((B, 1, 480, 640), device=d)
bbox = torch.zeros((B, 4), dtype=torch.int32, device=d)
pm = syn.plane_means()
# sixteen cameras: fx / fy within +-15 %, principal point within +-20 px of the LINEMOD camera (pair 0 keeps it)
rng = np.random.default_rng(0)
K = np.tile(syn.LINEMOD_K[None], (B, 1, 1)).astype(np.float32)
K[1:, 0, 0] *= rng.uniform(0.85, 1.15, B - 1)
K[1:, 1, 1] *= rng.uniform(0.85, 1.15, B - 1)
K[1:, 0, 2] += rng.uniform(-20, 20, B - 1)
K[1:, 1, 2] += rng.uniform(-20, 20, B - 1)
K_dev = torch.from_numpy(K.reshape(B, 9)).to(d)


def run(per_pair):
    kw = {"K": K_dev} if per_pair else {}
    rm.render_batch(ci, poses, image=img, mask=msk, bbox=bbox, plane_means=pm, **kw)


def timed(per_pair):
    run(per_pair)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        run(per_pair)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3


uni, per = [], []
for r in range(ROUNDS):
    a, b = (timed(False), timed(True)) if r % 2 == 0 else (timed(True), timed(False))[::-1]
    uni.append(a)
    per.append(b)
mu, mp = float(np.median(uni)), float(np.median(per))
print(json.dumps({"B": B, "renders_per_round": N, "rounds": ROUNDS, "uniform_K_us": round(mu, 2), "per_pair_K_us": round(mp, 2),
                  "ratio": round(mp / mu, 4), "uniform_K_rounds_us": [round(x, 1) for x in uni],
                  "per_pair_K_rounds_us": [round(x, 1) for x in per]}))
