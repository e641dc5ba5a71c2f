"""Time of the observed-image augmentation kernel (csrc/augment.hip) next to a plain copy of the same blob.
One dim_augment_observed over image_observed (16, 3, 480, 640) with the whole colour chain, noise and rounding on, every pair at blur
radius 0, at radius 2 (sigma 0.5) and at radius 7 (sigma 2.33), and with every pair off (the copy path of the kernel); next to it
dim_copy_words of the same blob, which moves the same compulsory bytes (59 MB read, 59 MB written).  Device events, medians of rounds
of launches, the stages in alternating order.  Prints one JSON line.  usage: augment_time.py [rounds] [launches per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.utils.augment import AugmentParams, blur_taps  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
d = "cuda:0"
B, H, W = 16, 480, 640
MEANS = np.array([103.939, 116.779, 123.68], dtype=np.float32)

g = torch.Generator(device=d)
g.manual_seed(0)
x = torch.randint(0, 256, (B, 3, H, W), generator=g, device=d).float() - torch.from_numpy(MEANS[::-1].copy()).to(d).view(1, 3, 1, 1)
y = torch.empty_like(x)


def params(sigma, on=1):
    p = AugmentParams(B)
    p.on[:] = on
    for b in range(B):
        p.radius[b], p.taps[b] = blur_taps(sigma)
        p.chain[b] = [0.7 + 0.04 * b, 0.8 + 0.03 * b, -20.0 + 2.5 * b, 0.93, 1.0, 1.08, 1.0 + 0.4 * b]
        p.seed[b] = 1000003 * (b + 1)
    return p, p.to_device(d)


def stage(sigma, on=1):
    p, t = params(sigma, on)
    return lambda: ops.augment_observed(x, t["on"], p.radius, t["taps"], t["chain"], t["seed"], MEANS, quantize=True, out=y)


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


stages = {"copy_words": lambda: ops.copy(y, x), "augment_off": stage(0.0, on=0), "augment_r0": stage(0.0), "augment_r2": stage(0.5),
          "augment_r7": stage(2.33)}
res = {k: [] for k in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for k, fn in (order if rd % 2 == 0 else order[::-1]):
        res[k].append(timed(fn))
med = {k: float(np.median(v)) for k, v in res.items()}
nbytes = 2 * x.numel() * 4
print(json.dumps({"B": B, "H": H, "W": W, "rounds": ROUNDS, "launches_per_round": REPS, "us": {k: round(v, 1) for k, v in med.items()},
                  "rounds_us": {k: [round(v, 1) for v in vs] for k, vs in res.items()}, "bytes_must_move": nbytes,
                  "TBps": {k: round(nbytes / (v * 1e-6) / 1e12, 3) for k, v in med.items()},
                  "over_copy": {k: round(v / med["copy_words"], 2) for k, v in med.items()}}))
