"""Time of the symmetry-aware point-matching loss (csrc/train.hip: dim_pm_sym_loss_grad, train_iter.SE3_PM_SYM).
One process, device events, alternating rounds, medians:
  kernel     pm_sym_loss_grad at B = 16, N = 3000 with symmetry sets of 1, 32 and 315 transformations (the identity; one continuous
             axis at the training step of 0.1 and at BOP's 0.01), next to pm_loss_grad at the same B, N
  iteration  one forward_backward of the LINEMOD 'ape' training graph at batch 16 with SE3_PM_SYM off and on (32 symmetries)
Prints one JSON line.  usage: pm_sym_time.py [rounds] [launches per round] [iterations per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deepim.config.config import config as cfg, update_config  # noqa: E402
from deepim.core.module import MutableModule  # noqa: E402
from deepim.symbols.deepIM_flownet import deepIM_flownet  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402
from lib.utils.symmetry import symmetry_tables  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
d = "cuda:0"
B, N = 16, 3000
AXIS = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
STEP = {1: None, 32: 0.1, 315: 0.01}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def medians(stages, reps):
    res = {k: [] for k in stages}
    for rd in range(ROUNDS):
        order = list(stages.items())
        for k, fn in (order if rd % 2 == 0 else order[::-1]):
            res[k].append(timed(fn, reps))
    return {k: round(float(np.median(v)), 2) for k, v in res.items()}


update_config(os.path.join(PKG, "experiments/deepim/cfgs/deepim_hip_LM_ape_test.yaml"))
sym = deepIM_flownet()
sym.get_symbol(cfg, True)
params = sym.init_weights(cfg, {}, {}, seed=0)
models = syn.make_models(seed=2333, n_models=1, subdiv=5)
rm = Render_Py(None, cfg.dataset.class_name, cfg.dataset.INTRINSIC_MATRIX, meshes=models)
batch = syn.build_device_train_batch(rm, B, seed=5, models=models, npts=N)
batch["class_index"] = batch["class_index"].to(torch.int32)
name = list(cfg.dataset.class_name)[0]

# ---- the kernel alone, on the batch's own clouds with the estimate a centimetre off the ground truth
p_est = batch["point_cloud_observed"] + 0.01 * torch.randn((B, 3, N), device=d)
grad, loss = torch.empty((B, 3, N), device=d), torch.zeros((1,), device=d)
best = torch.zeros((B,), dtype=torch.int32, device=d)
ti = cfg.train_iter
scale = (cfg.dataset.NORMALIZE_3D_POINT, ti.LW_PM / float(N))
stages = {"pm_loss_grad": lambda: ops.pm_loss_grad(p_est, batch["point_cloud_observed"], batch["point_cloud_weights"], grad, *scale,
                                                   loss_sum=loss)}
for n_sym, step in STEP.items():
    tab, off, max_sym = symmetry_tables([name], {name: AXIS} if step else {}, step or 0.1)
    assert max_sym == n_sym, (max_sym, n_sym)
    tab_d, off_d = torch.as_tensor(tab.astype(np.float32), device=d), torch.as_tensor(off, device=d)
    ws = ops.pm_sym_workspace(B, N, max_sym, d)
    stages["pm_sym_loss_grad S={}".format(n_sym)] = (
        lambda tab_d=tab_d, off_d=off_d, ws=ws, max_sym=max_sym: ops.pm_sym_loss_grad(
            p_est, batch["point_cloud_model"], batch["point_cloud_weights"], batch["tgt_pose"], tab_d, off_d, batch["class_index"], grad,
            *scale, max_sym, loss_sum=loss, best_sym=best, workspace=ws))
out = {"B": B, "N": N, "kernel_us": medians(stages, REPS)}

# ---- one training iteration's forward + backward, feature off and on
mods = {}
for key, on in (("off", False), ("on S=32", True)):
    cfg.train_iter.SE3_PM_SYM, cfg.train_iter.SE3_PM_SYM_STEP = on, 0.1
    mods[key] = MutableModule(cfg, params, B, symmetries={name: AXIS})
cfg.train_iter.SE3_PM_SYM = False
assert mods["on S=32"].pm_max_sym == 32
out["forward_backward_us"] = medians({k: (lambda m=m: m.forward_backward(batch)) for k, m in mods.items()}, ITERS)
fb = out["forward_backward_us"]
out["forward_backward_added_percent"] = round(100.0 * (fb["on S=32"] - fb["off"]) / fb["off"], 3)
print(json.dumps(out))
