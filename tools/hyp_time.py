"""Time of several hypotheses per pair (TEST.HYP_NUM): the captured refine() of P = 16 pairs at N = 1 and at N = 4 (the bench's test
config, 4 iterations), the post-loop stages of N = 4 (render at the last pose, dim_pose_score, dim_hyp_select) replayed from a graph of
their own (the in-graph cost) and launched eagerly (an upper bound: host launch gaps included), the load-time expansion
(dim_hyp_expand, broadcasts and the hypothesis renders), and dim_pose_score alone at B = 64 with the bytes it reads counted from the
actual boxes (rgb: 3 + 3 colour planes and the rendered depth per box pixel).  Device events, alternating rounds, medians.
Prints one JSON line.  usage: hyp_time.py [rounds] [replays per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deepim.config.config import config as cfg, update_config  # noqa: E402
from deepim.core.tester import Predictor, Refiner  # noqa: E402
from deepim.symbols.deepIM_flownet import deepIM_flownet  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
HBM_BPS = 6.29e12
d = "cuda:0"
P, N4 = 16, 4
update_config(os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test.yaml"))
sym = deepIM_flownet()
sym.get_symbol(cfg, is_train=False)
params = sym.init_weights(cfg, {}, {}, seed=0)
models = syn.make_models(seed=2333, n_models=1, subdiv=5)
rm = Render_Py(None, cfg.dataset.class_name, cfg.dataset.INTRINSIC_MATRIX, zNear=cfg.dataset.ZNEAR, zFar=cfg.dataset.ZFAR, meshes=models)
batch = syn.build_device_batch(rm, P, seed=1000, pixel_means=cfg.network.PIXEL_MEANS)
names = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")


def refiner(n):
    cfg.TEST.HYP_NUM = n
    r = Refiner(cfg, Predictor(cfg, params, P * n), rm, P, capture_graph=True)
    r.load(*[batch[k] for k in names])
    r.refine()   # captures
    torch.cuda.synchronize()
    return r


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


r1, r4 = refiner(1), refiner(N4)
cfg.TEST.HYP_NUM = 1
last4 = r4.poses_iter[r4.test_iter - 1]
work = ops.pose_score_workspace(r4.B, 480, 640, d)
score = torch.zeros((r4.B,), device=d)


def score_only():
    ops.pose_score(r4.batch["image_observed"], r4.image_sc, r4.depth_sc, "rgb", 0.02, bbox=r4.bbox_sc, score=score, workspace=work)


r4._select(last4)
torch.cuda.synchronize()
g_post = torch.cuda.CUDAGraph()
with torch.cuda.graph(g_post):
    r4._select(last4)
stages = {"replay_n1": r1.graph.replay, "replay_n4": r4.graph.replay, "post_loop_graph_n4": g_post.replay,
          "post_loop_eager_n4": lambda: r4._select(last4),
          "expand_n4": r4._expand, "score_kernel_b64": score_only}
res = {k: [] for k in stages}
for rd in range(ROUNDS):
    order = list(stages.items())
    for k, fn in (order if rd % 2 == 0 else order[::-1]):
        res[k].append(timed(fn))
torch.cuda.synchronize()
med = {k: float(np.median(v)) for k, v in res.items()}
bb = r4.bbox_sc.cpu().numpy()
box_px = int(sum(max(b[1] - b[0] + 1, 0) * max(b[3] - b[2] + 1, 0) for b in bb))
score_bytes = box_px * 7 * 4
print(json.dumps({
    "pairs": P, "hyp_num": N4, "samples": r4.B, "test_iter": r4.test_iter, "rounds": ROUNDS, "reps_per_round": REPS,
    "replay_n1_ms": round(med["replay_n1"] / 1e3, 3), "replay_n4_ms": round(med["replay_n4"] / 1e3, 3),
    "n4_over_n1": round(med["replay_n4"] / med["replay_n1"], 3),
    "post_loop_graph_n4_us": round(med["post_loop_graph_n4"], 1),
    "post_loop_share_of_n4": round(med["post_loop_graph_n4"] / med["replay_n4"], 4),
    "post_loop_eager_n4_us": round(med["post_loop_eager_n4"], 1),
    "load_expand_n4_us": round(med["expand_n4"], 1), "score_kernel_b64_us": round(med["score_kernel_b64"], 2),
    "score_box_pixels": box_px, "score_bytes": score_bytes, "score_gb_per_s": round(score_bytes / (med["score_kernel_b64"] * 1e-6) / 1e9, 1),
    "score_hbm_roof_us": round(score_bytes / HBM_BPS * 1e6, 2),
    "choice": r4.hyp_choice.cpu().tolist(), "scores": [round(float(x), 4) for x in r4.hyp_score.cpu()],
    "rounds_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))
