"""Time of the silhouette polish after the refinement loop (SilStage.run): 16 pairs, the shipped ape test config (FAST_TEST, 4 loop
iterations) and the stage as cfgs/deepim_hip_LM_ape_test_sil.yaml sets it (2 rounds x 6 iterations, Huber 2 px, gate 12 px), the
segmentation being the render at the ground-truth pose.  Device events, in alternating rounds:
  step_off / step_on   the whole refinement step replayed from its captured hipGraph, without and with the stage, in the same
                       process (the difference is what the stage costs a step)
  stage_eager / stage_graph   the stage alone (the field, then per round a depth render and dim_sil_refine), launched eagerly and
                       replayed from a graph of its own
  field_only / refine_only    dim_sil_edge_field alone and one dim_sil_refine alone, eagerly
Prints one JSON line.  usage: sil_time.py [rounds] [steps per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mx-deepim_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deepim.config.config import config as cfg, reset_config, update_config  # noqa: E402
from deepim.core.tester import Predictor, Refiner  # noqa: E402
from deepim.symbols.deepIM_flownet import deepIM_flownet  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
d = "cuda:0"
B, H, W = 16, 480, 640
reset_config()
update_config(os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test_sil.yaml"))
ITERS, SIL_ROUNDS = int(cfg.TEST.SIL_ITER), int(cfg.TEST.SIL_ROUNDS)
sym = deepIM_flownet()
sym.get_symbol(cfg, is_train=False)
params = sym.init_weights(cfg, {}, {}, seed=0)
models = syn.make_models(seed=2333, n_models=1, subdiv=4)
rm = Render_Py(None, cfg.dataset.class_name, syn.LINEMOD_K, meshes=models)
pred = Predictor(cfg, params, B)
batch = syn.build_device_batch(rm, B, 5, pixel_means=cfg.network.PIXEL_MEANS, device=d,
                               noise=dict(angle_std=2.0, angle_max=6.0, xy_std=0.003, z_std=0.01))
depth_gt = torch.zeros((B, 1, H, W), dtype=torch.float32, device=d)
rm.render_batch(batch["class_index"], batch["pose_gt"], depth=depth_gt, bbox=torch.zeros((B, 4), dtype=torch.int32, device=d), mask_thr=0.0)
batch["mask_observed"] = (depth_gt > 0).to(torch.float32).contiguous()    # the segmentation, in place of the loader's box mask
on = Refiner(cfg, pred, rm, B, capture_graph=True)
cfg.TEST.SIL_ITER = 0
off = Refiner(cfg, pred, rm, B, capture_graph=True)
cfg.TEST.SIL_ITER = ITERS
for r in (off, on):
    r.load(*[batch[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
    r.refine()
torch.cuda.synchronize()
assert torch.equal(off.poses_iter, on.poses_iter)
pose = on.poses_iter[-1].clone()
st = on.stages["sil"]


def field():
    ops.sil_edge_field(st.mask, st.radius, field=st.field)


def refine():
    ops.sil_refine(st.depth, st.field, pose, rm.K, ITERS, st.huber, st.gate, bbox=st.bbox, pose_out=st.pose_round[0], stats=st.stats_round,
                   status=st.status, workspace=st.work)


def stage():
    st.run(on, pose)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3


s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    stage()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    stage()
times = {k: [] for k in ("step_off", "step_on", "stage_eager", "stage_graph", "field_only", "refine_only")}
order = [("step_off", off.graph.replay), ("step_on", on.graph.replay), ("stage_eager", stage), ("stage_graph", g.replay), ("field_only", field),
         ("refine_only", refine)]
for r in range(ROUNDS):
    for tag, fn in (order if r % 2 == 0 else order[::-1]):
        times[tag].append(timed(fn))
on.graph.replay()
torch.cuda.synchronize()
bb = st.bbox.cpu().numpy()
box_px = int(sum(max(b[1] - b[0] + 1, 0) * max(b[3] - b[2] + 1, 0) for b in bb))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({
    "B": B, "rounds_of_the_stage": SIL_ROUNDS, "iters_per_round": ITERS, "radius": st.radius, "steps_per_round": N, "rounds": ROUNDS,
    "status": on.status_sil.cpu().tolist(), "points_first_iter": on.sil_stats[:, 0, 0].cpu().numpy().astype(int).tolist(),
    "points_last_iter": on.sil_stats[:, -1, 0].cpu().numpy().astype(int).tolist(),
    "rms_first_iter": [round(float(x), 3) for x in on.sil_stats[:, 0, 1].cpu()],
    "rms_last_iter": [round(float(x), 3) for x in on.sil_stats[:, -1, 1].cpu()], "box_pixels": box_px,
    "step_off_us": round(med["step_off"], 1), "step_on_us": round(med["step_on"], 1),
    "stage_cost_us": round(med["step_on"] - med["step_off"], 1),
    "stage_share_of_step": round((med["step_on"] - med["step_off"]) / med["step_off"], 4),
    "stage_eager_us": round(med["stage_eager"], 1), "stage_graph_us": round(med["stage_graph"], 1),
    "field_only_eager_us": round(med["field_only"], 1), "refine_only_eager_us": round(med["refine_only"], 1),
    "launches": 3 + SIL_ROUNDS * (2 * ITERS + 1), "renders": SIL_ROUNDS, "workspace_bytes": int(st.work.numel() * 8),
    "rounds_us": {k: [round(x, 1) for x in v] for k, v in times.items()}}))
