"""Time of the photometric polish after the refinement loop (PhotoStage.run): 16 pairs, the shipped ape test config (FAST_TEST, 4 loop
iterations) and the defaults of the stage (3 levels x 4 iterations, Huber 30, gate 180), with device events, in alternating rounds:
  step_off / step_on   the whole refinement step replayed from its captured hipGraph, without and with the stage (the difference is
                       what the stage costs a step; step_off is the step as it is without this feature, measured in the same run)
  stage_eager / stage_graph   the stage alone (render of image + depth + box at the last pose, then dim_photo_refine), launched
                       eagerly and replayed from a graph of its own
  photo_only           dim_photo_refine alone, eagerly
Bytes moved are counted from the planes (render: image + depth written; pyramid pass: 7 planes read, 4 x 4/3 written; statistics: 3
planes over the boxes; each iteration: 4 template planes over the box of its level + 4 gathered observed values per template pixel)
against the HBM roof (6.29 TB/s measured copy rate).  Prints one JSON line.  usage: photo_time.py [rounds] [steps per round]"""
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
HBM_BPS = 6.29e12
d = "cuda:0"
B, H, W = 16, 480, 640
reset_config()
update_config(os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test_photo.yaml"))
LEVELS, ITERS = int(cfg.TEST.PHOTO_LEVELS), int(cfg.TEST.PHOTO_ITER)
sym = deepIM_flownet()
sym.get_symbol(cfg, is_train=False)
params = sym.init_weights(cfg, {}, {}, seed=0)
models = syn.make_models(seed=2333, n_models=1, subdiv=4)
rm = Render_Py(None, cfg.dataset.class_name, syn.LINEMOD_K, meshes=models)
pred = Predictor(cfg, params, B)
batch = syn.build_device_batch(rm, B, 5, pixel_means=cfg.network.PIXEL_MEANS, device=d,
                               noise=dict(angle_std=2.0, angle_max=6.0, xy_std=0.003, z_std=0.01))
on = Refiner(cfg, pred, rm, B, capture_graph=True)
cfg.TEST.PHOTO_ITER = 0
off = Refiner(cfg, pred, rm, B, capture_graph=True)
cfg.TEST.PHOTO_ITER = ITERS
for r in (off, on):
    r.load(*[batch[k] for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose", "class_index")])
    r.refine()
torch.cuda.synchronize()
assert torch.equal(off.poses_iter, on.poses_iter)
pose = on.poses_iter[-1].clone()
st = on.stages["photo"]


def photo():
    ops.photo_refine(on.batch["image_observed"], st.image, st.depth, pose, rm.K, LEVELS, ITERS, st.huber, st.gate, gain=st.gain,
                     bbox=st.bbox, pose_out=st.pose, stats=st.stats, status=st.status, workspace=st.work)


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
times = {k: [] for k in ("step_off", "step_on", "stage_eager", "stage_graph", "photo_only")}
order = [("step_off", off.graph.replay), ("step_on", on.graph.replay), ("stage_eager", stage), ("stage_graph", g.replay), ("photo_only", photo)]
for r in range(ROUNDS):
    for tag, fn in (order if r % 2 == 0 else order[::-1]):
        times[tag].append(timed(fn))
torch.cuda.synchronize()
bb = st.bbox.cpu().numpy()
box_px = int(sum(max(b[1] - b[0] + 1, 0) * max(b[3] - b[2] + 1, 0) for b in bb))
tmpl_px = int((st.depth > 0).sum())
frame = B * H * W * 4
bytes_render = 4 * frame
bytes_pyramid = 7 * frame + 4 * frame + sum(4 * frame // 4 ** (l - 1) + 4 * frame // 4 ** l for l in range(1, LEVELS))
bytes_stats = 3 * box_px * 4
bytes_iters = ITERS * sum((4 * box_px + 4 * tmpl_px) * 4 // 4 ** l for l in range(LEVELS))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({
    "B": B, "levels": LEVELS, "iters_per_level": ITERS, "steps_per_round": N, "rounds": ROUNDS, "status": on.status_photo.cpu().tolist(),
    "points_first_iter": on.photo_stats[:, 0, 0].cpu().numpy().astype(int).tolist(),
    "points_last_iter": on.photo_stats[:, -1, 0].cpu().numpy().astype(int).tolist(), "box_pixels": box_px, "template_pixels": tmpl_px,
    "step_off_us": round(med["step_off"], 1), "step_on_us": round(med["step_on"], 1),
    "stage_share_of_step": round((med["step_on"] - med["step_off"]) / med["step_off"], 4),
    "stage_eager_us": round(med["stage_eager"], 1), "stage_graph_us": round(med["stage_graph"], 1),
    "photo_only_eager_us": round(med["photo_only"], 1), "photo_launches": LEVELS + 2 + 2 * LEVELS * ITERS,
    "workspace_bytes": int(st.work.numel() * 8),
    "bytes_render": bytes_render, "bytes_pyramid": bytes_pyramid, "bytes_stats": bytes_stats, "bytes_iterations": bytes_iters,
    "hbm_roof_us": round((bytes_render + bytes_pyramid + bytes_stats + bytes_iters) / HBM_BPS * 1e6, 2),
    "rounds_us": {k: [round(x, 1) for x in v] for k, v in times.items()}}))
