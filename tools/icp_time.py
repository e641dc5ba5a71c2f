"""Time of the depth ICP stage after the refinement loop (IcpStage.run): 16 pairs, TEST.ICP_ITER = 10, the depth + bbox render at the
loop's last pose followed by dim_icp_refine, with device events -- eagerly and replayed from a captured hipGraph -- and the ICP launches
alone.  Bytes moved are counted from the actual boxes (render: the depth plane written; each iteration: the box of the rendered depth
read + 5 gathered observed depths per source pixel) against the HBM roof (6.29 TB/s measured copy rate, MI355X_MICROARCH.md).
Prints one JSON line.  usage: icp_time.py [rounds] [stages per round]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mx-deepim_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
HBM_BPS = 6.29e12
d = "cuda:0"
B, H, W, ITERS, MAX_DIST = 16, 480, 640, 10, 0.02
models = syn.make_models(seed=2333, n_models=1, subdiv=4)
rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
cls, gt, init = syn.sample_pairs(5, B, angle_std=2.0, angle_max=6.0, xy_std=0.003, z_std=0.01)
ci = torch.zeros((B,), dtype=torch.int32, device=d)
pose = torch.from_numpy(init).to(d)
depth_obs = torch.empty((B, 1, H, W), device=d)
rm.render_batch(ci, torch.from_numpy(gt).to(d), depth=depth_obs, mask_thr=0.0)
depth_obs = torch.where(depth_obs > 0, depth_obs, torch.full_like(depth_obs, 1.5)).contiguous()   # object in front of a wall
depth_r = torch.zeros((B, 1, H, W), device=d)
bbox = torch.zeros((B, 4), dtype=torch.int32, device=d)
status = torch.zeros((B,), dtype=torch.int32, device=d)
stats = torch.zeros((B, ITERS, 2), device=d)
pose_out = torch.zeros((B, 3, 4), device=d)
work = ops.icp_workspace(B, H, W, d)


def icp():
    ops.icp_refine(depth_r, depth_obs, pose, rm.K, ITERS, MAX_DIST, bbox=bbox, pose_out=pose_out, stats=stats, status=status, workspace=work)


def stage():
    ops.fill(status, 0)
    rm.render_batch(ci, pose, depth=depth_r, bbox=bbox, mask_thr=0.0, status=status)
    icp()


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


rm.reserve(B)
stage()
torch.cuda.synchronize()
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    stage()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    stage()
eager, graph, alone = [], [], []
for r in range(ROUNDS):
    order = [("e", stage), ("g", g.replay), ("i", icp)]
    for tag, fn in (order if r % 2 == 0 else order[::-1]):
        {"e": eager, "g": graph, "i": alone}[tag].append(timed(fn))
torch.cuda.synchronize()
bb = bbox.cpu().numpy()
dr = depth_r.cpu().numpy()[:, 0]
box_px = int(sum(max(b[1] - b[0] + 1, 0) * max(b[3] - b[2] + 1, 0) for b in bb))
src_px = int((dr > 0).sum())
bytes_render = B * H * W * 4
bytes_icp = ITERS * (box_px * 4 + src_px * 5 * 4)
me, mg, mi = float(np.median(eager)), float(np.median(graph)), float(np.median(alone))
print(json.dumps({
    "B": B, "icp_iter": ITERS, "stages_per_round": N, "rounds": ROUNDS, "status": status.cpu().tolist(),
    "inliers_first_iter": stats[:, 0, 0].cpu().numpy().astype(int).tolist(), "box_pixels": box_px, "source_pixels": src_px,
    "stage_eager_us": round(me, 2), "stage_graph_us": round(mg, 2), "icp_only_eager_us": round(mi, 2),
    "icp_us_per_iteration": round(mi / ITERS, 2), "icp_launches": 2 * ITERS,
    "bytes_render": bytes_render, "bytes_icp": bytes_icp,
    "hbm_roof_us": round((bytes_render + bytes_icp) / HBM_BPS * 1e6, 2),
    "eager_rounds_us": [round(x, 1) for x in eager], "graph_rounds_us": [round(x, 1) for x in graph],
    "icp_rounds_us": [round(x, 1) for x in alone]}))
