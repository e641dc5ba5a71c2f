"""Time of the pose-from-flow stage (ops.flow_pnp, dim_flow_pnp): 16 pairs at 480x640, TEST.FLOW_PNP_ITER = 8, on the depth rendered
at the initial pose and the flow to the ground-truth pose (dim_depth_to_flow), with device events -- eagerly and replayed from a
captured hipGraph -- and with the extra depth render of the loop's first iteration in front of it.  Bytes moved are counted from the
actual boxes (each iteration reads the box of the rendered depth, and flow (two planes) and valid where a quad holds a drawn pixel)
against the HBM roof (6.29 TB/s measured copy rate, MI355X_MICROARCH.md).
Prints one JSON line.  usage: flow_pnp_time.py [rounds] [stages per round]"""
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
B, H, W, ITERS, WARM, HUBER, GATE = 16, 480, 640, 8, 2, 2.0, 8.0
models = syn.make_models(seed=2333, n_models=1, subdiv=4)
rm = Render_Py(None, ["ape"], syn.LINEMOD_K, meshes=models)
cls, gt, init = syn.sample_pairs(5, B, angle_std=5.0, angle_max=15.0, xy_std=0.005, z_std=0.02)
ci = torch.zeros((B,), dtype=torch.int32, device=d)
pose, pose_gt = torch.from_numpy(init).to(d), torch.from_numpy(gt).to(d)
depth_gt = torch.zeros((B, 1, H, W), device=d)
rm.render_batch(ci, pose_gt, depth=depth_gt, mask_thr=0.0)
depth_r = torch.zeros((B, 1, H, W), device=d)
bbox = torch.zeros((B, 4), dtype=torch.int32, device=d)
status = torch.zeros((B,), dtype=torch.int32, device=d)
rm.render_batch(ci, pose, depth=depth_r, bbox=bbox, mask_thr=0.0, status=status)
flow, valid = ops.depth_to_flow(depth_r, depth_gt, ops.pose_to_KT(pose, pose_gt, rm.K), np.linalg.inv(np.asarray(rm.K, np.float64)))
stats = torch.zeros((B, ITERS, 2), device=d)
pose_out, se3_q = torch.zeros((B, 3, 4), device=d), torch.zeros((B, 7), device=d)
work = ops.flow_pnp_workspace(B, H, W, d)


def pnp():
    ops.flow_pnp(depth_r, flow, pose, rm.K, ITERS, WARM, HUBER, GATE, valid=valid, bbox=bbox, pose_out=pose_out, se3_q=se3_q, stats=stats,
                 status=status, workspace=work)


def stage():
    ops.fill(status, 0)
    rm.render_batch(ci, pose, depth=depth_r, bbox=bbox, mask_thr=0.0, status=status)
    pnp()


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
    pnp()
torch.cuda.current_stream().wait_stream(s)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    pnp()
eager, graph, with_render = [], [], []
for r in range(ROUNDS):
    order = [("e", pnp), ("g", g.replay), ("r", stage)]
    for tag, fn in (order if r % 2 == 0 else order[::-1]):
        {"e": eager, "g": graph, "r": with_render}[tag].append(timed(fn))
torch.cuda.synchronize()
bb = bbox.cpu().numpy()
dr = depth_r.cpu().numpy()[:, 0]
box_px = int(sum(max(b[1] - b[0] + 1, 0) * max(b[3] - b[2] + 1, 0) for b in bb))
quads = dr.reshape(B, H, W // 4, 4)
drawn_quad_px = int((quads > 0).any(axis=3).sum()) * 4
bytes_pnp = ITERS * (box_px * 4 + drawn_quad_px * 3 * 4)
me, mg, mr = float(np.median(eager)), float(np.median(graph)), float(np.median(with_render))
est = pose_out.cpu().numpy().astype(np.float64)
err_mm = [float(np.linalg.norm(est[b][:, 3] - gt[b][:, 3]) * 1e3) for b in range(B)]
print(json.dumps({
    "B": B, "flow_pnp_iter": ITERS, "stages_per_round": N, "rounds": ROUNDS, "status": status.cpu().tolist(),
    "points_first_iter": stats[:, 0, 0].cpu().numpy().astype(int).tolist(), "points_last_iter": stats[:, -1, 0].cpu().numpy().astype(int).tolist(),
    "translation_error_mm_max": round(max(err_mm), 4), "box_pixels": box_px, "drawn_quad_pixels": drawn_quad_px,
    "pnp_eager_us": round(me, 2), "pnp_graph_us": round(mg, 2), "pnp_with_depth_render_eager_us": round(mr, 2),
    "pnp_us_per_iteration": round(mg / ITERS, 2), "pnp_launches": 2 * ITERS, "bytes_pnp": bytes_pnp,
    "hbm_roof_us": round(bytes_pnp / HBM_BPS * 1e6, 2), "fraction_of_roof": round(bytes_pnp / HBM_BPS * 1e6 / mg, 4),
    "eager_rounds_us": [round(x, 1) for x in eager], "graph_rounds_us": [round(x, 1) for x in graph],
    "with_render_rounds_us": [round(x, 1) for x in with_render]}))
