"""Time of the coarse stage (TEST.COARSE_VIEWS): P = 16 pairs, a 48 x 12 grid (M = 576, 9216 candidates), 480 x 640, chunks of 256,
both score modes.  Per mode: the whole CoarseInit.run (host clock around a synchronise) and its split into box fit, render, score and
top-k (device events around every call, summed over the chunks).  Next to it the path the indexed score replaces, on the same rendered
candidates: chunks of 192 (a third of a pair, so that a chunk has one observed frame), scored once by dim_pose_score_indexed and once by
dim_hyp_broadcast of the frame (rgb: the three colour planes, depth: the depth plane) into 192 rows + dim_pose_score.  Alternating
rounds, medians.  Prints one JSON line.
usage: coarse_time.py [rounds]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mx-deepim_amd")
sys.path[:0] = [ROOT, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from deepim.config.config import config as cfg, update_config  # noqa: E402
from deepim.core.coarse import CoarseInit, boxes_from_int  # noqa: E402
from lib.hip import ops  # noqa: E402
from lib.render_hip.render_py_multi import Render_Py  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
d = "cuda:0"
P, VIEWS, INPLANE, CHUNK, SUB = 16, 48, 12, 256, 192
H, W = 480, 640
update_config(os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_test.yaml"))
cfg.TEST.COARSE_VIEWS, cfg.TEST.COARSE_INPLANE, cfg.TEST.COARSE_CHUNK = VIEWS, INPLANE, CHUNK
models = syn.make_models(seed=2333, n_models=1, subdiv=5)
rm = Render_Py(None, cfg.dataset.class_name, cfg.dataset.INTRINSIC_MATRIX, zNear=cfg.dataset.ZNEAR, zFar=cfg.dataset.ZFAR, meshes=models)
batch = syn.build_device_batch(rm, P, seed=1000, pixel_means=cfg.network.PIXEL_MEANS)
img_o, cls = batch["image_observed"], batch["class_index"]
dep_o = torch.zeros((P, 1, H, W), device=d)
rm.render_batch(cls, batch["pose_gt"], depth=dep_o, mask_thr=0.0)
boxes = boxes_from_int(ops.mask_bbox(dep_o, 0.0))
dep_wall = torch.where(dep_o > 0, dep_o, torch.full_like(dep_o, 1.5)).contiguous()


def ev():
    return torch.cuda.Event(enable_timing=True)


def split_run(co):
    """one run with device events around every call -> us per stage"""
    marks = {"fit": [], "render": [], "score": [], "topk": []}

    def timed(key, fn, *a):
        e0, e1 = ev(), ev()
        e0.record()
        fn(*a)
        e1.record()
        marks[key].append((e0, e1))

    timed("fit", co.fit, boxes, cls, None)
    for a, e in co.chunks():
        timed("render", co.render, a, e, False)
        timed("score", co.score_chunk, a, e, img_o, dep_wall)
    timed("topk", co.topk)
    torch.cuda.synchronize()
    return {k: sum(e0.elapsed_time(e1) for e0, e1 in v) * 1e3 for k, v in marks.items()}


def whole_run(co):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    co.run(img_o, boxes, cls, depth_observed=dep_wall)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def replaced_path(co, mode, obs_b, dep_b, row_b, score_b, work_b):
    """chunks of SUB candidates of one pair, rendered once (untimed) and scored both ways -> (indexed us, broadcast us, copy us of it)"""
    t = {"indexed": [], "broadcast": [], "score": []}
    M = co.M
    for p in range(P):
        for a in range(p * M, (p + 1) * M, SUB):
            co.render(a, a + SUB, False)
            order = ("indexed", "broadcast") if (a // SUB) % 2 == 0 else ("broadcast", "indexed")
            for which in order:
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                if which == "indexed":
                    ops.pose_score(img_o, co.image[:SUB], co.depth[:SUB], mode, co.tau, depth_observed=dep_wall if mode == "depth" else None,
                                   bbox=co.bbox[:SUB], score=score_b, workspace=work_b, obs_row=row_b[a:a + SUB])
                    e1.record()
                    t["indexed"].append((e0, e1))
                else:
                    if mode == "depth":   # the depth score reads no colour: only the observed depth has to be in every row
                        ops.hyp_broadcast(dep_b, dep_wall[p:p + 1], SUB)
                    else:
                        ops.hyp_broadcast(obs_b, img_o[p:p + 1], SUB)
                    e1.record()
                    ops.pose_score(obs_b, co.image[:SUB], co.depth[:SUB], mode, co.tau, depth_observed=dep_b if mode == "depth" else None,
                                   bbox=co.bbox[:SUB], score=score_b, workspace=work_b)
                    e2.record()
                    t["broadcast"].append((e0, e2))
                    t["score"].append((e1, e2))
    torch.cuda.synchronize()
    return {k: sum(e0.elapsed_time(e1) for e0, e1 in v) * 1e3 for k, v in t.items()}


out = {"pairs": P, "candidates_per_pair": VIEWS * INPLANE, "chunk": CHUNK, "frame": [H, W], "rounds": ROUNDS,
       "points_per_class": int(rm.verts.shape[0]), "box_iter": int(cfg.TEST.COARSE_BOX_ITER)}
obs_b = torch.zeros((SUB, 3, H, W), device=d)
dep_b = torch.zeros((SUB, 1, H, W), device=d)
score_b = torch.zeros((SUB,), device=d)
work_b = ops.pose_score_workspace(SUB, H, W, d)
rm.reserve(SUB)
for mode in ("rgb", "depth"):
    cfg.TEST.COARSE_SCORE = mode
    co = CoarseInit(cfg, rm, None, P, 4)
    row_b = co.obs_row
    co.run(img_o, boxes, cls, depth_observed=dep_wall)   # warm-up of every shape
    replaced_path(co, mode, obs_b, dep_b, row_b, score_b, work_b)
    res = {}
    for rd in range(ROUNDS):
        parts = [("whole", lambda: {"whole": whole_run(co)}), ("split", lambda: split_run(co)),
                 ("replaced", lambda: {"sub_" + k: v for k, v in replaced_path(co, mode, obs_b, dep_b, row_b, score_b, work_b).items()})]
        for _, fn in (parts if rd % 2 == 0 else parts[::-1]):
            for k, v in fn().items():
                res.setdefault(k, []).append(v)
    med = {k: float(np.median(v)) for k, v in res.items()}
    idx = co.idx.cpu().numpy()
    out[mode] = {
        "run_ms": round(med["whole"] / 1e3, 3), "fit_us": round(med["fit"], 1), "render_ms": round(med["render"] / 1e3, 3),
        "score_ms": round(med["score"] / 1e3, 3), "topk_us": round(med["topk"], 1),
        "split_sum_ms": round((med["fit"] + med["render"] + med["score"] + med["topk"]) / 1e3, 3),
        "score_indexed_sub192_ms": round(med["sub_indexed"] / 1e3, 3), "broadcast_plus_score_sub192_ms": round(med["sub_broadcast"] / 1e3, 3),
        "score_after_broadcast_sub192_ms": round(med["sub_score"] / 1e3, 3),
        "broadcast_over_indexed": round(med["sub_broadcast"] / med["sub_indexed"], 2),
        "rejected_candidates": int((co.status_all & co.reject_mask).ne(0).sum()), "top1": idx[:, 0].tolist(),
        "spread_run_ms": [round(min(res["whole"]) / 1e3, 3), round(max(res["whole"]) / 1e3, 3)]}
print(json.dumps(out))
