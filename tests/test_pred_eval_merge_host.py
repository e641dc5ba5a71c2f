"""CPU, gloo, world sizes 2 and 3: pred_eval(merge_ranks=True) on the shards of a test set gives on every rank what one process
gives on the whole set, for every list it collects -- the four reference lists, the ICP row, the per-pair hypothesis lists, the
pose-from-flow lists and rows, the coarse stage's lists -- and one result cache is written.  The refiner is a fake on CPU tensors,
so the families that need the device (DEVICE_EVAL errors, VSD, the BOP_VSD grid, BOP) do not run here: they are ScoreLists like
the others and travel through the same `extend`."""
import functools
import os
import pickle

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from lib.utils.dist_utils import shard_range
from test_dist_gloo import _free_port
from test_icp_host import _same

CONFIGS = ("icp_hyp", "flow_coarse")
N_BATCHES, P, T = 4, 3, 2   # 4 batches: 2/2 on two ranks, 2/1/1 on three


class _FakeShardRefiner(object):
    """what pred_eval reads from a Refiner, on CPU tensors: load() takes the next prepared batch, whose entries become the
    attributes the configuration's features leave on a Refiner"""

    def __init__(self, N, runs, coarse):
        self.P, self.N, self.B = P, N, P * N
        if coarse:
            self.coarse = object()
        self._runs = list(runs)

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None, hyp_poses=None, det_boxes=None):
        run = dict(self._runs.pop(0))
        self._refined = run.pop("refined")
        self.__dict__.update(run)

    def refine(self):
        return self._refined


def _setup(name):
    """-> cfg, evaluator, batches, runs (one per batch) of one configuration, the same in every process; pair 1 of every batch is
    undetected (src_pose = -1), so every shard holds one"""
    from lib.dataset.evaluation import PoseEvaluator
    from lib.utils import synthetic as syn
    from scene import make_test_config

    cfg = make_test_config(test_iter=T)
    cfg.dataset.class_name = ["ape", "cat"]
    cfg.network.PRED_FLOW = False   # no FlowEPE
    N = 1
    if name == "icp_hyp":
        cfg.TEST.ICP_ITER, N = 10, 2
    else:
        cfg.TEST.FLOW_PNP_ITER = 3
    rng = np.random.default_rng(11)
    pts = {c: rng.uniform(-0.05, 0.05, size=(200, 3)) for c in cfg.dataset.class_name}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, {c: 0.15 for c in cfg.dataset.class_name})
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    batches, runs = [], []
    for k in range(N_BATCHES):
        cls, gt, init = syn.sample_pairs(400 + k, P, n_classes=2)
        init = init.copy()
        init[1] = -1.0
        near = lambda s, shape=(): gt + rng.normal(0, s, shape + gt.shape)  # noqa: E731
        z = torch.zeros((P, 1, 4, 4))
        batch = {"image_observed": z, "mask_observed": z, "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt)}
        run = {"refined": f32(np.stack([near(0.02 / (it + 1)) for it in range(T)]))}
        if name == "icp_hyp":
            batch.update(image_rendered=z, mask_rendered=z, src_pose=f32(init))
            choice = rng.integers(0, N, size=P).astype(np.int32)
            run.update(poses_iter=f32(near(0.02, (T, N)).transpose(0, 2, 1, 3, 4).reshape(T, P * N, 3, 4)),
                       hyp_score=f32(rng.uniform(0, 1, P * N)), hyp_choice=torch.from_numpy(choice), pose_icp=None,
                       pose_icp_sel=f32(near(0.001)))
        else:
            batch["det_bbox"] = torch.full((P, 4), float(k))
            run.update(coarse_out={"pose": f32(init.reshape(P, 1, 3, 4)), "idx": torch.full((P, 1), 7 + k, dtype=torch.int32),
                                   "score": f32(rng.uniform(0, 1, (P, 1))), "status": torch.zeros((P, 1), dtype=torch.int32)},
                       pose_flow_iter=f32(near(0.01, (T,))), flow_pnp_stats=f32(rng.uniform(1, 50, (T, P, 3, 2))),
                       status_flow=torch.from_numpy(rng.integers(0, 2, (T, P)).astype(np.int32) * 0xFFFF))
        batches.append(batch)
        runs.append(run)
    return cfg, ev, batches, runs, N


def _run(name, lo, hi, result_file):
    from deepim.core.tester import pred_eval

    cfg, ev, batches, runs, N = _setup(name)
    return pred_eval(cfg, _FakeShardRefiner(N, runs[lo:hi], name == "flow_coarse"), batches[lo:hi], ev, result_file=result_file)


@functools.lru_cache(maxsize=None)
def _single(name, out_dir):
    """one process, all batches in rank order -> out, the result cache's objects"""
    cache = os.path.join(out_dir, "single_{}.pkl".format(name))
    out = _run(name, 0, N_BATCHES, cache)
    with open(cache, "rb") as f:
        return out, pickle.load(f)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for name in CONFIGS:
        lo, hi = shard_range(N_BATCHES, rank, world)
        out = _run(name, lo, hi, os.path.join(out_dir, "cache_{}_rank{}.pkl".format(name, rank)))
        with open(os.path.join(out_dir, "out_{}_rank{}.pkl".format(name, rank)), "wb") as f:
            pickle.dump(out, f)
    dist.destroy_process_group()


def _check_world(world, tmp_path, single_dir):
    d = str(tmp_path)
    mp.spawn(_worker, args=(world, _free_port(), d), nprocs=world, join=True)
    for name in CONFIGS:
        want, want_cache = _single(name, single_dir)
        assert want["merged_over_ranks"] is False
        assert ("icp" in want and "hyp" in want) if name == "icp_hyp" else ("flow_pnp" in want and "coarse" in want)
        undetected = sum(r == 1000 for per_cls in want["all_rot_err"] for r in per_cls[T - 1])
        assert undetected == N_BATCHES and sum(len(per_cls[0]) for per_cls in want["all_rot_err"]) == N_BATCHES * P
        for rank in range(world):
            with open(os.path.join(d, "out_{}_rank{}.pkl".format(name, rank)), "rb") as f:
                got = pickle.load(f)
            assert got.pop("merged_over_ranks") is True
            _same(got, {k: v for k, v in want.items() if k != "merged_over_ranks"}, "{} rank {}".format(name, rank))
        caches = sorted(f for f in os.listdir(d) if f.startswith("cache_" + name))
        assert caches == ["cache_{}_rank0.pkl".format(name)]   # one result cache, written by rank 0
        with open(os.path.join(d, caches[0]), "rb") as f:
            _same(pickle.load(f), want_cache, name + " cache")


def test_two_ranks_score_what_one_process_scores(tmp_path, tmp_path_factory):
    _check_world(2, tmp_path, str(tmp_path_factory.getbasetemp()))


def test_three_ranks_with_uneven_shards_score_what_one_process_scores(tmp_path, tmp_path_factory):
    _check_world(3, tmp_path, str(tmp_path_factory.getbasetemp()))
