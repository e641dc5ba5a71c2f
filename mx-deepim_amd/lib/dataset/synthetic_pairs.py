"""Seeded synthetic (observed, rendered) pairs standing in for the LINEMOD / ModelNet pairdbs (no datasets offline):
procedural textured meshes, GT pose uniform on SO(3) with z ~ U(0.6, 1.2) m, initial pose = GT + noise, observed image = render
over uniform noise.  Batches are built ON the device by the HIP rasteriser (lib/utils/synthetic.py) with the reference's blob names
(deepim/core/loader.py:35-41, :164-193), one list entry per batch of `batch_pairs` pairs of this rank's shard."""
import numpy as np
import torch

from lib.dataset.evaluation import PoseEvaluator
from lib.render_hip.render_py_multi import Render_Py
from lib.utils import synthetic as syn
from lib.utils.dist_utils import even_shard_range, shard_range

ICP_WALL_M = 1.5   # observed background depth of the synthetic pairs when the depth ICP is on


class SyntheticPairs(object):
    def __init__(self, config, num_pairs, batch_pairs, seed=2333, subdiv=4, device="cuda:0", rank=0, world=1, equal_shards=False):
        """equal_shards: every rank gets floor(n_batches / world) batches (training: one collective per optimizer step, so the
        counts must agree); False = sizes differ by at most one (test / inference: no collective on the data path)."""
        self.config = config
        self.classes = list(config.dataset.class_name)
        self.models = syn.make_models(seed=seed, n_models=len(self.classes), subdiv=subdiv)
        self.K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float32).reshape(3, 3)
        from deepim.symbols.deepIM_flownet import source_size

        self.height, self.width = source_size(config)   # config.SCALES: the size of the pairs, K the camera of that image
        self.render_machine = Render_Py(None, self.classes, self.K, width=self.width, height=self.height, zNear=config.dataset.ZNEAR,
                                        zFar=config.dataset.ZFAR, device=device, meshes=self.models)
        self.batch_pairs, self.device, self.seed = int(batch_pairs), device, seed
        # occluded / lit training scenes (dataset.SYN_OCC_OBJECTS, SYN_OCC_MAX_RATE, SYN_LIGHT); all off = the batches of before
        self.occluders = int(config.dataset.get("SYN_OCC_OBJECTS", 0) or 0)
        self.occ_max_rate = float(config.dataset.get("SYN_OCC_MAX_RATE", 0.85))
        self.lit = bool(config.dataset.get("SYN_LIGHT", False))
        self.light_machine = None
        if self.lit:
            from lib.render_hip.render_py_light_multi_program import Render_Py_Light_MultiProgram

            self.light_machine = Render_Py_Light_MultiProgram(self.classes, None, self.K, width=self.width, height=self.height,
                                                              zNear=config.dataset.ZNEAR, zFar=config.dataset.ZFAR,
                                                              brightness_ratios=syn.LM_BRIGHTNESS_RATIOS, device=device,
                                                              meshes=[(v, None, t, f, tex) for v, t, f, tex in self.models])
        # photometric augmentation of the observed training image (TRAIN.AUG_OBSERVED, lib/utils/augment.py); never at test time
        self.augmenter = None
        if config.TRAIN.get("AUG_OBSERVED", False):
            from lib.utils.augment import ObservedAugmenter

            self.augmenter = ObservedAugmenter(config)
        n_batches = int(num_pairs) // self.batch_pairs  # whole batches only
        lo, hi = (even_shard_range if equal_shards else shard_range)(n_batches, rank, world)
        if equal_shards and hi == lo:
            raise ValueError("{} batches cannot be split over {} ranks for training".format(n_batches, world))
        self.batch_ids = list(range(lo, hi))
        self.num_pairs = len(self.batch_ids) * self.batch_pairs

    def __len__(self):
        return len(self.batch_ids)

    def evaluator(self):
        pts = {c: m[0].astype(np.float64) for c, m in zip(self.classes, self.models)}
        diam = {c: float(np.linalg.norm(p.max(0) - p.min(0))) for c, p in pts.items()}
        return PoseEvaluator(self.classes, pts, diam)

    def test_batches(self):
        # the full test graph also scores the flow head (tester.py:500-512): its labels need the two depth planes of the pair record
        with_depth = bool(self.config.network.PRED_FLOW and not self.config.TEST.FAST_TEST)
        # the depth ICP after the loop (TEST.ICP_ITER > 0) reads an observed depth: the GT render over a flat wall at ICP_WALL_M, which
        # gives its gate something to reject
        # (the depth score of several hypotheses per pair and the VSD errors of TEST.VSD and TEST.BOP_VSD read it too)
        T = self.config.TEST
        icp = int(T.get("ICP_ITER", 0) or 0) > 0 or (int(T.get("HYP_NUM", 1) or 1) > 1 and T.get("HYP_SCORE", "rgb") == "depth")
        icp = icp or bool(T.get("VSD", False)) or bool(T.get("BOP_VSD", False))
        icp = icp or (int(T.get("COARSE_VIEWS", 0) or 0) > 0 and T.get("COARSE_SCORE", "rgb") == "depth")   # the coarse stage's depth score
        for i in self.batch_ids:
            b = syn.build_device_batch(self.render_machine, self.batch_pairs, seed=self.seed + 1000 * (i + 1), n_classes=len(self.classes),
                                       pixel_means=self.config.network.PIXEL_MEANS, device=self.device, with_depth=with_depth or icp)
            if icp:
                d = b["depth_gt_observed"]
                b["depth_observed"] = torch.where(d > 0, d, torch.full_like(d, ICP_WALL_M))
                if not with_depth:
                    del b["depth_gt_observed"], b["depth_rendered"]
            b["pose_observed"] = b["pose_gt"]
            yield b

    def train_batches(self, epoch):
        order = np.random.RandomState(self.seed + epoch).permutation(len(self.batch_ids)) if self.config.TRAIN.SHUFFLE else np.arange(len(self.batch_ids))
        for j in order:
            i = self.batch_ids[int(j)]
            b = syn.build_device_train_batch(self.render_machine, self.batch_pairs, seed=self.seed + 1000 * (i + 1), models=self.models,
                                             n_classes=len(self.classes), pixel_means=self.config.network.PIXEL_MEANS,
                                             npts=int(self.config.train_iter.NUM_3D_SAMPLE), device=self.device,
                                             occluders=self.occluders, lit=self.lit, occ_max_rate=self.occ_max_rate,
                                             light_machine=self.light_machine)
            if self.augmenter is not None:
                # the pair's key: batch_id * batch_pairs + slot.  image_observed is the only observed colour image of a batch (the
                # occluded-scene path merges its occluded and unoccluded renders into it), so it is the only blob that changes
                params = self.augmenter.draw([i * self.batch_pairs + s for s in range(self.batch_pairs)], epoch)
                b["image_observed"] = self.augmenter.apply(b["image_observed"], params, self.config.network.PIXEL_MEANS)
            yield b
