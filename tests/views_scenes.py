"""Inputs of the joint-solve tests (tests/test_gpu_views_kernels.py; tests/test_views_host.py fixes them on the CPU): the analytic ICP
scenes of tests/icp_terms_scenes.py as the views of a group, under seeded general rigid extrinsics.  The fusion is algebra on the
partials, so the views of a group need not show one physical object."""
import numpy as np

import icp_reference as ir
import icp_terms_scenes as sc
import views_reference as vr


def rig(seed, n):
    """n general rigid extrinsics (n,3,4) float32: rotations up to about a radian, shifts up to half a metre"""
    rng = np.random.default_rng(1000 + seed)
    return np.stack([vr.random_rigid(rng) for _ in range(n)]).astype(np.float32)


def identity_rig(n):
    return np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))


def batch_scenes(n):
    """n scenes of one frame size (24 x 32) with the same switches: the three of BATCH, then again from the first"""
    return [sc.make(sc.BATCH[i % len(sc.BATCH)], "cut") for i in range(n)]


def rig_poses(seed, G):
    rng = np.random.default_rng(2000 + seed)
    return np.stack([vr.random_rigid(rng) + [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1.0]] for _ in range(G)]).astype(np.float32)


def empty_box(s):
    s.bbox = np.array([20, 10, 3, 15], np.int32)   # inverted: no source pixel
    return s


# ---------------------------------------------------------------------------------------------------------------- the group threshold
THRESHOLD_BOXES = ((8, 14, 4, 10), (15, 21, 4, 10))   # two 7 x 7 windows of f24a side by side; the too-deep patch takes some of the first
THRESHOLD_ITERS = 3


def threshold_views():
    """-> (scenes, X): two views of f24a-plain that differ in their box only, both in the same general camera, so the group's step is the
    single-view step over both windows and converges like it.  Each window holds between 32 and 63 counted points at every iteration."""
    scenes = []
    for box in THRESHOLD_BOXES:
        s = sc.make("f24a", "plain")
        s.name, s.bbox = "threshold-{}".format(box[0]), np.array(box, np.int32)
        scenes.append(s)
    return scenes, np.tile(rig(15, 1), (2, 1, 1))


def float32_model_chain(scenes, X, iters):
    """the joint reference driven by the float32 model of icp_accumulate_kernel -> vr.joint_refine's dict, plus `margins`: per iteration
    and view the gate margins of the float64 truth at the state row the model reached, and `truth_counts` next to the model's counts"""
    margins, truth_counts = [], []

    def view_sums(v, R, t):
        m = {}
        truth, _ = scenes[v].truth(R, t, margins=m)
        margins.append(m)
        truth_counts.append(truth[27])
        part, _ = scenes[v].partial(R, t, np.float32)
        return part.sum(axis=0)

    out = vr.joint_refine(view_sums, X.astype(np.float64), iters, np.stack([s.pose_in for s in scenes]), scenes[0].pose_in)
    V = len(scenes)
    out["margins"] = [margins[i * V:(i + 1) * V] for i in range(iters)]
    out["truth_counts"] = np.asarray(truth_counts).reshape(iters, V).T
    return out


def single_view_counts(s, iters):
    """the counts dim_icp_refine sees on one view alone (it never steps below the bound, so every iteration sees the first count)"""
    N = s.truth(np.eye(3), np.zeros(3))[0][27]
    assert N < ir.MIN_POINTS
    return [N] * iters
