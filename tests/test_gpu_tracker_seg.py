"""deepim.core.tracker.Tracker with TEST.TRACK_SEG "color" on the device: P = 2 objects of one small mesh through a few 480x640 frames
of lib.dataset.synthetic_sequences with restricted colour ranges (object 96..255, background 0..159 per channel), the pose head
zeroed so that the loop holds the pose it starts from.

  mask parity    on every frame the device mask, its counts and the updated colour model equal tests/track_seg_reference.py run on the
                 read-back frame, start box, render and state, bit for bit
  mask quality   the IoU of every frame's mask against the silhouette of the ground-truth render
  graph replay   eager and graph-replayed runs agree bit for bit, also on a second video after reset()
  the polish     started a few pixels sideways, the silhouette stage fed the tracker's mask lands nearer the truth than the loop
  no model       without learn_colors() frame 0 has an empty mask and the silhouette stage returns the loop's pose
  occluder       the colour model of an occluded track stands still
  feature off    TRACK_SEG "none" gives the bits of a configuration without the keys"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_seg_reference as S  # noqa: E402
from test_gpu_tracker import MODEL_SEED, P, _cfg, _host, _observed, _tracker  # noqa: E402

DEV = "cuda:0"
FRAMES = 7
OBJECT_COLORS, BACKGROUND_COLORS = (96, 255), (0, 159)
SIL_FEW_POINTS = 2048
# The floor of the mask's IoU against the ground-truth silhouette: the minimum measured over the frames of both videos below (the table
# is in DESIGN.md section 6g) less 0.02 -- a seeded scene is deterministic apart from rasteriser edge pixels across driver versions
IOU_MEASURED_MIN = 0.9927
SEG_KEYS = ("TRACK_SEG", "TRACK_SEG_BITS", "TRACK_SEG_MARGIN", "TRACK_SEG_SMOOTH", "TRACK_SEG_RATE", "TRACK_SEG_MIN_PIXELS")


def _sequence(cfg, frames, seed, events=()):
    from lib.dataset.synthetic_sequences import SyntheticSequence

    return SyntheticSequence(cfg, frames, P, seed, device=DEV, events=events, subdiv=3, model_seed=MODEL_SEED, object_colors=OBJECT_COLORS,
                             background_colors=BACKGROUND_COLORS)


def _seg_cfg(sil_iter=0, **track):
    cfg = _cfg(test_iter=2, seg="color", **track)
    cfg.TEST.SIL_ITER = sil_iter
    return cfg


def _silhouettes(seq, poses):
    """(P,H,W) bool: where the render of each object at `poses` draws"""
    rm = seq.render_machine
    dep = torch.empty((P, 1, rm.height, rm.width), device=DEV)
    rm.render_batch(torch.from_numpy(seq.class_index).to(DEV), torch.from_numpy(np.ascontiguousarray(poses, np.float32)).to(DEV), depth=dep)
    return _host(dep)[:, 0] > 0


def _adds(seq, poses, poses_gt):
    from lib.utils import pose_error

    out = []
    for p in range(P):
        pts = seq.models[int(seq.class_index[p])][0].astype(np.float64)
        a, g = np.asarray(poses[p], np.float64), np.asarray(poses_gt[p], np.float64)
        out.append(float(pose_error.add(a[:, :3], a[:, 3], g[:, :3], g[:, 3], pts)))
    return out


def _follow(tr, seq, check):
    """reset, learn the colours on frame 0 at the true pose, then every frame -> per-frame host records; check: compare every frame
    with the reference from the state the tracker had"""
    from deepim.core.tracker import SEG_SKIP_MASK

    seg = tr.segmentation
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    first = seq.frame(0)
    n = _host(tr.learn_colors(first["frame_bgr"], pose=first["pose_gt"]))
    assert (n >= seg["min_pixels"]).all() and _host(tr.seg_age).tolist() == [1] * P, n
    recs = []
    for t in range(len(seq)):
        fr = seq.frame(t)
        hist0, age0 = _host(tr.seg_hist), _host(tr.seg_age)
        out = tr.step(fr["frame_bgr"])
        rec = {k: _host(out[k]) for k in ("pose", "flags", "mask", "seg_counts", "seg_age")}
        rec["seg_hist"] = _host(tr.seg_hist)
        recs.append(rec)
        if not check:
            continue
        frame = _host(fr["frame_bgr"])
        want_mask, want_cnt, want_bits = S.seg_mask(frame, _host(tr.bbox_start), hist0, age0, seg["bits"], seg["margin"], seg["radius"])
        assert rec["mask"].tobytes() == want_mask.tobytes(), ("mask", t, np.abs(rec["mask"] - want_mask).sum())
        assert np.array_equal(rec["seg_counts"], want_cnt) and not want_bits.any(), (t, rec["seg_counts"], want_cnt)
        want_hist, want_age, want_n = S.seg_learn(frame, _host(tr.depth_sc), None, _host(tr.bbox_sc), rec["flags"], SEG_SKIP_MASK, seg["bits"],
                                                  seg["margin"], seg["rate"], seg["min_pixels"], hist0, age0)
        assert np.array_equal(_host(tr.seg_learn_counts), want_n) and np.array_equal(rec["seg_age"], want_age), (t, want_n, want_age)
        assert rec["seg_hist"].tobytes() == want_hist.tobytes(), ("seg_hist", t)
    return recs


@pytest.fixture(scope="module")
def followed(hip_lib):
    """two videos through one eager and one graph-capturing tracker (velocity model, zeroed head: the tracked pose is the true one)"""
    runs = {}
    for graph in (False, True):
        cfg = _seg_cfg(motion="velocity", damping=1.0)
        seqs = [_sequence(cfg, FRAMES, seed) for seed in (8, 6)]
        tr, _ = _tracker(cfg, "zero", seqs[0], graph)
        assert tr.seg_on and "sil" not in tr.refiner.stages and (tr.graph is None)
        runs[graph] = [_follow(tr, seq, check=not graph) for seq in seqs]
        assert (tr.graph is not None) == graph
    return seqs, runs


def test_mask_and_model_match_the_reference_on_every_frame(followed):
    seqs, runs = followed      # the comparisons ran inside the fixture, frame by frame; here: that they compared something
    from lib.hip import ops

    for recs in runs[False]:
        flags = np.stack([r["flags"] for r in recs])
        assert not (flags & (ops.STATUS_TRACK_LOST | ops.STATUS_TRACK_SEG_NO_MODEL)).any(), flags
        assert [r["seg_age"].tolist() for r in recs] == [[t + 2] * P for t in range(FRAMES)]      # one update per frame after learn_colors
        assert all(r["seg_counts"][:, 1].min() > 5000 for r in recs)
        assert recs[0]["seg_hist"].tobytes() != recs[-1]["seg_hist"].tobytes()


def test_mask_quality_against_the_ground_truth_silhouette(followed):
    seqs, runs = followed
    table = []
    for seq, recs in zip(seqs, runs[False]):
        for t, rec in enumerate(recs):
            sil = _silhouettes(seq, seq.pose_gt[t])
            table.append([S.iou(rec["mask"][p, 0] > 0, sil[p]) for p in range(P)])
    table = np.asarray(table)
    print("IoU of the mask against the ground-truth silhouette, per frame (rows: video a frames 0.., then video b) and track:")
    print(np.round(table, 4).tolist(), "min {:.4f}".format(table.min()))
    assert IOU_MEASURED_MIN is not None, "the measured minimum has not been recorded"
    assert table.min() >= IOU_MEASURED_MIN - 0.02, table.min()


def test_eager_and_graph_runs_agree_bit_for_bit(followed):
    _, runs = followed
    for video, (eager, graph) in enumerate(zip(runs[False], runs[True])):
        for t, (a, b) in enumerate(zip(eager, graph)):
            for k in ("mask", "seg_counts", "seg_hist", "seg_age", "pose", "flags"):
                assert a[k].tobytes() == b[k].tobytes(), (video, t, k)


# ------------------------------------------------------------------------------------------------ the silhouette stage in the tracker
SIDEWAYS_PX = 4.0


def _sideways(seq, poses):
    """the poses moved SIDEWAYS_PX pixels along the image's x axis"""
    out = np.array(poses, np.float32, copy=True)
    out[:, 0, 3] += np.float32(SIDEWAYS_PX) * out[:, 2, 3] / np.float32(seq.K[0, 0])
    return out


def test_the_silhouette_polish_pays(hip_lib):
    from deepim.core.tester import Predictor, Refiner
    from lib.hip import ops

    cfg = _seg_cfg(sil_iter=2, motion="hold")
    seq = _sequence(cfg, 1, seed=8)
    tr, params = _tracker(cfg, "zero", seq, False)
    fr, gt = seq.frame(0), seq.pose_gt[0]
    start = _sideways(seq, gt)
    tr.reset(seq.class_index, start)
    tr.learn_colors(fr["frame_bgr"], pose=fr["pose_gt"])
    out = tr.step(fr["frame_bgr"])
    loop, sil = _host(out["pose"]), _host(tr.refiner.pose_sil)
    assert np.abs(loop - start).max() <= 1e-5 and out["mask"].data_ptr() == tr.refiner.mask_sil.data_ptr()   # the zeroed head holds the start
    assert not (_host(out["flags"]) & (ops.STATUS_TRACK_LOST | ops.STATUS_TRACK_SEG_NO_MODEL)).any()
    assert not (_host(tr.refiner.status_sil) & SIL_FEW_POINTS).any()
    add_loop, add_sil = _adds(seq, loop, gt), _adds(seq, sil, gt)
    # for the record: the plain Refiner's silhouette stage from the same start, fed the ground-truth silhouette
    rm, cls = seq.render_machine, torch.from_numpy(seq.class_index).to(DEV)
    H, W = rm.height, rm.width
    img_r, mask_r = torch.empty((P, 3, H, W), device=DEV), torch.empty((P, 1, H, W), device=DEV)
    d_start = torch.from_numpy(start).to(DEV)
    rm.render_batch(cls, d_start, image=img_r, mask=mask_r, plane_means=tr.refiner.net.plane_means, mask_thr=0.2)
    truth = torch.from_numpy(_silhouettes(seq, gt)[:, None].astype(np.float32)).to(DEV)
    plain = Refiner(cfg, Predictor(cfg, params, P), rm, P)
    plain.load(_observed(cfg, fr), img_r, truth, mask_r, d_start, cls)
    plain.refine()
    add_truth = _adds(seq, _host(plain.pose_sil), gt)
    iou = [S.iou(_host(out["mask"])[p, 0] > 0, _host(truth)[p, 0] > 0) for p in range(P)]
    print("ADD (m) per track from {} px sideways: loop {}, silhouette stage on the tracker's mask {}, on the ground-truth mask {}; "
          "IoU of the tracker's mask {}".format(SIDEWAYS_PX, add_loop, add_sil, add_truth, iou))
    for p in range(P):
        assert add_sil[p] < add_loop[p], (p, add_sil, add_loop)


def test_without_a_model_the_stage_returns_the_loops_pose(hip_lib):
    from lib.hip import ops

    cfg = _seg_cfg(sil_iter=2, motion="hold", pose="sil")
    seq = _sequence(cfg, 1, seed=8)
    tr, _ = _tracker(cfg, "zero", seq, False)
    fr = seq.frame(0)
    tr.reset(seq.class_index, _sideways(seq, seq.pose_gt[0]))
    out = tr.step(fr["frame_bgr"])               # no learn_colors
    flags, T = _host(out["flags"]), tr.refiner.test_iter
    assert not _host(out["mask"]).any() and _host(out["seg_counts"])[:, 1].tolist() == [0] * P
    assert _host(tr.refiner.pose_sil).tobytes() == _host(tr.refiner.poses_iter[T - 1]).tobytes()
    assert _host(out["pose"]).tobytes() == _host(tr.refiner.poses_iter[T - 1]).tobytes()
    assert (flags & SIL_FEW_POINTS).all() and (flags & ops.STATUS_TRACK_SEG_NO_MODEL).all() and not (flags & ops.STATUS_TRACK_LOST).any(), flags
    assert (_host(tr.refiner.status_sil) & SIL_FEW_POINTS).all()
    # the frame was accepted, so the model has learnt from it: the next frame has a mask
    assert _host(out["seg_age"]).tolist() == [1] * P
    out = tr.step(fr["frame_bgr"])
    assert not (_host(out["flags"]) & ops.STATUS_TRACK_SEG_NO_MODEL).any() and (_host(out["seg_counts"])[:, 1] > 5000).all()


# ------------------------------------------------------------------------------------------------ occluder
def test_the_model_of_an_occluded_track_stands_still(hip_lib):
    from lib.hip import ops
    from test_gpu_tracker_occlusion import HIDDEN, OCCLUDER

    cfg = _seg_cfg(motion="velocity", damping=1.0, score="rgb", occlusion="depth")
    seq = _sequence(cfg, 8, seed=8, events=[OCCLUDER])
    tr, _ = _tracker(cfg, "zero", seq, True)
    tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
    first = seq.frame(0)
    tr.learn_colors(first["frame_bgr"], pose=first["pose_gt"])
    flags, ages, hists = [], [], []
    for t in range(8):
        fr = seq.frame(t)
        out = tr.step(fr["frame_bgr"], depth_raw=fr["depth_raw"])
        flags.append(_host(out["flags"]))
        ages.append(_host(out["seg_age"]))
        hists.append(_host(tr.seg_hist))
    flags, ages = np.stack(flags), np.stack(ages)
    print("flags:", flags.tolist(), "seg_age:", ages.tolist())
    assert (flags[list(HIDDEN), 0] & ops.STATUS_TRACK_OCCLUDED).all() and not (flags[:, 1] & ops.STATUS_TRACK_OCCLUDED).any(), flags
    assert not (flags & ops.STATUS_TRACK_LOST).any(), flags
    before = HIDDEN[0] - 1
    for t in HIDDEN:
        assert ages[t, 0] == ages[before, 0] and hists[t][0].tobytes() == hists[before][0].tobytes(), t
    assert ages[:, 1].tolist() == list(range(2, 10))                       # the other track learns on every frame
    assert ages[-1, 0] == ages[before, 0] + (8 - 1 - HIDDEN[-1])            # ... and the hidden one again once it is back
    assert hists[-1][0].tobytes() != hists[before][0].tobytes()


# ------------------------------------------------------------------------------------------------ feature off
def test_none_is_a_configuration_without_the_keys(hip_lib):
    state = ("hist", "age", "ring", "ring_n", "ring_pos", "occ_age", "occluder_ok")
    runs = []
    for drop in (False, True):
        cfg = _cfg(test_iter=2, motion="velocity", damping=1.0, score="rgb")
        assert cfg.TEST.TRACK_SEG == "none"
        if drop:
            for k in SEG_KEYS:
                del cfg.TEST[k]
        seq = _sequence(cfg, 3, seed=8)
        tr, _ = _tracker(cfg, "moving", seq, True)
        tr.reset(seq.class_index, seq.pose_start[1], pose_prev=seq.pose_start[0])
        assert not tr.seg_on and tr.seg_hist is None
        rec = []
        for t in range(3):
            out = tr.step(seq.frame(t)["frame_bgr"])
            assert out.get("mask") is None and out.get("seg_counts") is None and out.get("seg_age") is None
            rec.append({k: _host(v) for k, v in out.items() if v is not None})
            rec[-1].update({k: _host(getattr(tr, k)) for k in state})
            rec[-1]["poses_iter"] = _host(tr.refiner.poses_iter)
        runs.append(rec)
    for t, (a, b) in enumerate(zip(*runs)):
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (t, k)
    with pytest.raises(ValueError, match="TRACK_SEG is 'none'"):
        tr.learn_colors(seq.frame(0)["frame_bgr"])


# ------------------------------------------------------------------------------------------------ the entry point
def test_track_entry_point_with_a_segmentation(hip_lib, tmp_path):
    import os
    import subprocess
    import sys

    from test_gpu_tracker import PKG

    cfg = os.path.join(PKG, "experiments", "deepim", "cfgs", "deepim_hip_LM_ape_track_seg.yaml")
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(PKG, "deepim", "track.py"), "--cfg", cfg, "--gpus", "0", "--num_frames", "4",
                        "--num_objects", "2", "--subdiv", "3", "--reinit_from_gt", "--seg", "--object_colors", "96", "255",
                        "--background_colors", "0", "159"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout
    assert "object  class  tracked  lost  reinit  mean ADD (m)  occluded  mask IoU  loop ADD (m)  sil ADD (m)" in out, out[-2000:]
    rows = [line.split() for line in out.splitlines() if line.split()[:1] in (["0"], ["1"]) and "ape" in line]
    assert len(rows) == 2 and all(len(row) == 10 and int(row[2]) + int(row[3]) == 4 for row in rows), out[-2000:]
    assert all(0.0 <= float(row[7]) <= 1.0 for row in rows), rows
    [float(row[k]) for row in rows for k in (8, 9)]     # numbers (nan for a track that was lost on every frame)
