"""GPU: photometric augmentation of observed training images (TRAIN.AUG_OBSERVED).  dim_augment_observed against the numpy restatement of
its rules (tests/augment_reference.py) bit for bit, on shapes smaller than a tile, shorter than the halo, off the tile grid and at the
network size, into guarded buffers; then both training data paths -- TrainDataLoader on a tiny written dataset and
SyntheticPairs.train_batches -- where image_observed is the reference applied to the unaugmented blob with the augmenter's own draws
and every other blob keeps its bits; and a few training iterations on augmented batches."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import augment_reference as ref  # noqa: E402
import guard_arena as ga  # noqa: E402
from scene import make_train_config  # noqa: E402

DEV = "cuda:0"
MEANS_BGR = np.array([103.939, 116.779, 123.68], dtype=np.float32)
IDENTITY = [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0]
SIGMA_OF_RADIUS = {1: 0.3, 2: 0.5, 3: 1.0, 7: 2.33}


def _params(B, on, radius, chain, seeds):
    from lib.utils.augment import AugmentParams, blur_taps

    p = AugmentParams(B)
    p.on[:] = on
    for b in range(B):
        if radius[b]:
            r, p.taps[b] = blur_taps(SIGMA_OF_RADIUS[radius[b]])
            assert r == radius[b]
        p.radius[b] = radius[b]
        p.chain[b] = np.asarray(chain[b] if isinstance(chain[0], (list, tuple)) else chain, dtype=np.float32)
    p.seed[:] = np.asarray(seeds, dtype=np.uint32)[:B]
    return p


SEEDS = [2 ** 32 - 1, 0, 12345]
ALL = [0.7, 1.25, 14.5, 0.93, 1.0, 1.08, 6.5]


def _sets(B, r_mix):
    """(name, AugmentParams, quantize): each component alone, all together, radii 0 / 1 / 7 mixed in one batch, a pair that is off,
    sigma = 0, rounding on and off"""
    ones, zero_r = [1] * B, [0] * B
    off_mid = [1, 0, 1][:B] if B == 3 else [0, 1]
    return [("blur alone", _params(B, ones, r_mix, IDENTITY, SEEDS), False),
            ("saturation alone", _params(B, ones, zero_r, [0.6, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0], SEEDS), False),
            ("contrast and brightness alone", _params(B, ones, zero_r, [1.0, 1.3, -21.25, 1.0, 1.0, 1.0, 0.0], SEEDS), False),
            ("gain alone", _params(B, ones, zero_r, [1.0, 1.0, 0.0, 0.9, 1.05, 1.1, 0.0], SEEDS), False),
            ("noise alone", _params(B, ones, zero_r, [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 8.0], SEEDS), False),
            ("rounding alone", _params(B, ones, zero_r, IDENTITY, SEEDS), True),
            ("all, rounded", _params(B, ones, r_mix, ALL, SEEDS), True),
            ("all, not rounded, sigma 0", _params(B, ones, r_mix[::-1], ALL[:6] + [0.0], SEEDS), False),
            ("all, one pair off", _params(B, off_mid, r_mix, [ALL, [1.4, 0.7, -30.0, 1.1, 0.9, 1.0, 2.0], ALL][:B], SEEDS), True)]


def _blob(B, H, W, seed):
    """grey levels beyond both ends of [0, 255] minus the plane means: the clamp works at both ends"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-40.0, 300.0, size=(B, 3, H, W)).astype(np.float32)
    v[:, :, :, : W // 3] = np.rint(v[:, :, :, : W // 3])      # whole grey levels, as a decoded file holds them
    return v - MEANS_BGR[::-1].reshape(1, 3, 1, 1)


def _run(blob, p, quantize):
    """the kernel on `blob` into a guarded output -> numpy; the guards and the input are checked"""
    from lib.hip import ops

    x = torch.from_numpy(blob).to(DEV)
    out = ga.dense(blob.shape, device=DEV)
    d = p.to_device(DEV)
    ops.augment_observed(x, d["on"], p.radius, d["taps"], d["chain"], d["seed"], MEANS_BGR, quantize=quantize, out=out.tensor)
    out.check("augment_observed")
    assert torch.equal(x.cpu(), torch.from_numpy(blob))
    return out.tensor.cpu().numpy()


def _assert_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("{}: {} of {} values differ, first at {}: {!r} != {!r}".format(what, len(bad), got.size, tuple(bad[0]),
                                                                                         got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("shape,r_mix", [((3, 19, 44), [0, 1, 7]),      # smaller than a tile in both axes
                                         ((2, 5, 64), [7, 1]),          # shorter than the halo: the clamp works on both sides at once
                                         ((2, 70, 136), [7, 1])])       # off the tile grid, several workgroups
def test_kernel_matches_the_rules_bit_for_bit(hip_lib, shape, r_mix):
    B, H, W = shape
    blob = _blob(B, H, W, seed=H)
    for name, p, quantize in _sets(B, r_mix):
        got = _run(blob, p, quantize)
        want = ref.augment(blob, MEANS_BGR, p.on, p.radius, p.taps, p.chain, p.seed, quantize)
        _assert_bits(got, want, "{} at {}".format(name, shape))
        for b in range(B):
            if p.on[b] == 0:
                assert np.array_equal(got[b].view(np.uint32), blob[b].view(np.uint32)), name
            else:
                assert not np.array_equal(got[b], blob[b]), name
        if name.startswith("all, rounded"):
            grey = got + MEANS_BGR[::-1].reshape(1, 3, 1, 1)
            assert grey.min() == 0.0 and grey.max() == 255.0            # both ends of the clamp were reached
            assert np.array_equal(np.rint(grey), grey)


def test_kernel_at_the_network_size(hip_lib):
    B, H, W = 2, 480, 640
    blob = _blob(B, H, W, seed=1)
    p = _params(B, [1, 1], [7, 2], [ALL, [1.4, 0.7, -30.0, 1.1, 0.9, 1.0, 2.0]], SEEDS)
    _assert_bits(_run(blob, p, True), ref.augment(blob, MEANS_BGR, p.on, p.radius, p.taps, p.chain, p.seed, True), "network size")


def test_wrapper_refuses_what_the_entry_refuses(hip_lib):
    from lib.hip import capi, ops

    x = torch.zeros((2, 3, 8, 16), device=DEV)
    p = _params(2, [1, 1], [0, 0], IDENTITY, SEEDS)
    d = p.to_device(DEV)
    with pytest.raises(capi.DeepIMHipError, match="alias"):
        ops.augment_observed(x, d["on"], p.radius, d["taps"], d["chain"], d["seed"], MEANS_BGR, out=x)
    with pytest.raises(capi.DeepIMHipError, match="radius 8 of pair 1"):
        ops.augment_observed(x, d["on"], [0, 8], d["taps"], d["chain"], d["seed"], MEANS_BGR)
    with pytest.raises(capi.DeepIMHipError, match="multiple of 4"):
        ops.augment_observed(torch.zeros((2, 3, 8, 18), device=DEV), d["on"], p.radius, d["taps"], d["chain"], d["seed"], MEANS_BGR)


# ---------------------------------------------------------------------------------------------------------------------- file loader
LH, LW = 120, 160


def _write_pairs(root, n, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    db = []
    for i in range(n):
        ren = np.zeros((LH, LW), np.uint16)
        ren[20 + i:70 + i, 30:100] = 700 + 10 * i
        label = np.zeros((LH, LW), np.uint8)
        label[24 + i:72 + i, 34:104] = 1
        p = {k: os.path.join(root, "{:03d}-{}.png".format(i, k)) for k in ("color", "color_r", "depth", "depth_r", "label")}
        Image.fromarray(rng.integers(0, 256, size=(LH, LW, 3)).astype(np.uint8)).save(p["color"], compress_level=1)
        Image.fromarray(rng.integers(0, 256, size=(LH, LW, 3)).astype(np.uint8)).save(p["color_r"], compress_level=1)
        Image.fromarray(np.where(label == 1, 710, 0).astype(np.uint16)).save(p["depth"])
        Image.fromarray(ren).save(p["depth_r"])
        Image.fromarray(label).save(p["label"])
        pose_r = np.hstack([np.eye(3), [[0.01 * i], [0.02], [0.7 + 0.01 * i]]]).astype(np.float32)
        pose_o = np.hstack([np.eye(3), [[0.012 * i], [0.018], [0.71]]]).astype(np.float32)
        db.append({"image_observed": p["color"], "image_rendered": p["color_r"], "depth_gt_observed": p["depth"], "depth_rendered": p["depth_r"],
                   "mask_gt_observed": p["label"], "mask_idx": 1, "pose_observed": pose_o, "pose_rendered": pose_r,
                   "gt_class": ["ape", "can"][i % 2], "height": LH, "width": LW, "img_flipped": False})
    return db


def _epochs(db, cfg, n_epochs):
    """-> [[batch dicts (numpy)] per epoch] of a fresh TrainDataLoader"""
    from deepim.core.loader import TrainDataLoader
    from lib.utils import image as I

    I.point_cloud_dict.clear()
    loader = TrainDataLoader(None, db, cfg, batch_size=2, shuffle=False, device=DEV, workers=2, height=LH, width=LW)
    out = []
    for e in range(n_epochs):
        loader.reset()
        out.append([{k: v.cpu().numpy().copy() for k, v in batch.items()} for batch in loader])
    loader.close()
    return out


def test_file_loader_augments_image_observed_alone(hip_lib, tmp_path):
    from lib.utils.augment import ObservedAugmenter

    cfg = make_train_config()
    try:
        cfg.SCALES = [(LH, LW)]
        cfg.dataset.class_name = ["ape", "can"]
        cfg.TRAIN.INIT_MASK, cfg.TRAIN.MASK_DILATE = "box_gt", True       # dilate thicknesses and point samples: global draws
        cfg.train_iter.NUM_3D_SAMPLE = 100
        cfg.dataset.model_dir = os.path.join(str(tmp_path), "models")
        for cls in cfg.dataset.class_name:
            os.makedirs(os.path.join(cfg.dataset.model_dir, cls))
            np.savetxt(os.path.join(cfg.dataset.model_dir, cls, "points.xyz"), np.random.default_rng(1).normal(size=(300, 3)) * 0.05)
        db = _write_pairs(os.path.join(str(tmp_path), "imgs"), 4)
        plain = _epochs(db, cfg, 2)
        cfg.TRAIN.AUG_OBSERVED = True
        first, again = _epochs(db, cfg, 2), _epochs(db, cfg, 1)
        aug = ObservedAugmenter(cfg)
        assert len(plain[0]) == 2 and set(plain[0][0]) == set(first[0][0])
        draws = []
        for e in range(2):
            for k in range(2):
                p = aug.draw([2 * k, 2 * k + 1], e)      # the key of a pair is its index in the pairdb
                draws.append(p)
                want = ref.augment(plain[e][k]["image_observed"], cfg.network.PIXEL_MEANS, p.on, p.radius, p.taps, p.chain, p.seed, True)
                _assert_bits(first[e][k]["image_observed"], want, "epoch {} batch {}".format(e, k))
                for name, blob in plain[e][k].items():
                    if name != "image_observed":
                        assert np.array_equal(first[e][k][name], blob), (name, e, k)
        assert sum(int(p.on.sum()) for p in draws) >= 4 and any(p.radius.any() for p in draws)
        assert any(not np.array_equal(first[0][k]["image_observed"], plain[0][k]["image_observed"]) for k in range(2))
        for k in range(2):       # a second epoch draws other parameters; the same seed gives the same batches
            assert not (np.array_equal(draws[k].chain, draws[2 + k].chain) and np.array_equal(draws[k].seed, draws[2 + k].seed))
            for name, blob in first[0][k].items():
                assert np.array_equal(again[0][k][name], blob), name
        assert any(not np.array_equal(first[0][k]["image_observed"], first[1][k]["image_observed"]) for k in range(2))
    finally:
        from deepim.config.config import reset_config

        reset_config()


# ---------------------------------------------------------------------------------------------------------------------- synthetic pairs
def _host(batch):
    return {k: v.cpu().numpy().copy() for k, v in batch.items() if torch.is_tensor(v)}


def test_synthetic_pairs_and_a_short_training_run(hip_lib):
    from deepim.core.module import MutableModule, fit_batch
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.synthetic_pairs import SyntheticPairs
    from lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti
    from lib.utils.augment import ObservedAugmenter

    cfg = make_train_config()
    try:
        cfg.TRAIN.SHUFFLE = False
        cfg.network.TRAIN_ITER_SIZE = 2
        B = 2
        plain = [_host(b) for b in SyntheticPairs(cfg, 4, B, subdiv=3, device=DEV).train_batches(0)]
        cfg.TRAIN.AUG_OBSERVED = True
        data = SyntheticPairs(cfg, 4, B, subdiv=3, device=DEV)
        aug = ObservedAugmenter(cfg)
        dev_batches = list(data.train_batches(0))
        got = [_host(b) for b in dev_batches]
        assert len(plain) == len(got) == 2
        n_on = 0
        for i in range(2):
            p = aug.draw([i * B, i * B + 1], 0)         # the key of a pair: batch_id * batch_pairs + slot
            n_on += int(p.on.sum())
            want = ref.augment(plain[i]["image_observed"], cfg.network.PIXEL_MEANS, p.on, p.radius, p.taps, p.chain, p.seed, True)
            _assert_bits(got[i]["image_observed"], want, "batch {}".format(i))
            assert set(got[i]) == set(plain[i])
            for name, blob in plain[i].items():
                if name != "image_observed":
                    assert np.array_equal(got[i][name], blob), (name, i)
        assert n_on >= 2
        same = [_host(b) for b in data.train_batches(0)]
        other = [_host(b) for b in data.train_batches(1)]
        for i in range(2):
            assert np.array_equal(same[i]["image_observed"], got[i]["image_observed"])
            assert np.array_equal(other[i]["image_rendered"], got[i]["image_rendered"])      # SHUFFLE off: the same pairs, other draws
        assert any(not np.array_equal(other[i]["image_observed"], got[i]["image_observed"]) for i in range(2))
        # ---- a few iterations through fit_batch on the augmented batches: the blob reaches the network, nothing about accuracy
        sym = deepIM_flownet()
        sym.get_symbol(cfg, is_train=True)
        params = sym.init_weights(cfg, {}, {}, seed=0)
        mod = MutableModule(cfg, params, B)
        upd = batchUpdaterPyMulti(cfg, 480, 640, render_machine=data.render_machine)
        w0 = mod.flat_w.clone()
        for batch in dev_batches:
            for o in fit_batch(mod, batch, upd, cfg.TRAIN.lr):
                assert torch.isfinite(o["loss_sums"]).all()
        assert mod.num_update == 4 and torch.isfinite(mod.flat_w).all() and not torch.equal(mod.flat_w, w0)
    finally:
        from deepim.config.config import reset_config

        reset_config()
