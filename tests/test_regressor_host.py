"""CPU: per-class pose regressors (network.REGRESSOR_NUM = K > 1).  The float64 restatement of tests/regressor_reference.py separates
every named mutant by more than 10 bars on the inputs the GPU tests use and reduces to tests/train_head_reference.py for K = 1; the
shape table, the per-class initialisation, the warm start from a class-agnostic checkpoint and the configuration checks."""
import numpy as np
import pytest

import regressor_reference as G
import train_head_reference as R

SEP = 10.0


def _cfg(classes, k, rot_type="QUAT"):
    from scene import make_test_config

    cfg = make_test_config(test_iter=2)
    cfg.dataset.class_name = list(classes)
    cfg.network.REGRESSOR_NUM = k
    cfg.network.ROT_TYPE = rot_type
    return cfg


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mutant", G.MUTANTS)
@pytest.mark.parametrize("B,K,classes", G.CASES[1:])      # a single sample has no second class to confuse it with
def test_shared_inputs_separate_every_mutant(B, K, classes, mutant):
    inp = G.inputs(B, K, classes)
    ref, mut = G.run_all(inp, K), G.run_all(inp, K, mutant=mutant)
    for op, name in G.MUTANT_OUTPUTS[mutant]:
        sep = R.worst_ratio(mut[op][name][0], ref[op][name][0], ref[op][name][1])
        print("{} {}.{} B={} K={}: {:.3g} bars".format(mutant, op, name, B, K, sep))
        assert sep > SEP, (mutant, op, name, sep)


def test_single_sample_case_separates_the_layout_mutant():
    B, K, classes = G.CASES[0]
    inp = G.inputs(B, K, classes)
    ref, mut = G.run_all(inp, K), G.run_all(inp, K, mutant="rot_block_stride_3")
    for op, name in G.MUTANT_OUTPUTS["rot_block_stride_3"]:
        assert R.worst_ratio(mut[op][name][0], ref[op][name][0], ref[op][name][1]) > SEP, (op, name)
    ref, mut = G.run_all(inp, K), G.run_all(inp, K, mutant="absent_class_rows_left_unwritten")
    assert R.worst_ratio(mut["wgrad"]["dW"][0], ref["wgrad"]["dW"][0], ref["wgrad"]["dW"][1]) > SEP


def test_cases_are_what_they_claim():
    (_, _, c1), (_, k2, c2), (b3, k3, c3) = G.CASES
    assert set(range(k2)) - set(c2) == {1} and list(c2).index(0) < len(c2) - 1 - list(c2)[::-1].index(2)   # 2 on both sides of a 0
    assert len(c3) == b3 and len(set(range(k3)) - set(c3)) >= 2
    assert [c for c in G.BAD_CASE[2] if not 0 <= c < G.BAD_CASE[1]] == [-1, G.BAD_CASE[1]]


@pytest.mark.parametrize("B", (1, 5))
def test_one_regressor_is_the_shared_head_reference(B):
    inp = G.inputs(B, 1, (0,) * B)
    for cls in (None, np.zeros(B, np.int32)):
        got = G.run_all(inp, 1, class_index=cls, trans_type="smooth_L1")
        want = R.pose_head_bwd(inp["fc6a"], inp["fc7"], inp["rot_raw"], inp["d_rot_norm"], inp["d_trans"], inp["fc7_w"], inp["rot_w"], inp["trans_w"])
        for k in want:
            np.testing.assert_allclose(got["bwd"][k][0], want[k][0], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(got["bwd"][k][1], want[k][1], rtol=1e-12, atol=1e-300)
        want = R.se3_dist_loss_grad(inp["rot_norm"], inp["rot_gt"], inp["fc7_dist"], inp["trans_w"], inp["trans_b"], inp["zt_gt"],
                                    inp["d_rot_prior"], inp["d_zt_prior"], G.DIST_ARGS["lw_rot"], G.DIST_ARGS["lw_trans"], trans_type="smooth_L1",
                                    s=G.DIST_ARGS["s"], sums_prior=inp["sums_prior"])
        for k in ("d_rot_norm", "d_zoom_trans"):
            np.testing.assert_allclose(got["dist"][k][0], want[k][0], rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(got["dist"][k][1], want[k][1], rtol=1e-12, atol=1e-300)
        for k in ("rot_loss_sum", "trans_loss_sum"):
            assert abs(got["dist"][k][0] - want[k][0]) <= 1e-12 * max(1.0, abs(want[k][0]))
        want = R.fc_wgrad(inp["d_rot_norm"], inp["fc7"])
        for k in want:
            np.testing.assert_array_equal(got["wgrad"][k][0], want[k][0])
            np.testing.assert_array_equal(got["wgrad"][k][1], want[k][1])


def test_forward_reference_vs_torch_float64():
    import torch
    import torch.nn.functional as F

    B, K, classes = G.CASES[1]
    inp = G.inputs(B, K, classes)
    ref = G.run_all(inp, K)["fwd"]
    t = lambda a: torch.from_numpy(R.f64(a))  # noqa: E731
    fc7 = F.leaky_relu(F.linear(t(inp["fc6"]), t(inp["fc7_w"]), t(inp["fc7_b"])), 0.1)
    rot = F.linear(fc7, t(inp["rot_w"]), t(inp["rot_b"])).view(B, K, 4)       # FullyConnected(num_hidden = 4K) reshaped and picked
    trans = F.linear(fc7, t(inp["trans_w"]), t(inp["trans_b"])).view(B, K, 3)
    pick = torch.as_tensor(np.asarray(classes), dtype=torch.long)
    rot, trans = rot[torch.arange(B), pick], trans[torch.arange(B), pick].clone()
    trans[:, :2] *= t(inp["zoom_factor"])[:, :1]
    np.testing.assert_allclose(ref["se3"][0], torch.cat([rot, trans], dim=1).numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["fc7"][0], fc7.numpy(), rtol=1e-12, atol=1e-15)
    assert np.all(ref["se3"][1] > 0) and np.all(ref["se3"][1] < 1e-2)      # worst-case bars: ~1e-3 of values of order 1


def test_out_of_range_class_in_the_reference():
    B, K, classes = G.BAD_CASE
    inp = G.inputs(B, K, classes)
    ref = G.run_all(inp, K)
    bad = [b for b, c in enumerate(classes) if not 0 <= c < K]
    for b in bad:
        assert list(ref["fwd"]["se3"][0][b]) == [1, 0, 0, 0, 0, 0, 0]
        assert not ref["bwd"]["dz7"][0][b].any() and not ref["bwd"]["dz6"][0][b].any() and not ref["bwd"]["d_rot"][0][b].any()
        np.testing.assert_array_equal(ref["dist"]["d_rot_norm"][0][b], R.f64(inp["d_rot_prior"][b]))
        np.testing.assert_array_equal(ref["dist"]["d_zoom_trans"][0][b], R.f64(inp["d_zt_prior"][b]))
    good = [b for b in range(B) if b not in bad]
    sub = {k: (v[good] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in inp.items()}
    want = G.run_all(sub, K)
    np.testing.assert_allclose(ref["wgrad"]["dW"][0], want["wgrad"]["dW"][0], rtol=1e-12)
    assert abs(ref["dist"]["trans_loss_sum"][0] - want["dist"]["trans_loss_sum"][0]) < 1e-12


# ------------------------------------------------------------------------------------------------ shapes, init, warm start, validation
def test_param_shapes_follow_regressor_num():
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    names = ["c{}".format(i) for i in range(13)]
    shp = deepIM_flownet().infer_param_shapes(_cfg(names, 13))
    assert shp["rot_weight"] == (52, 256) and shp["rot_bias"] == (52,)
    assert shp["trans_weight"] == (39, 256) and shp["trans_bias"] == (39,)
    assert shp["fc7_weight"] == (256, 256) and shp["fc6_weight"] == (256, 1024 * 8 * 10)      # shared
    shp = deepIM_flownet().infer_param_shapes(_cfg(names, 1))
    assert shp["rot_weight"] == (4, 256) and shp["trans_weight"] == (3, 256) and shp["trans_bias"] == (3,)


def test_init_weights_applies_the_head_rule_per_class():
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    K = 3
    sym = deepIM_flownet()
    cfg = _cfg(["a", "b", "c"], K)
    sym.get_symbol(cfg, is_train=True)
    p = sym.init_weights(cfg, {}, {}, seed=0)
    w = p["rot_weight"].reshape(K, 4, 256)
    assert w.dtype == np.float32
    assert np.all(w[:, 0] >= 0.01) and np.all(w[:, 0] <= 1.01) and np.all(w[:, 0].max(axis=1) > 0.5)     # row 0 of every block ~U(.01, 1.01)
    assert np.all(w[:, 1:] >= 0.0) and np.all(w[:, 1:] <= 0.01)                                          # the rest ~U(0, .01)
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2])                             # the classes draw their own
    assert not p["trans_weight"].any() and p["trans_weight"].shape == (9, 256)
    assert not p["rot_bias"].any() and p["rot_bias"].shape == (12,) and p["trans_bias"].shape == (9,)


def test_warm_start_tiles_a_class_agnostic_checkpoint():
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    one = deepIM_flownet()
    cfg1 = _cfg(["a", "b", "c"], 1)
    one.get_symbol(cfg1, is_train=True)
    ckpt = one.init_weights(cfg1, {}, {}, seed=5)
    rng = np.random.RandomState(0)
    for k in ("rot_bias", "trans_weight", "trans_bias"):
        ckpt[k] = rng.randn(*ckpt[k].shape).astype(np.float32)
    K = 3
    sym = deepIM_flownet()
    cfg = _cfg(["a", "b", "c"], K)
    sym.get_symbol(cfg, is_train=True)
    p = sym.init_weights(cfg, {k: v.copy() for k, v in ckpt.items()}, {}, seed=0)
    for k, rows in (("rot_weight", 4), ("rot_bias", 4), ("trans_weight", 3), ("trans_bias", 3)):
        assert p[k].shape[0] == rows * K
        for c in range(K):
            np.testing.assert_array_equal(p[k][rows * c:rows * (c + 1)], ckpt[k])
    np.testing.assert_array_equal(p["fc7_weight"], ckpt["fc7_weight"])


def test_a_per_class_checkpoint_under_one_regressor_is_refused():
    from deepim.symbols.deepIM_flownet import deepIM_flownet

    K = 3
    sym = deepIM_flownet()
    cfg = _cfg(["a", "b", "c"], K)
    sym.get_symbol(cfg, is_train=True)
    ckpt = sym.init_weights(cfg, {}, {}, seed=0)
    one = deepIM_flownet()
    cfg1 = _cfg(["a", "b", "c"], 1)
    one.get_symbol(cfg1, is_train=True)
    with pytest.raises(ValueError) as e:
        one.init_weights(cfg1, ckpt, {}, seed=0)
    assert "(12, 256)" in str(e.value) and "(4, 256)" in str(e.value)


def test_regressor_num_is_checked_against_the_class_list_and_the_rotation_type():
    from deepim.symbols.deepIM_flownet import deepIM_flownet, regressor_num

    assert regressor_num(_cfg(["a", "b"], 1)) == 1 and regressor_num(_cfg(["a", "b"], 2)) == 2
    with pytest.raises(ValueError) as e:
        regressor_num(_cfg(["a", "b", "c"], 13))
    assert "13" in str(e.value) and "3" in str(e.value).replace("13", "") and "REGRESSOR_NUM" in str(e.value)
    with pytest.raises(ValueError, match="REGRESSOR_NUM"):
        regressor_num(_cfg(["a", "b"], 0))
    with pytest.raises(ValueError, match="ROT_TYPE"):
        regressor_num(_cfg(["a", "b"], 2, rot_type="EULER"))
    assert regressor_num(_cfg(["a", "b"], 1, rot_type="EULER")) == 1
    # the shape table, which the training and the test entry both build first, goes through the same check
    with pytest.raises(ValueError, match="REGRESSOR_NUM"):
        deepIM_flownet().get_symbol(_cfg(["a", "b", "c"], 2), is_train=False)
    with pytest.raises(ValueError, match="REGRESSOR_NUM"):
        deepIM_flownet().get_symbol(_cfg(["a", "b", "c"], 2), is_train=True)
