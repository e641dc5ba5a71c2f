"""CPU: the numpy restatement of the visible surface discrepancy (lib/utils/misc.py, lib/utils/visibility.py, lib/utils/pose_error.py
vsd) against the reference's own distance images and visibility masks (tests/golden/vsd_golden.npz, written by
tests/golden/make_vsd_golden.py), the composition of the error, the config keys and the VSD table of the evaluator."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

CASES = ("a", "b")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "vsd_golden.npz"))
    return {k: g[k] for k in g.files}


def case(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")}


def compose(c, tau, cost_type, admit_through_gt=True):
    """the error from the golden masks and distance images, written out here once more (and, for the negative control, without the
    term that admits the estimate where the ground truth is visible)"""
    visib_gt, visib_est = c["visib_gt"], c["visib_est"]
    if not admit_through_gt:
        own = (c["dist_test"] > 0) & (c["dist_est"] > 0) & (c["dist_est"].astype(np.float32) - c["dist_test"].astype(np.float32) <= np.float32(c["delta"]))
        visib_est = own
    inter, union = visib_gt & visib_est, visib_gt | visib_est
    cost = np.abs(c["dist_gt"] - c["dist_est"])[inter]
    cost = (cost >= tau).astype(np.float64) if cost_type == "step" else np.minimum(cost * (1.0 / tau), 1.0)
    n_u, n_i = int(union.sum()), int(inter.sum())
    return (cost.sum() + (n_u - n_i)) / float(n_u), (int(visib_gt.sum()), n_u, n_i)


def test_golden_shapes_hold_the_vector_tail(golden):
    assert case(golden, "a")["depth_gt"].shape == (48, 64) and case(golden, "b")["depth_gt"].shape == (50, 63)
    assert len(golden["taus"]) == 8


@pytest.mark.parametrize("name", CASES)
def test_distance_images_equal_the_reference_bit_for_bit(golden, name):
    from lib.utils.misc import depth_im_to_dist_im

    c = case(golden, name)
    for k in ("test", "gt", "est"):
        got = depth_im_to_dist_im(c["depth_" + k], c["K"])
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), c["dist_" + k].view(np.uint64)), k


@pytest.mark.parametrize("name", CASES)
def test_visibility_masks_equal_the_reference(golden, name):
    from lib.utils import visibility as vis

    c = case(golden, name)
    visib_gt = vis.estimate_visib_mask_gt(c["dist_test"], c["dist_gt"], float(c["delta"]))
    visib_est = vis.estimate_visib_mask_est(c["dist_test"], c["dist_est"], visib_gt, float(c["delta"]))
    assert visib_gt.dtype == bool and np.array_equal(visib_gt, c["visib_gt"])
    assert np.array_equal(visib_est, c["visib_est"])
    assert np.array_equal(vis.estimate_visib_mask(c["dist_test"], c["dist_gt"], float(c["delta"])), c["visib_gt"])


@pytest.mark.parametrize("cost_type", ["step", "tlinear"])
@pytest.mark.parametrize("name", CASES)
def test_vsd_equals_the_error_composed_from_the_golden_masks(golden, name, cost_type):
    from lib.utils.pose_error import vsd

    c = case(golden, name)
    for tau in golden["taus"]:
        e, counts = vsd(c["depth_est"], c["depth_gt"], c["depth_test"], c["K"], float(c["delta"]), float(tau), cost_type)
        want, want_counts = compose(c, float(tau), cost_type)
        assert e == want and counts == want_counts, (tau, e, want)
        assert 0.0 < e < 1.0


def test_negative_control_the_admission_through_visib_gt_matters(golden):
    for name in CASES:
        c = case(golden, name)
        full, _ = compose(c, 0.02, "step")
        without, _ = compose(c, 0.02, "step", admit_through_gt=False)
        assert full != without, name


def test_unknown_cost_type_raises(golden):
    from lib.utils.pose_error import vsd

    c = case(golden, "a")
    with pytest.raises(ValueError):
        vsd(c["depth_est"], c["depth_gt"], c["depth_test"], c["K"], 0.015, 0.02, "linear")


def test_empty_union_gives_one(golden):
    from lib.utils.pose_error import vsd

    c = case(golden, "a")
    zero = np.zeros_like(c["depth_gt"])
    for planes in ((zero, zero, c["depth_test"]), (c["depth_est"], c["depth_gt"], zero), (zero, zero, zero)):
        for cost_type in ("step", "tlinear"):
            e, counts = vsd(planes[0], planes[1], planes[2], c["K"], 0.015, 0.02, cost_type)
            assert e == 1.0 and counts == (0, 0, 0)


def test_identical_planes_give_zero_under_any_occluder(golden):
    from lib.utils.pose_error import vsd

    c = case(golden, "b")
    rng = np.random.default_rng(5)
    for _ in range(3):
        test = c["depth_gt"].copy()
        test[test == 0] = 1.5
        y0, x0 = rng.integers(5, 30), rng.integers(5, 40)
        test[y0:y0 + 12, x0:x0 + 15] = 0.4                      # in front of the object
        e, (n_gt, n_u, n_i) = vsd(c["depth_gt"], c["depth_gt"], test, c["K"], 0.015, 0.02, "tlinear")
        assert e == 0.0 and n_gt == n_u == n_i and 0 < n_gt < int((c["depth_gt"] > 0).sum())


def test_config_defaults():
    from deepim.config.config import reset_config

    T = reset_config().TEST
    assert T.VSD is False and T.VSD_DELTA == 0.015 and list(T.VSD_TAU) == [0.02] and T.VSD_COST == "step" and T.VSD_THRESH == 0.3


def test_evaluate_pose_vsd_on_hand_made_lists():
    from deepim.config.config import reset_config
    from lib.dataset.evaluation import PoseEvaluator

    cfg = reset_config()
    cfg.TEST.VSD_TAU = [0.02, 0.05]
    try:
        ev = PoseEvaluator(["ape", "can", "cat"], {}, {})
        # [cls][iter]: ape has four poses, can none, cat two; two taus per pose
        errors = {"vsd": [[[[0.1, 0.0], [0.5, 0.2], [0.29, 0.31], [1.0, 1.0]], [[0.0, 0.0], [0.1, 0.1], [0.2, 0.2], [0.3, 0.25]]],
                          [[], []],
                          [[[0.9, 0.8], [0.7, 0.6]], [[0.9, 0.1], [0.2, 0.6]]]],
                  "visib_gt": [[[50, 100, 0, 0], [50, 100, 0, 0]], [[], []], [[30, 30], [30, 30]]],
                  "drawn_gt": [[[100, 100, 100, 0], [100, 100, 100, 0]], [[], []], [[40, 60], [40, 60]]]}
        out = ev.evaluate_pose_vsd(cfg, errors)
        assert out["num_valid_class"] == 2 and out["taus"] == [0.02, 0.05] and out["thresh"] == 0.3
        assert np.array_equal(out["acc"][0], [[0.5, 0.5], [0.75, 1.0]])
        assert np.array_equal(out["acc"][1], [[0.0, 0.0], [0.0, 0.0]])
        assert np.array_equal(out["acc"][2], [[0.0, 0.0], [0.5, 0.5]])
        assert out["visible_fraction"][0, 0] == pytest.approx(0.5) and np.isnan(out["visible_fraction"][1]).all()
        assert out["visible_fraction"][2, 1] == pytest.approx((0.75 + 0.5) / 2)
        assert out["overall"][0] == {0.02: 25.0, 0.05: 25.0} and out["overall"][1] == {0.02: 62.5, 0.05: 75.0}
        assert out["count_all"].tolist() == [4, 0, 2]
    finally:
        reset_config()
