"""CPU: the host side of BOP's average recall (TEST.BOP_VSD): the tau table of the evaluator, evaluate_pose_bop19 against a table worked
out by hand below, the config keys, and the two configurations pred_eval refuses by name."""
import numpy as np
import pytest


def test_vsd_tau_table_equals_the_hand_written_products():
    from lib.dataset.evaluation import PoseEvaluator

    ev = PoseEvaluator(["ape", "can", "cat"], {}, {"ape": 0.1, "can": 0.2, "cat": 0.5})
    fracs = [0.05, 0.1, 0.5]
    got = ev.vsd_tau_table(fracs)
    assert got.dtype == np.float64 and got.shape == (3, 3)
    want = [[0.05 * 0.1, 0.1 * 0.1, 0.5 * 0.1], [0.05 * 0.2, 0.1 * 0.2, 0.5 * 0.2], [0.05 * 0.5, 0.1 * 0.5, 0.5 * 0.5]]
    assert got.tolist() == want and got[2, 2] == 0.25
    # float32 fractions or diameters are widened first, then multiplied once in float64
    ev32 = PoseEvaluator(["ape"], {}, {"ape": np.float32(0.1)})
    assert ev32.vsd_tau_table(np.array([0.3], np.float32))[0, 0] == float(np.float32(0.3)) * float(np.float32(0.1))
    assert ev.vsd_tau_table([0.05]).shape == (3, 1)


def hand_made():
    """[cls][iter], one iteration.  ape (diameter 0.1): p0 half visible; p1 below the visibility bar and p2 not drawn at all, both with
    perfect errors that must not count; p3 exactly at the bar (a target), with an inf MSSD and an MSPD exactly at a threshold.
    can (diameter 0.2): one fully visible pose.  cat: no pose."""
    return {"vsd_grid": [[[[0.2, 0.3], [0.0, 0.0], [0.0, 0.0], [0.5, 0.6]]], [[[0.1, 0.4]]], [[]]],
            "visib_gt": [[[50, 5, 0, 10]], [[80]], [[]]],
            "drawn_gt": [[[100, 100, 0, 100]], [[80]], [[]]],
            "mssd": [[[0.005, 0.0, 0.0, float("inf")]], [[0.03]], [[]]],
            "mspd": [[[4.0, 0.0, 0.0, 5.0]], [[7.0]], [[]]]}


def test_evaluate_pose_bop19_equals_the_table_worked_out_by_hand():
    from deepim.config.config import reset_config
    from lib.dataset.evaluation import PoseEvaluator

    cfg = reset_config()
    try:
        cfg.TEST.BOP_VSD_TAU = [0.1, 0.2]
        cfg.TEST.BOP_VSD_THRESH = [0.3, 0.5]
        cfg.TEST.BOP_MSSD_THRESH = [0.1, 0.2]
        cfg.TEST.BOP_MSPD_THRESH = [5, 10]
        ev = PoseEvaluator(["ape", "can", "cat"], {}, {"ape": 0.1, "can": 0.2, "cat": 0.3})
        out = ev.evaluate_pose_bop19(cfg, hand_made())
        assert out["count_all"].tolist() == [4, 1, 0] and out["count_targets"].tolist() == [[2], [1], [0]]
        assert out["num_valid_class"] == [2]
        assert out["recall_vsd"].shape == (3, 1, 2, 2)
        # ape, targets p0 and p3.  tau 0: errors 0.2, 0.5 -> below 0.3: p0; below 0.5: p0 (0.5 < 0.5 is a miss).
        #                         tau 1: errors 0.3, 0.6 -> below 0.3: none (0.3 < 0.3 is a miss); below 0.5: p0
        assert out["recall_vsd"][0, 0].tolist() == [[0.5, 0.5], [0.0, 0.5]]
        # can: tau 0: 0.1 -> both; tau 1: 0.4 -> the second only
        assert out["recall_vsd"][1, 0].tolist() == [[1.0, 1.0], [0.0, 1.0]]
        assert out["recall_vsd"][2, 0].tolist() == [[0.0, 0.0], [0.0, 0.0]]
        # MSSD below {0.1, 0.2} of the diameter: ape {0.01, 0.02}: p0 twice, p3 (inf) never; can {0.02, 0.04}: 0.03 the second only
        assert out["recall_mssd"][:, 0].tolist() == [[0.5, 0.5], [0.0, 1.0], [0.0, 0.0]]
        # MSPD below {5, 10} px: ape p0 (4) twice, p3 (5.0) the second only; can (7) the second only
        assert out["recall_mspd"][:, 0].tolist() == [[0.5, 1.0], [0.0, 1.0], [0.0, 0.0]]
        assert out["AR_VSD"][:, 0].tolist() == [0.375, 0.75, 0.0]
        assert out["AR_MSSD"][:, 0].tolist() == [0.5, 0.5, 0.0]
        assert out["AR_MSPD"][:, 0].tolist() == [0.75, 0.5, 0.0]
        assert out["AR"][:, 0] == pytest.approx([(0.375 + 0.5 + 0.75) / 3, (0.75 + 0.5 + 0.5) / 3, 0.0], abs=1e-15)
        # the mean over the two classes that have a target, in percent
        row = out["overall"][0]
        assert row["AR_VSD"] == 56.25 and row["AR_MSSD"] == 50.0 and row["AR_MSPD"] == 62.5
        assert row["AR"] == pytest.approx((0.375 + 0.5 + 0.75 + 0.75 + 0.5 + 0.5) / 6 * 100, abs=1e-12)
        # pooled over the three targets: VSD hits {2, 2, 0, 2} of 3; MSSD (each pose against its own diameter) {1, 2} of 3;
        # MSPD {1, 3} of 3
        pool = out["pooled"][0]
        assert pool["AR_VSD"] == pytest.approx(50.0, abs=1e-12) and pool["AR_MSSD"] == pytest.approx(50.0, abs=1e-12)
        assert pool["AR_MSPD"] == pytest.approx(200.0 / 3, abs=1e-12)
        assert pool["AR"] == pytest.approx((50.0 + 50.0 + 200.0 / 3) / 3, abs=1e-12)
        # three targets in classes of two and one: the pooled AR is not the class mean
        assert abs(pool["AR"] - row["AR"]) > 0.5
        assert out["tau_fracs"] == [0.1, 0.2] and out["thresh_vsd"] == [0.3, 0.5] and out["min_visib_fract"] == 0.1
    finally:
        reset_config()


def test_the_visibility_bar_moves_the_targets():
    from deepim.config.config import reset_config
    from lib.dataset.evaluation import PoseEvaluator

    cfg = reset_config()
    try:
        cfg.TEST.BOP_VSD_TAU = [0.1, 0.2]
        cfg.TEST.BOP_MIN_VISIB_FRACT = 0.05   # p1 (5 of 100 pixels) becomes a target; p2 (nothing drawn) never does
        ev = PoseEvaluator(["ape", "can", "cat"], {}, {"ape": 0.1, "can": 0.2, "cat": 0.3})
        out = ev.evaluate_pose_bop19(cfg, hand_made())
        assert out["count_targets"].tolist() == [[3], [1], [0]]
        bad = hand_made()
        bad["mssd"][0][0] = bad["mssd"][0][0][:3]
        with pytest.raises(ValueError, match="mssd"):
            ev.evaluate_pose_bop19(cfg, bad)
    finally:
        reset_config()


def test_config_defaults():
    from deepim.config.config import reset_config

    T = reset_config().TEST
    grid = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
    assert T.BOP_VSD is False and T.BOP_VSD_DELTA == 0.015 and T.BOP_MIN_VISIB_FRACT == 0.1
    assert list(T.BOP_VSD_TAU) == grid and list(T.BOP_VSD_THRESH) == grid


def test_pred_eval_refuses_bop_vsd_without_bop_and_without_depth_observed():
    from deepim.config.config import reset_config
    from deepim.core.tester import VsdScorer, bop_vsd_settings, pred_eval
    from lib.dataset.evaluation import PoseEvaluator

    cfg = reset_config()
    try:
        ev = PoseEvaluator(["ape"], {}, {"ape": 0.1})
        assert bop_vsd_settings(cfg) == (False, None, None)
        cfg.TEST.BOP_VSD = True
        with pytest.raises(ValueError, match=r"TEST\.BOP_VSD needs TEST\.BOP"):
            pred_eval(cfg, None, [], ev)   # refused before the refiner is looked at
        cfg.TEST.BOP = True
        on, delta, fracs = bop_vsd_settings(cfg)
        assert on is True and delta == 0.015 and len(fracs) == 10
        with pytest.raises(KeyError, match=r"TEST\.BOP_VSD needs the blob 'depth_observed'"):
            VsdScorer.check({"image_observed": None}, "TEST.BOP_VSD")
        VsdScorer.check({"depth_observed": np.zeros((1, 1, 2, 2), np.float32)}, "TEST.BOP_VSD")
        cfg.TEST.BOP_VSD_TAU = [0.05] * 17
        with pytest.raises(ValueError, match="BOP_VSD_TAU"):
            bop_vsd_settings(cfg)
        cfg.TEST.BOP_VSD_TAU = [0.05, 0.0]
        with pytest.raises(ValueError, match="BOP_VSD_TAU"):
            bop_vsd_settings(cfg)
    finally:
        reset_config()
