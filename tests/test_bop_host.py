"""CPU: the symmetry sets (lib/utils/symmetry.py, PoseEvaluator), the host errors lib/utils/pose_error.py mssd / mspd against the
restatement tests/bop_reference.py, and the table of PoseEvaluator.evaluate_pose_bop against a case worked out by hand.

Bars: the host functions and the restatement compute the same float64 expression up to the order of three-term sums inside the
matrix products: |host - ref| <= 1e-10 * max(1, |ref|), the project's bar for metres and pixels."""
import numpy as np
import pytest

import bop_reference as ref

K_LM = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float64)
FLIP_X = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]          # 180 degrees about x
CONT_Z = {"axis": [0, 0, 1], "offset": [0, 0, 0]}


def _within_bar(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff = np.abs(got - want)
    bar = 1e-10 * np.maximum(1.0, np.abs(want))
    print("{}: max |got - ref| = {:.3e} (bar 1e-10 * max(1, |ref|), largest ratio {:.3e})".format(what, diff.max(), (diff / bar).max()))
    assert np.all(diff <= bar), (what, float(diff.max()))


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _pose(rng):
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
    return np.concatenate([_rot(rng.normal(size=3), rng.uniform(0, 180)), t[:, None]], axis=1)


def _mul(P, S):
    return np.concatenate([P[:, :3] @ S[:, :3], (P[:, :3] @ S[:, 3] + P[:, 3])[:, None]], axis=1)


# ------------------------------------------------------------------------------------------------------------------ symmetry sets
@pytest.mark.parametrize("info,step,size", [({}, 0.01, 1), ({"symmetries_discrete": [FLIP_X]}, 0.01, 2),
                                            ({"symmetries_continuous": [CONT_Z]}, 0.01, 315),
                                            ({"symmetries_discrete": [FLIP_X], "symmetries_continuous": [CONT_Z]}, 0.01, 630),
                                            ({"symmetries_continuous": [CONT_Z]}, 0.5, 7)])
def test_set_sizes_and_the_restatement(info, step, size):
    from lib.utils.symmetry import get_symmetry_transformations

    s = get_symmetry_transformations(info, step)
    assert s.shape == (size, 3, 4) and s.dtype == np.float64
    assert np.array_equal(s[0], np.eye(4)[:3])   # the identity first, exactly
    _within_bar(s, ref.symmetry_set(info, step), "set of {}".format(size))
    for m in s:   # rigid
        assert np.allclose(m[:, :3] @ m[:, :3].T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(m[:, :3]), 1.0)


def test_order_is_discrete_outer_continuous_inner():
    from lib.utils.symmetry import get_symmetry_transformations

    cont = get_symmetry_transformations({"symmetries_continuous": [CONT_Z]}, 0.5)
    both = get_symmetry_transformations({"symmetries_discrete": [FLIP_X], "symmetries_continuous": [CONT_Z]}, 0.5)
    assert both.shape == (14, 3, 4)
    assert np.array_equal(both[:7], cont)   # the identity among the discrete ones comes first
    flip = np.asarray(FLIP_X, np.float64).reshape(4, 4)[:3]
    assert np.array_equal(both[7], flip)
    for i in range(7):
        # rotation i by 2 pi i / 7 about z, applied after the flip
        assert np.allclose(cont[i][:, :3], _rot([0, 0, 1], 360.0 * i / 7), atol=1e-15)
        assert np.allclose(both[7 + i], _mul(cont[i], flip), atol=1e-15)


def test_offset_axis_keeps_its_own_points():
    from lib.utils.symmetry import get_symmetry_transformations

    axis, off = np.array([1.0, 2.0, -0.5]), np.array([0.02, -0.01, 0.03])
    s = get_symmetry_transformations({"symmetries_continuous": [{"axis": axis.tolist(), "offset": off.tolist()}]}, 0.3)
    assert len(s) == 11
    on_axis = off[None, :] + np.linspace(-0.1, 0.1, 5)[:, None] * axis[None, :] / np.linalg.norm(axis)
    away = off + np.array([0.05, 0.0, 0.0])
    for m in s[1:]:
        assert np.abs(on_axis @ m[:, :3].T + m[:, 3] - on_axis).max() < 1e-16 * 10
        assert np.linalg.norm(m[:, :3] @ away + m[:, 3] - away) > 1e-3
    with pytest.raises(ValueError):
        get_symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 0], "offset": [0, 0, 0]}]}, 0.3)


def test_evaluator_defaults_and_given_sets():
    from lib.dataset.evaluation import RT_Z, PoseEvaluator

    classes = ["ape", "eggbox", "bowl", "can"]
    ready = np.stack([np.eye(4)[:3], _mul(np.eye(4)[:3], np.concatenate([_rot([0, 1, 0], 120), np.zeros((3, 1))], axis=1))])
    ev = PoseEvaluator(classes, {}, {}, symmetries={"bowl": {"symmetries_continuous": [CONT_Z]}, "can": ready})
    sets = ev.symmetry_sets(0.5)
    assert [len(s) for s in sets] == [1, 2, 7, 2] and ev.max_sym(0.5) == 7 and ev.max_sym() == 315
    assert np.array_equal(sets[0], np.eye(4)[None, :3])                     # a class without an entry
    assert np.array_equal(sets[1], np.stack([np.eye(4)[:3], RT_Z]))        # the rule evaluation.py states for eggbox
    assert np.array_equal(sets[3], ready) and sets[3].dtype == np.float64
    # the constructor as every caller so far uses it
    plain = PoseEvaluator(["eggbox", "glue"], {}, {})
    assert [len(s) for s in plain.symmetry_sets()] == [2, 1]
    # an entry for eggbox replaces the default
    assert len(PoseEvaluator(["eggbox"], {}, {}, symmetries={"eggbox": {}}).symmetry_sets()[0]) == 1
    with pytest.raises(ValueError):
        PoseEvaluator(["can"], {}, {}, symmetries={"can": np.zeros((2, 4, 4))}).symmetry_sets()


# ------------------------------------------------------------------------------------------------------------------ host errors
def test_mssd_mspd_against_the_restatement():
    from lib.utils import pose_error as pe
    from lib.utils.symmetry import get_symmetry_transformations

    rng = np.random.default_rng(5)
    sets = [get_symmetry_transformations({}, 0.01), get_symmetry_transformations({"symmetries_discrete": [FLIP_X]}, 0.01),
            get_symmetry_transformations({"symmetries_discrete": [FLIP_X],
                                          "symmetries_continuous": [{"axis": [0, 1, 1], "offset": [0.01, 0, -0.02]}]}, 0.2)]
    got, want = [], []
    for syms in sets:
        for n in (1, 37, 500):
            pts = rng.uniform(-0.05, 0.05, size=(n, 3))
            gt = _pose(rng)
            est = np.concatenate([_rot(rng.normal(size=3), rng.uniform(0.5, 175)) @ gt[:, :3], gt[:, 3:] + rng.normal(size=(3, 1)) * 0.015], axis=1)
            got.append([pe.mssd(est[:, :3], est[:, 3], gt[:, :3], gt[:, 3], pts, syms),
                        pe.mspd(est[:, :3], est[:, 3], gt[:, :3], gt[:, 3], K_LM, pts, syms)])
            want.append(ref.mssd_mspd(est, gt, K_LM, pts, syms)[0])
    got, want = np.array(got), np.array(want)
    assert want[:, 0].min() > 1e-4 and want[:, 1].min() > 0.1
    _within_bar(got[:, 0], want[:, 0], "mssd")
    _within_bar(got[:, 1], want[:, 1], "mspd")


def test_invariant_cloud_scores_zero_only_with_its_set():
    from lib.utils import pose_error as pe
    from lib.utils.symmetry import get_symmetry_transformations

    rng = np.random.default_rng(9)
    info = {"symmetries_discrete": [FLIP_X], "symmetries_continuous": [CONT_Z]}
    syms = get_symmetry_transformations(info, 0.4)   # 8 rotations about z, times the flip about x: 16
    assert len(syms) == 16
    seed = rng.uniform(0.01, 0.05, size=(6, 3))
    # the orbit of six points under the whole set is invariant under it (the set is a group: the dihedral group of order 16)
    pts = np.concatenate([seed @ m[:, :3].T + m[:, 3] for m in syms])
    gt = _pose(rng)
    ident = np.eye(4)[None, :3]
    for k in (1, 5, 8, 13):
        est = _mul(gt, syms[k])
        args = (est[:, :3], est[:, 3], gt[:, :3], gt[:, 3])
        assert pe.mssd(*args, pts, syms) <= 1e-12
        assert pe.mspd(*args, K_LM, pts, syms) <= 1e-9    # pixels: 1e-12 m at ~1 m under a focal length of 572
        assert pe.mssd(*args, pts, ident) > 0.01
        assert pe.mspd(*args, K_LM, pts, ident) > 1.0
        assert ref.mssd_mspd(est, gt, K_LM, pts, syms)[1] == (k, k)


# ------------------------------------------------------------------------------------------------------------------ the table
def test_evaluate_pose_bop_by_hand():
    from deepim.config.config import config as cfg
    from lib.dataset.evaluation import PoseEvaluator

    assert list(cfg.TEST.BOP_MSSD_THRESH) == [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
    assert list(cfg.TEST.BOP_MSPD_THRESH) == [5, 10, 15, 20, 25, 30, 35, 40, 45, 50]
    assert cfg.TEST.BOP is False and cfg.TEST.BOP_SYM_STEP == 0.01
    ev = PoseEvaluator(["ape", "can", "cat"], {}, {"ape": 0.1, "can": 0.2, "cat": 0.3})
    inf = float("inf")
    # ape (d = 0.1): thresholds 0.005 .. 0.05.  iter 0: 0.004 passes all ten, 0.012 passes 0.015 .. 0.05 (8), inf none, 0.05 none (strict)
    # can (d = 0.2): thresholds 0.01 .. 0.1.  0.031 passes 0.04 .. 0.1 (7); cat has no poses
    errors = {"mssd": [[[0.004, 0.012, inf, 0.05], [0.004, 0.004, 0.004, 0.004]], [[0.031], [0.2]], [[], []]],
              "mspd": [[[4.0, 5.0, inf, 49.0], [1.0, 1.0, 1.0, 60.0]], [[26.0], [3.0]], [[], []]],
              "sym_mssd": [[[0, 0, -1, 0], [0, 0, 0, 0]], [[0], [0]], [[], []]],
              "sym_mspd": [[[0, 0, -1, 0], [0, 0, 0, 0]], [[0], [0]], [[], []]]}
    out = ev.evaluate_pose_bop(cfg, errors)
    assert out["num_valid_class"] == 2 and out["count_all"].tolist() == [4, 1, 0]
    assert out["recall_mssd"].shape == (3, 2, 10) and out["recall_mspd"].shape == (3, 2, 10)
    assert np.allclose(out["recall_mssd"][0, 0], [0.25, 0.25] + [0.5] * 8)
    assert np.allclose(out["recall_mssd"][0, 1], [1.0] * 10)
    assert np.allclose(out["recall_mssd"][1, 0], [0, 0, 0] + [1.0] * 7) and np.allclose(out["recall_mssd"][1, 1], 0.0)
    # mspd, ape iter 0: 4.0 passes all ten, 5.0 nine (not < 5), inf none, 49.0 one (50)
    assert np.allclose(out["recall_mspd"][0, 0], [0.25] + [0.5] * 8 + [0.75])
    assert np.allclose(out["recall_mspd"][0, 1], [0.75] * 10)
    assert np.allclose(out["recall_mspd"][1, 0], [0] * 5 + [1.0] * 5) and np.allclose(out["recall_mspd"][1, 1], 1.0)
    assert np.isclose(out["AR_MSSD"][0, 0], (2 * 0.25 + 8 * 0.5) / 10) and np.isclose(out["AR_MSSD"][1, 0], 0.7)
    assert np.isclose(out["AR_MSPD"][0, 0], (0.25 + 4.0 + 0.75) / 10) and np.isclose(out["AR_MSPD"][1, 0], 0.5)
    # the mean over the two classes that have poses, in per cent
    assert np.isclose(out["overall"][0]["AR_MSSD"], (0.45 + 0.7) / 2 * 100)
    assert np.isclose(out["overall"][1]["AR_MSSD"], (1.0 + 0.0) / 2 * 100)
    assert np.isclose(out["overall"][0]["AR_MSPD"], (0.5 + 0.5) / 2 * 100)
    assert np.isclose(out["overall"][1]["AR_MSPD"], (0.75 + 1.0) / 2 * 100)
    assert out["AR_MSSD"][2].tolist() == [0.0, 0.0]
