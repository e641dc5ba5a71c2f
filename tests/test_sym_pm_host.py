"""CPU: the float64 restatement of the symmetry-aware point-matching loss (tests/sym_pm_reference.py) against torch autograd of
min_s L_s, the separation of its named mutants, the margin that keeps a float32 arg-min from legitimately differing on the inputs the
GPU test uses, the tie rule, and lib.utils.symmetry.symmetry_tables."""
import numpy as np
import pytest
import torch

import sym_pm_reference as S
from train_head_reference import f64, sc, worst_ratio


def _autograd(inp, loss_type, s):
    """sum_b min_s L_s and its gradient times grad_scale, by float64 autograd"""
    a = torch.tensor(f64(inp["p_est"]), requires_grad=True)
    x, w, pose = (torch.tensor(f64(inp[k])) for k in ("points_model", "weights", "tgt_pose"))
    inv, s = 1.0 / sc(S.ARGS["norm_term"]), sc(s)
    total = 0.0
    for b, S_all in enumerate(S._sets(inp["sym"], inp["sym_off"], inp["class_index"])):
        Ls = []
        for Sm in torch.tensor(S_all):
            G_R, G_t = pose[b, :, :3] @ Sm[:, :3], pose[b, :, :3] @ Sm[:, 3] + pose[b, :, 3]
            r = (a[b] - (G_R @ x[b] + G_t[:, None])) * inv
            if loss_type == "L1":
                v = r.abs()
            elif loss_type == "L2":
                v = r * r
            else:
                v = torch.where(r.abs() < 1.0 / (s * s), 0.5 * s * s * r * r, r.abs() - 0.5 / (s * s))
            Ls.append((w[b] * v).sum())
        total = total + torch.stack(Ls).min()
    total.backward()
    return float(total.detach()), a.grad.numpy() * sc(S.ARGS["grad_scale"])


@pytest.mark.parametrize("loss_type,s", S.CASES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_reference_is_autograd_of_min(loss_type, s, variant):
    inp = S.inputs(257, variant)
    ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, **S.ARGS)
    loss, grad = _autograd(inp, loss_type, s)
    assert np.array_equal(ref["best_sym"], inp["true_sym"])
    assert abs(ref["loss_sum"][0] - loss) <= 1e-12 * abs(loss)
    assert np.abs(ref["grad"][0] - grad).max() <= 1e-12 * np.abs(grad).max()


@pytest.mark.parametrize("loss_type,s", S.CASES)
@pytest.mark.parametrize("n", S.SIZES)
def test_gpu_inputs_keep_the_margin(n, loss_type, s):
    """on every input set of tests/test_gpu_sym_pm.py (and the other two variants of each), the runner-up L_s exceeds the winner's by at
    least 100 x the sum of their two bars: no float32 evaluation inside the bars can pick another symmetry"""
    for variant in range(3):
        inp = S.inputs(n, variant)
        ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, **S.ARGS)
        assert np.array_equal(ref["best_sym"], inp["true_sym"])
        m = S.margins(ref)
        print("n={} {} variant {}: margins {}".format(n, loss_type, variant, m))
        assert np.all(m >= 100.0), (n, loss_type, variant, m)
    assert {S.variant_of(k, t) for k in S.SIZES for t, _ in S.CASES if k == n} == {0, 1, 2}
    assert {S.variant_of(k, t) for k in S.SIZES for t, _ in S.CASES if t == loss_type} == {0, 1, 2}


def test_true_symmetries_cover_first_last_and_a_later_chunk():
    sym, off, max_sym = S.tables()
    assert list(np.diff(off)) == [1, 2, 33] and max_sym == 33
    axis = sorted({row[1] for row in S.TRUE_SYM})
    assert axis == [0, S.CHUNK, 32] and S.CHUNK % S.CHUNK == 0 and 32 == np.diff(off)[2] - 1
    assert sorted({row[0] for row in S.TRUE_SYM}) == [0, 1]
    assert np.any(sym[off[1] + 1, :, 3] != 0.0)          # the flip's axis does not pass through the origin
    inp = S.inputs(257)
    assert np.all(inp["weights"][:, :, -25:] == 0.0) and np.all(inp["points_model"][:, :, -25:] == 0.0) and np.all(inp["weights"][:, :, :-25] == 1.0)


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_mutants_are_separated(mutant):
    """every mutant differs from the reference by more than 10 bars on at least one output of at least one shared input set (a
    different best_sym counts as separated: it is an integer)"""
    worst, index_differs = 0.0, False
    for inp in [S.inputs(257, v) for v in range(3)] + [S.tie_inputs()]:
        for loss_type, s in S.CASES:
            ref = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, **S.ARGS)
            mut = S.pm_sym_loss_grad(**S.kernel_args(inp), loss_type=loss_type, s=s, mutant=mutant, **S.ARGS)
            index_differs = index_differs or not np.array_equal(ref["best_sym"], mut["best_sym"])
            for k in ("target", "grad", "loss_sum"):
                worst = max(worst, worst_ratio(mut[k][0], *ref[k]))
    print("{}: {:.3g} bars, best_sym differs: {}".format(mutant, worst, index_differs))
    if mutant == "tie_to_last":     # two entries with the same bits: only the index tells them apart
        assert index_differs
    else:
        assert worst > 10.0, (mutant, worst)


def test_duplicate_entry_goes_to_the_smaller_index():
    inp = S.tie_inputs()
    ref = S.pm_sym_loss_grad(**S.kernel_args(inp), **S.ARGS)
    for L, _ in ref["L"]:
        assert L[1] == L[2] and L[1] < L[0]
    assert list(ref["best_sym"]) == [1, 1]
    assert list(S.pm_sym_loss_grad(**S.kernel_args(inp), mutant="tie_to_last", **S.ARGS)["best_sym"]) == [2, 2]


def test_bad_class_and_non_finite_rules():
    inp = S.inputs(3, 1)
    args = S.kernel_args(inp)
    args["class_index"] = np.array([3, 1, -1], np.int32)
    ref = S.pm_sym_loss_grad(**args, **S.ARGS)
    assert list(ref["best_sym"]) == [-1, 1, -1] and np.all(ref["grad"][0][[0, 2]] == 0.0) and np.any(ref["grad"][0][1] != 0.0)
    assert list(S.pm_sym_loss_grad(**S.kernel_args(inp), max_sym=2, **S.ARGS)["best_sym"]) == [0, 1, -1]
    nan = S.kernel_args(inp)
    nan["p_est"] = nan["p_est"].copy()
    nan["p_est"][1, 0, 0] = np.nan           # every L_s of pair 1 is NaN: the identity stays
    assert list(S.pm_sym_loss_grad(**nan, **S.ARGS)["best_sym"]) == [0, 0, 32]


def test_symmetry_tables_mixed_class_list():
    from lib.utils.symmetry import get_symmetry_transformations, symmetry_tables

    info = S.class_symmetries()
    classes = ["axis", "unlisted", "flip", "ready"]
    ready = np.stack([np.eye(4)[:3], get_symmetry_transformations(info["flip"])[1]])
    sym, off, max_sym = symmetry_tables(classes, dict(info, ready=ready), 0.1)
    assert sym.dtype == np.float64 and sym.shape == (32 + 1 + 2 + 2, 3, 4) and off.dtype == np.int32
    assert list(off) == [0, 32, 33, 35, 37] and max_sym == 32
    for c in range(4):
        assert np.array_equal(sym[off[c]], np.eye(4)[:3])            # identity first in every set
    assert np.array_equal(sym[0:32], get_symmetry_transformations(info["axis"], 0.1))
    assert np.array_equal(sym[33:35], get_symmetry_transformations(info["flip"], 0.1)) and np.array_equal(sym[35:37], ready)
    assert symmetry_tables(["a", "b"], {}, 0.1)[2] == 1 and symmetry_tables(["a"], None, 0.1)[0].shape == (1, 3, 4)
    with pytest.raises(ValueError):
        symmetry_tables(["a"], {"a": ready[::-1]}, 0.1)              # a set that does not start with the identity
    with pytest.raises(ValueError):
        symmetry_tables([], {}, 0.1)
