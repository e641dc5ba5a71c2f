"""CPU: the reference's per-pair camera rule of the test loop (deepim/core/tester.py:165, :560-562) as deepim.core.loader applies it --
K starts as the config K and a pair's `image_observed[:-10] + "-K.txt"` replaces it before that pair's re-render; nothing resets it."""
import os

import numpy as np
import pytest

K_CFG = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float32)


def _pairdb(root, n, with_k=()):
    """n records whose image_observed names end in the 10 characters the reference strips ("-color.png"); with_k: {i: K}"""
    db = []
    for i in range(n):
        db.append({"image_observed": os.path.join(root, "{:06d}-color.png".format(i))})
    for i, K in dict(with_k).items():
        np.savetxt(os.path.join(root, "{:06d}-K.txt".format(i)), K)
    return db


def _cam(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def test_no_files_keeps_the_config_K(tmp_path):
    from deepim.core.loader import resolve_pair_intrinsics

    K, has = resolve_pair_intrinsics(_pairdb(str(tmp_path), 4), K_CFG)
    assert K.shape == (4, 3, 3) and K.dtype == np.float32
    assert not has.any()
    for i in range(4):
        np.testing.assert_array_equal(K[i], K_CFG)


def test_file_on_the_first_record_holds_for_all(tmp_path):
    from deepim.core.loader import resolve_pair_intrinsics

    Ka = _cam(600.0, 610.0, 330.5, 250.25)
    K, has = resolve_pair_intrinsics(_pairdb(str(tmp_path), 3, {0: Ka}), K_CFG)
    assert has.tolist() == [True, False, False]
    for i in range(3):
        np.testing.assert_array_equal(K[i], Ka)


def test_file_in_the_middle_is_sticky(tmp_path):
    from deepim.core.loader import resolve_pair_intrinsics

    Ka = _cam(480.0, 470.0, 300.0, 220.0)
    K, has = resolve_pair_intrinsics(_pairdb(str(tmp_path), 5, {2: Ka}), K_CFG)
    assert has.tolist() == [False, False, True, False, False]
    for i in (0, 1):
        np.testing.assert_array_equal(K[i], K_CFG)   # before any file: the config K
    for i in (2, 3, 4):
        np.testing.assert_array_equal(K[i], Ka)      # the last K loaded, never reset


def test_two_different_files(tmp_path):
    from deepim.core.loader import resolve_pair_intrinsics

    Ka, Kb = _cam(500.0, 505.0, 310.0, 230.0), _cam(650.0, 640.0, 350.0, 260.0)
    K, has = resolve_pair_intrinsics(_pairdb(str(tmp_path), 6, {1: Ka, 4: Kb}), K_CFG)
    assert has.tolist() == [False, True, False, False, True, False]
    want = [K_CFG, Ka, Ka, Ka, Kb, Kb]
    for i in range(6):
        np.testing.assert_array_equal(K[i], want[i])


@pytest.mark.parametrize("content", ["1 2 3\n4 5 6\n", "not a number\n", "1 0 2\n0 nan 3\n0 0 1\n"])
def test_malformed_file_raises_with_its_path(tmp_path, content):
    from deepim.core.loader import resolve_pair_intrinsics

    db = _pairdb(str(tmp_path), 3)
    bad = os.path.join(str(tmp_path), "000001-K.txt")
    with open(bad, "w") as f:
        f.write(content)
    with pytest.raises(ValueError) as e:
        resolve_pair_intrinsics(db, K_CFG)
    assert bad in str(e.value)
