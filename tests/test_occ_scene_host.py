"""Host side of the occluded / lit synthetic scenes: the numpy restatement of the composition rule against hand-written 4x6 cases,
the LINEMOD light draw against values typed in from the reference rule, the config defaults and the exported C symbols."""
import ctypes
import os

import numpy as np

import occ_scene_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dim_scene_compose_workspace_bytes", "dim_scene_compose", "dim_raster_render_lit_lm"]


def _layers(depths, labels):
    """depths: list of 4x6 arrays -> (bgr, depth, label) with colour = 10 * (slot + 1) + channel where the layer has any depth value"""
    S = len(depths)
    d = np.stack([np.asarray(x, np.float32) for x in depths]).reshape(S, 1, 4, 6)
    bgr = np.zeros((S, 4, 6, 3), np.float32)
    for s in range(S):
        bgr[s] = 10.0 * (s + 1) + np.arange(3, dtype=np.float32)
    return bgr, d, np.asarray(labels, np.int32)


def test_compose_hand_case_overlap_and_tie():
    a = np.zeros((4, 6)); a[1:3, 0:4] = 1.0          # slot 0: rows 1-2, columns 0-3 at 1.0 m
    b = np.zeros((4, 6)); b[0:3, 2:6] = 0.5          # slot 1 in front: rows 0-2, columns 2-5
    b[2, 2:6] = 1.0                                  # ... but row 2 ties with slot 0 where they overlap
    bgr, d, lab = _layers([a, b], [3, 7])
    o = ref.compose(bgr, d, lab, 2)
    want_label = np.array([[0, 0, 7, 7, 7, 7],
                           [3, 3, 7, 7, 7, 7],
                           [3, 3, 3, 3, 7, 7],      # the tie at columns 2-3 goes to the lower slot
                           [0, 0, 0, 0, 0, 0]], np.float32)
    np.testing.assert_array_equal(o["scene_label"][0, 0], want_label)
    want_depth = np.array([[0, 0, .5, .5, .5, .5], [1, 1, .5, .5, .5, .5], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]], np.float32)
    np.testing.assert_array_equal(o["scene_depth"][0, 0], want_depth)
    np.testing.assert_array_equal(o["counts"], [[8, 6], [12, 10]])
    np.testing.assert_array_equal(o["vis_bbox"], [[0, 3, 1, 2], [2, 5, 0, 2]])
    np.testing.assert_array_equal(o["vis_mask"][0, 0], (want_label == 3).astype(np.float32))
    np.testing.assert_array_equal(o["vis_mask"][1, 0], (want_label == 7).astype(np.float32))
    np.testing.assert_array_equal(o["scene_bgr"][0, 1, 0], [10, 11, 12])
    np.testing.assert_array_equal(o["scene_bgr"][0, 0, 2], [20, 21, 22])
    np.testing.assert_array_equal(o["scene_bgr"][0, 3, 3], [0, 0, 0])


def test_compose_hand_case_unused_hidden_empty_nan_negative():
    front = np.zeros((4, 6)); front[:, :] = 0.4      # slot 0 covers everything
    unused = np.zeros((4, 6)); unused[:, :] = 0.1    # slot 1 would win everywhere, but its label is 0: ignored
    hidden = np.zeros((4, 6)); hidden[1:3, 1:3] = 0.9   # slot 2 wholly behind slot 0
    empty = np.zeros((4, 6))                         # slot 3 has no pixel
    bad = np.zeros((4, 6)); bad[0, 0] = np.nan; bad[0, 1] = -0.2; bad[0, 2] = np.inf; bad[0, 3] = 0.3   # slot 4: one real pixel
    bgr, d, lab = _layers([front, unused, hidden, empty, bad], [1, 0, 2, 3, 4])
    o = ref.compose(bgr, d, lab, 5)
    want = np.ones((4, 6), np.float32); want[0, 3] = 4
    np.testing.assert_array_equal(o["scene_label"][0, 0], want)
    # full = depth > 0 of a USED layer: inf counts, NaN and negatives do not; the unused slot counts nothing
    np.testing.assert_array_equal(o["counts"], [[24, 23], [0, 0], [4, 0], [0, 0], [2, 1]])
    np.testing.assert_array_equal(o["vis_bbox"], [[0, 5, 0, 3], [6, -1, 4, -1], [6, -1, 4, -1], [6, -1, 4, -1], [3, 3, 0, 0]])
    assert o["vis_mask"][1].sum() == 0 and o["vis_mask"][2].sum() == 0
    np.testing.assert_array_equal(o["scene_depth"][0, 0, 0, :4], np.array([0.4, 0.4, 0.4, 0.3], np.float32))


def test_compose_two_scenes_are_independent():
    a = np.zeros((4, 6)); a[0, 0] = 1.0
    b = np.zeros((4, 6)); b[3, 5] = 2.0
    bgr, d, lab = _layers([a, b], [5, 6])
    o = ref.compose(bgr, d, lab, 1)   # S = 1: two scenes of one layer
    assert o["scene_label"].shape == (2, 1, 4, 6)
    assert o["scene_label"][0, 0, 0, 0] == 5 and o["scene_label"][1, 0, 3, 5] == 6 and o["scene_label"].sum() == 11
    np.testing.assert_array_equal(o["vis_bbox"], [[0, 0, 0, 0], [5, 5, 3, 3]])


def test_light_draw_against_typed_values():
    from lib.utils import synthetic as syn

    pose = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 0.9]], np.float64)
    # typed in from LM6d_occ_dsm_1_gen_observed_light.py:130-142, :187-192: idx % 6 == 3 -> [-1, 1, 1] * 0.5, then += tx, -= ty, -= tz
    want_pos = {0: [0.6, 0.2, -0.4], 1: [0.6, 0.7, -0.4], 2: [0.1, 0.7, -0.4], 3: [-0.4, 0.7, -0.4], 4: [-0.4, 0.2, -0.4],
                5: [0.1, 0.2, -0.4], 9: [-0.4, 0.7, -0.4]}
    for idx, w in want_pos.items():
        lp, li, k = syn.lm_light_draw(7, idx, pose)
        np.testing.assert_allclose(lp, w, rtol=0, atol=1e-15)
    # the colour table (:146-156) and U(0.8, 1.2): every channel is 0 or in [0.8, 1.2], and the zero pattern is a table row
    rows = set()
    for seed in range(200):
        lp, li, k = syn.lm_light_draw(seed, 0, pose)
        r_lp, r_li, r_k = ref.light_draw(seed, 0, pose.tolist())
        np.testing.assert_array_equal(li, r_li)
        np.testing.assert_array_equal(lp, r_lp)
        assert k == r_k and 0 <= k < 5
        assert all(v == 0 or 0.8 <= v <= 1.2 for v in li)
        rows.add(tuple(int(v > 0) for v in li))
    assert rows == set(tuple(r) for r in [[0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]])
    assert syn.LM_BRIGHTNESS_RATIOS == [0.2, 0.25, 0.3, 0.35, 0.4]   # :98
    # given draws: colour row 4 = [1, 0, 1], factors typed in
    lp, li, k = ref.light_from_draws(4, pose.tolist(), [0.9, 1.1, 1.2], 4, 2)
    np.testing.assert_allclose(li, [0.9, 0.0, 1.2], rtol=0, atol=0)
    # seeded: the same seed gives the same light, another seed another one
    a, b = syn.lm_light_draw(11, 2, pose), syn.lm_light_draw(11, 2, pose)
    np.testing.assert_array_equal(a[1], b[1])
    assert not np.array_equal(a[1], syn.lm_light_draw(12, 2, pose)[1])


def test_distractor_draw_is_seeded_and_inside_the_box():
    from lib.utils import synthetic as syn

    models = syn.make_models(seed=3, n_models=3, subdiv=2)
    cls, gt, _ = syn.sample_pairs(5, 4, n_classes=3)
    dc, dp = syn.sample_distractors(9, cls, gt, models, 3, n_classes=3)
    dc2, dp2 = syn.sample_distractors(9, cls, gt, models, 3, n_classes=3)
    np.testing.assert_array_equal(dc, dc2)
    np.testing.assert_array_equal(dp, dp2)
    K = syn.LINEMOD_K
    for b in range(4):
        x0, x1, y0, y1 = syn.target_box(models[int(cls[b])][0], gt[b])
        for j in range(3):
            assert dc[b, j] != cls[b] and 0 <= dc[b, j] < 3
            t = dp[b, j, :, 3].astype(np.float64)
            u, v = K[0, 0] * t[0] / t[2] + K[0, 2], K[1, 1] * t[1] / t[2] + K[1, 2]
            assert x0 - 1e-3 <= u <= x1 + 1e-3 and y0 - 1e-3 <= v <= y1 + 1e-3
            assert abs(t[2] - gt[b][2, 3]) <= 0.3 + 1e-6
    one, _ = syn.sample_distractors(9, np.zeros(2, np.int32), gt[:2], models, 2, n_classes=1)
    assert (one == 0).all()   # a single class: the distractors are the same class


def test_config_defaults():
    from deepim.config.config import config

    assert config.dataset.SYN_OCC_OBJECTS == 0
    assert config.dataset.SYN_OCC_MAX_RATE == 0.85
    assert config.dataset.SYN_LIGHT is False


def test_new_symbols_exported_and_argument_checks(hip_lib):
    from lib.hip import capi

    header = open(os.path.join(ROOT, "include", "deepim_hip.h")).read()
    assert "#define DIM_STATUS_LAYER_HIDDEN 256" in header
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in capi.SIGNATURES, name
        assert hasattr(hip_lib, name), name
    # one row of 6 ints per workgroup of 256 pixels, layer and scene
    assert hip_lib.dim_scene_compose_workspace_bytes(16, 4, 480, 640) == 16 * 4 * 1200 * 6 * 4
    assert hip_lib.dim_scene_compose_workspace_bytes(0, 4, 480, 640) == 0
    fake = ctypes.c_void_p(16)
    call = lambda depth, S: hip_lib.dim_scene_compose(fake, depth, fake, 2, S, 4, 6, fake, fake, fake, fake, fake, fake, fake, None, None)  # noqa: E731
    assert call(fake, 0) == -1 and b"scene_compose" in hip_lib.dim_last_error()
    assert call(fake, 17) == -1 and b"S must be" in hip_lib.dim_last_error()
    assert call(None, 2) == -1 and b"null pointer" in hip_lib.dim_last_error()
