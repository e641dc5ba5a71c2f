"""CPU: the silhouette pose polish after the refinement loop -- the rules of the nearest-edge field on hand-built masks (the
restatement tests/sil_reference.py against what the header says, and against a numpy column-then-row pass, the form the kernels
take), the restatement's convergence on analytic ellipsoid renders with its negative control, the new TEST keys and their refusals,
the host side of the C ABI (argument checks before any device call, the workspace size), the out["sil"] table of pred_eval with a
fake refiner on CPU tensors, and gpu_batches(): the small-frame inputs tests/test_gpu_sil.py compares the kernels on, proven sound
here.

The thresholds of the device comparisons are HUBER = 2.5 and GATE = 11.5 pixels, not the config defaults 2 and 12: in the first
iteration T is the identity, every contour point projects back onto its own pixel, and its distance e to an edge pixel is the root
of an integer -- exactly 2 or 12 for many points, where the last bit of e would decide the weight.  No integer has the root 2.5 or
11.5.

Convergence (4 pairs at 120x160, 3 rounds x 4 iterations, from 3-4 degrees and about a centimetre off; printed by the test): the rms
contour distance at the start of a round goes 0.86 / 0.69 / 0.64, 2.90 / 1.35 / 0.74, 2.62 / 0.62 / 0.56 and 2.64 / 0.69 / 0.62
pixels, and the displacement of the ellipsoid's axis ends from 9.8, 19.7, 19.3 and 13.7 mm to 6.7, 9.1, 9.7 and 5.3 mm: a silhouette
at this size (a pixel is 4 mm at the object) leaves depth and the rotation about the viewing direction of a near-round outline
weakly constrained."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import sil_reference as sr
from conftest import ROOT
from test_photo_host import _rot, ellipsoid_render

HUBER, GATE, RADIUS = 2.5, 11.5, 12       # device comparisons (see above); RADIUS = ceil(GATE), as the Refiner takes it
AXES = (0.20, 0.16, 0.13)                 # the ellipsoid of every frame here: its outline stays inside a 48x64 frame
HEADER = os.path.join(ROOT, "include", "deepim_hip.h")
FIELD_SIZES = ((37, 51), (48, 64))
FIELD_RADII = (1, 5, 12, 64)


# ------------------------------------------------------------------------------------------------------------------ the field
def hand_masks(H, W):
    """name -> (H,W) float32: the hand-built masks of the field tests"""
    ys, xs = np.mgrid[0:H, 0:W]
    out = {"empty": np.zeros((H, W), np.float32), "full": np.ones((H, W), np.float32)}
    one = np.zeros((H, W), np.float32)
    one[H // 3, W // 2 + 3] = 1.0
    out["one pixel"] = one
    out["disc"] = (((xs - 0.45 * W) ** 2 + (ys - 0.55 * H) ** 2) <= (0.3 * H) ** 2).astype(np.float32)
    rect = np.zeros((H, W), np.float32)
    rect[0:H // 2, W - W // 3:W] = 1.0      # touches the top and the right side of the frame
    out["rectangle at two sides"] = rect
    # two blobs, mirror images about the column c: pixels of column c are equally far from both (a tie in d^2 between ex < c and ex > c),
    # and the blobs' own rows mirror about row H // 2 (ties in d^2 and ex between two ey on the line between the blobs' halves)
    c, m = W // 2, H // 2
    blobs = np.zeros((H, W), np.float32)
    for dx, dy in ((5, 0), (6, 0), (7, 1), (7, -1), (8, 3), (8, -3), (6, 4), (6, -4), (9, 0)):
        blobs[m + dy, c - dx] = blobs[m + dy, c + dx] = 1.0
    out["mirror blobs"] = blobs
    val = np.zeros((H, W), np.float32)
    val[5:12, 6:20] = 0.5                   # exactly 0.5: foreground
    val[8, 10] = np.nan                     # a NaN: background, a hole with four edge pixels around it
    val[20:26, 8:14] = np.float32(0.49999997)   # just below: background
    val[14:17, 30:40] = np.nan
    out["0.5 and NaN"] = val
    return out


def two_pass_field(mask, radius):
    """the form the kernels take: per pixel the nearest edge row of its own column within the radius (the smaller row on a tie), then
    along the row the first least dx^2 + dy^2 <= radius^2 over x' = x - radius .. x + radius upwards"""
    edge = sr.edge_pixels(mask)
    H, W = edge.shape
    near = np.full((H, W), -1, np.int64)
    for x in range(W):
        for y in range(H):
            for dy in range(radius + 1):
                if y - dy >= 0 and edge[y - dy, x]:
                    near[y, x] = y - dy
                    break
                if y + dy < H and edge[y + dy, x]:
                    near[y, x] = y + dy
                    break
    out = np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in range(W):
            best = radius * radius + 1
            for xe in range(max(x - radius, 0), min(x + radius, W - 1) + 1):
                if near[y, xe] < 0:
                    continue
                d2 = (xe - x) ** 2 + (near[y, xe] - y) ** 2
                if d2 < best:
                    best, out[y, x] = d2, (near[y, xe] << 16) | xe
    return out


@functools.lru_cache(maxsize=None)
def field_reference(H, W, radius):
    """name -> the restatement's field of hand_masks(H, W); computed once per case"""
    return {k: sr.edge_field_pair(m, radius) for k, m in hand_masks(H, W).items()}


@pytest.mark.parametrize("size", FIELD_SIZES)
def test_field_rules_on_hand_built_masks(size):
    H, W = size
    masks = hand_masks(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    for radius in FIELD_RADII:
        f = field_reference(H, W, radius)
        assert np.all(f["empty"] == -1) and np.all(f["full"] == -1)      # the frame border is not an edge
        # one pixel: itself within the disc, nothing beyond
        py, px = H // 3, W // 2 + 3
        inside = (xs - px) ** 2 + (ys - py) ** 2 <= radius * radius
        assert np.array_equal(f["one pixel"], np.where(inside, (py << 16) | px, -1))
        # the rectangle: edges along its two inner sides only
        e = sr.edge_pixels(masks["rectangle at two sides"])
        x_in, y_in = W - W // 3, H // 2 - 1
        want = np.zeros((H, W), bool)
        want[0:H // 2, x_in] = True
        want[y_in, x_in:W] = True
        assert np.array_equal(e, want)
        # the frame corner inside it: straight left to (x_in, 0) or straight down to (W - 1, y_in), the left one on a tie (the smaller ex)
        left, down = W - 1 - x_in, y_in
        want = -1 if min(left, down) > radius else (x_in if left <= down else (y_in << 16) | (W - 1))
        assert f["rectangle at two sides"][0, W - 1] == want
        # every entry is an edge pixel within the radius, and no edge pixel is nearer
        for name, m in masks.items():
            e = sr.edge_pixels(m)
            got = f[name]
            has = got >= 0
            ey, ex = got >> 16, got & 0xFFFF
            assert np.all(e[ey[has], ex[has]]), name
            d2 = (ex - xs) ** 2 + (ey - ys) ** 2
            assert np.all(d2[has] <= radius * radius), name
            if e.any():
                qy, qx = np.nonzero(e)
                least = ((qy[None, None] - ys[..., None]) ** 2 + (qx[None, None] - xs[..., None]) ** 2).min(axis=2)
                assert np.array_equal(has, least <= radius * radius), name
                assert np.array_equal(d2[has], least[has]), name
        # the mirror line: a tie in d^2 goes to the smaller ex, and on the blobs' middle row a tie in (d^2, ex) to the smaller ey
        c, mid = W // 2, H // 2
        col = f["mirror blobs"][:, c]
        assert np.all((col[col >= 0] & 0xFFFF) < c)
        if radius >= 5:
            assert col[mid] == ((mid << 16) | (c - 5))
            assert f["mirror blobs"][mid, c - 6] == ((mid << 16) | (c - 6))           # an edge pixel is its own nearest
        # (c - 7, mid) is one pixel from (c - 7, mid - 1), (c - 7, mid + 1) and (c - 6, mid): the least ex, then the least ey
        assert f["mirror blobs"][mid, c - 7] == (((mid - 1) << 16) | (c - 7))
        # exactly 0.5 is foreground, a NaN and 0.49999997 are background
        e = sr.edge_pixels(masks["0.5 and NaN"])
        assert e[5, 6] and e[11, 19] and not e[7, 12]
        assert e[7, 10] and e[9, 10] and e[8, 9] and e[8, 11] and not e[8, 10]
        assert not e[20:26, 8:14].any() and not e[14:17, 30:40].any()


@pytest.mark.parametrize("size", FIELD_SIZES)
def test_column_then_row_gives_the_same_field(size):
    """the two-pass form of csrc/sil.hip is the brute-force minimum of (d^2, ex, ey), ties included"""
    H, W = size
    for radius in (1, 5, 12):
        f = field_reference(H, W, radius)
        for name, m in hand_masks(H, W).items():
            assert np.array_equal(two_pass_field(m, radius), f[name]), (name, radius)


def test_tie_rule_is_d2_then_ex_then_ey():
    m = np.zeros((9, 9), np.float32)
    m[4, 2] = m[4, 6] = m[2, 4] = m[6, 4] = 1.0     # four pixels, all 2 away from the centre: the least ex wins, not the least ey
    f = sr.edge_field_pair(m, 3)
    assert f[4, 4] == ((4 << 16) | 2)
    m[4, 2] = 0.0                                   # then ex = 4 twice: the least ey
    assert sr.edge_field_pair(m, 3)[4, 4] == ((2 << 16) | 4)
    assert np.array_equal(two_pass_field(m, 3), sr.edge_field_pair(m, 3))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _pose_err(pose, gt):
    """a pose distance without a model: the mean displacement of the ellipsoid's six axis ends"""
    ends = np.concatenate([np.diag(AXES), -np.diag(AXES)])
    return sr.add_error(pose, gt, ends)


def _pairs(H, W, n, seed):
    """n pairs at H x W: the ellipsoid near the frame's middle, the input pose 3-4 degrees and about a centimetre off; every pair but
    the first has its own K -> K0 (3,3), K_per_sample (n,9), pose_gt, pose_in (n,3,4) float32"""
    rng = np.random.default_rng(seed)
    K0 = np.array([[1.7 * W, 0, 0.5 * W - 0.3], [0, 1.7 * W, 0.5 * H + 0.2], [0, 0, 1]], np.float32)
    Ks, gts, inits = [], [], []
    for b in range(n):
        K = K0.copy()
        if b > 0:
            K[0, 0] *= 1.0 + 0.03 * b
            K[1, 1] *= 1.0 - 0.02 * b
            K[0, 2] += 1.5 * b
            K[1, 2] -= 1.0 * b
        R = _rot(rng.uniform(0, 360), rng.normal(size=3))
        gt = np.concatenate([R, np.array([[rng.uniform(-0.03, 0.03)], [rng.uniform(-0.02, 0.02)], [rng.uniform(0.95, 1.05)]])], axis=1)
        dR = _rot(rng.uniform(3.0, 4.0), rng.normal(size=3))
        init = np.concatenate([dR @ gt[:, :3], gt[:, 3:] + rng.normal(0, [0.008, 0.008, 0.01])[:, None]], axis=1).astype(np.float32)
        Ks.append(K.reshape(9))
        gts.append(gt.astype(np.float32))
        inits.append(init)
    return K0, np.stack(Ks).astype(np.float32), np.stack(gts), np.stack(inits)


def _depth(pose, K, H, W):
    return ellipsoid_render(pose, K, H, W, axes=AXES)[1]


def polish(pose_in, Ks, field, H, W, rounds, iters, huber, gate):
    """the Refiner's rounds on the restatement: render the depth at the current pose, refine from it -> pose, stats (B, rounds*iters, 2),
    status (B,)"""
    B = pose_in.shape[0]
    pose, stats, status = pose_in, [], np.zeros(B, np.int32)
    for _ in range(rounds):
        d = np.stack([_depth(pose[b], Ks[b], H, W) for b in range(B)])
        pose, st, flag = sr.sil_refine(d, field, pose, Ks, iters, huber, gate)
        stats.append(st)
        status |= flag
    return pose, np.concatenate(stats, axis=1), status


@functools.lru_cache(maxsize=None)
def convergence_scene():
    H, W, B = 120, 160, 4
    K0, Ks, gt, init = _pairs(H, W, B, 13)
    mask = np.stack([(_depth(gt[b], Ks[b], H, W) > 0).astype(np.float32) for b in range(B)])
    return H, W, Ks, gt, init, mask


def test_restatement_converges():
    H, W, Ks, gt, init, mask = convergence_scene()
    rounds, iters = 3, 4
    field = sr.edge_field(mask, 12)
    pose, stats, status = polish(init, Ks, field, H, W, rounds, iters, 2.0, 12.0)
    assert status.tolist() == [0] * len(init)
    for b in range(len(init)):
        before, after = _pose_err(init[b], gt[b]), _pose_err(pose[b], gt[b])
        rms = stats[b, ::iters, 1]      # at the start of every round
        print("pair", b, "rms at the start of a round (px)", np.round(rms, 3), "points", stats[b, ::iters, 0], "axis ends (mm)",
              round(1e3 * before, 2), "->", round(1e3 * after, 2))
        assert stats[b, :, 0].min() >= sr.MIN_POINTS
        assert np.all(np.diff(rms) < 0), (b, rms)           # the contour distance falls from round to round
        assert stats[b, -1, 1] < stats[b, 0, 1]
        assert after < before, (b, before, after)


def test_negative_control_gate_below_the_contour_distance():
    """a gate of a quarter pixel on the pairs that start 2.6-2.9 pixels rms off (pair 0 starts at 0.86 with a good part of its outline
    already on the edge): only the few points where the two outlines cross pass it, every pair is flagged in every iteration and keeps
    its pose bit for bit"""
    H, W, Ks, gt, init, mask = convergence_scene()
    far = slice(1, 4)
    field = sr.edge_field(mask[far], 12)
    first = polish(init[far], Ks[far], field, H, W, 1, 1, 2.0, 12.0)[1]
    assert np.all(first[:, 0, 1] > 2.0)      # the contour distance the gate lies below
    pose, stats, status = polish(init[far], Ks[far], field, H, W, 2, 3, 0.25, 0.25)
    print("points within a quarter pixel", stats[:, :, 0])
    assert status.tolist() == [sr.STATUS_SIL_FEW_POINTS] * 3
    assert np.array_equal(pose.view(np.uint32), init[far].view(np.uint32))
    assert stats[:, :, 0].max() < sr.MIN_POINTS


def test_contour_points_rules():
    d = np.zeros((9, 11), np.float32)
    d[0:5, 6:11] = 1.0                       # cut by the top and the right side of the frame
    K = np.array([[20.0, 0, 5.0], [0, 20.0, 4.0], [0, 0, 1]], np.float32)
    p0, px = sr.contour_points(d, K)
    want = {(6, y) for y in range(5)} | {(x, 4) for x in range(6, 11)}
    assert {tuple(p) for p in px.tolist()} == want
    assert np.allclose(p0[0], [(px[0][0] - 5.0) / 20.0, (px[0][1] - 4.0) / 20.0, 1.0])
    # the box restricts the points, not the neighbours they look at: column 8 alone has its contour pixel in row 4 only
    p0, px = sr.contour_points(d, K, [8, 8, -3, 30])
    assert px.tolist() == [[8, 4]]
    assert len(sr.contour_points(d, K, [11, -1, 9, -1])[0]) == 0       # the render's empty box
    bad = K.copy()
    bad[0, 0] = -20.0
    assert len(sr.contour_points(d, bad)[0]) == 0
    d[2, 8] = np.nan                        # not > 0: a hole, its four neighbours become contour pixels
    assert {tuple(p) for p in sr.contour_points(d, K)[1].tolist()} == want | {(8, 1), (8, 3), (7, 2), (9, 2)}


# ------------------------------------------------------------------------------------------------------------------ config
def test_config_defaults_and_yaml_merge(tmp_path):
    from deepim.config.config import config, reset_config, update_config

    reset_config()
    T = config.TEST
    assert (T.SIL_ITER, T.SIL_ROUNDS, T.SIL_HUBER_PX, T.SIL_MAX_PX, T.SIL_MASK) == (0, 2, 2.0, 12.0, "observed")
    p = tmp_path / "sil.yaml"
    p.write_text("TEST:\n  SIL_ITER: 5\n  SIL_ROUNDS: 3\n  SIL_MAX_PX: 9.0\n  SIL_MASK: pred\n  test_iter: 4\n")
    update_config(str(p))
    assert (T.SIL_ITER, T.SIL_ROUNDS, T.SIL_HUBER_PX, T.SIL_MAX_PX, T.SIL_MASK, T.test_iter) == (5, 3, 2.0, 9.0, "pred", 4)
    reset_config()
    assert config.TEST.SIL_ITER == 0


def test_shipped_yamls():
    from deepim.config.config import config, reset_config, update_config
    from deepim.core.tester import sil_settings

    cfgs = os.path.join(ROOT, "mx-deepim_amd", "experiments", "deepim", "cfgs")
    reset_config()
    update_config(os.path.join(cfgs, "deepim_hip_LM_ape_test.yaml"))
    assert config.TEST.SIL_ITER == 0 and sil_settings(config)[0] == 0
    base = {k: v for k, v in config.TEST.items() if not k.startswith("SIL_")}
    network = dict(config.network)
    reset_config()
    update_config(os.path.join(cfgs, "deepim_hip_LM_ape_test_sil.yaml"))
    assert sil_settings(config) == (6, 2, 2.0, 12.0, "observed")
    assert {k: v for k, v in config.TEST.items() if not k.startswith("SIL_")} == base   # the ape test config plus the new keys
    assert {k: np.asarray(v).tolist() for k, v in config.network.items()} == {k: np.asarray(v).tolist() for k, v in network.items()}
    reset_config()


def test_sil_settings_refusals():
    from deepim.config.config import config, reset_config
    from deepim.core.tester import refuse_at_source_size, sil_settings

    reset_config()
    assert sil_settings(config) == (0, 2, 2.0, 12.0, "observed")
    bad = {"SIL_ITER": [-1, 2.5, True], "SIL_ROUNDS": [0, 9, 1.5, True], "SIL_HUBER_PX": [0.0, -1.0, float("nan"), float("inf")],
           "SIL_MAX_PX": [1.5, 64.5, float("nan"), float("inf")], "SIL_MASK": ["rendered", 1, None]}
    for key, values in bad.items():
        for v in values:
            reset_config()
            config.TEST[key] = v
            with pytest.raises(ValueError, match="TEST." + key):
                sil_settings(config)
    reset_config()
    config.TEST.SIL_MAX_PX = 64.0
    config.TEST.SIL_HUBER_PX = 64.0
    assert sil_settings(config)[2:4] == (64.0, 64.0)
    for key, v in (("HYP_NUM", 4), ("COARSE_VIEWS", 42)):
        reset_config()
        config.TEST[key] = v
        assert sil_settings(config)[0] == 0           # fine while the stage is off
        config.TEST.SIL_ITER = 6
        with pytest.raises(ValueError, match="TEST.SIL_ITER.*TEST." + key):
            sil_settings(config)
    # SIL_MASK 'pred': the mask head of the full graph
    for pred_mask, fast, ok in ((True, False, True), (True, True, False), (False, False, False)):
        reset_config()
        config.TEST.SIL_MASK = "pred"
        config.network.PRED_MASK = pred_mask
        config.TEST.FAST_TEST = fast
        assert sil_settings(config)[0] == 0
        config.TEST.SIL_ITER = 6
        if ok:
            assert sil_settings(config) == (6, 2, 2.0, 12.0, "pred")
        else:
            with pytest.raises(ValueError, match="TEST.SIL_ITER.*TEST.SIL_MASK"):
                sil_settings(config)
    reset_config()
    config.TEST.SIL_ITER = 6
    assert sil_settings(config) == (6, 2, 2.0, 12.0, "observed")
    refuse_at_source_size(config, (480, 640))
    with pytest.raises(ValueError, match="TEST.SIL_ITER"):
        refuse_at_source_size(config, (960, 1280))
    reset_config()


# ------------------------------------------------------------------------------------------------------------------ C ABI, host side
def test_header_defines_the_status_bit():
    text = open(HEADER).read()
    assert "#define DIM_STATUS_SIL_FEW_POINTS 2048" in text
    assert sr.STATUS_SIL_FEW_POINTS == 2048
    from lib.hip import ops

    assert ops.STATUS_SIL_FEW_POINTS == 2048


def test_workspace_bytes(hip_lib):
    per_pair = (16 + 16 * 32) * 8     # T state + 16 workgroup partials of 32 doubles, as the header states
    for B, H, W in ((1, 480, 640), (16, 480, 640), (3, 48, 64), (2, 61, 83)):
        assert hip_lib.dim_sil_workspace_bytes(B, H, W) == B * per_pair
    assert hip_lib.dim_sil_workspace_bytes(0, 480, 640) == 0 and hip_lib.dim_sil_workspace_bytes(-2, 480, 640) == 0


def test_bad_arguments_return_err_arg_without_a_device(hip_lib):
    K9 = (ctypes.c_float * 9)(572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is enqueued

    def field(B=2, H=480, W=640, radius=12, mask=fake, out=fake):
        return hip_lib.dim_sil_edge_field(mask, B, H, W, radius, out, None)

    cases = {"B=0": dict(B=0), "B<0": dict(B=-1), "radius=0": dict(radius=0), "radius<0": dict(radius=-3), "radius=65": dict(radius=65),
             "H=2": dict(H=2), "W=2": dict(W=2), "H=32768": dict(H=32768), "W=32768": dict(W=32768), "mask": dict(mask=None),
             "field": dict(out=None)}
    for name, kw in cases.items():
        assert field(**kw) == -1, name
        assert hip_lib.dim_last_error().decode().startswith("sil_edge_field"), name

    def refine(B=2, H=480, W=640, iters=6, huber=2.0, gate=12.0, dr=fake, fl=fake, pose=fake, k9=K9, ws=fake, out=fake):
        return hip_lib.dim_sil_refine(dr, fl, None, pose, k9, None, B, H, W, iters, huber, gate, ws, out, None, None, None)

    cases = {"B=0": dict(B=0), "B<0": dict(B=-3), "iters<0": dict(iters=-1), "huber=0": dict(huber=0.0), "huber<0": dict(huber=-1.0),
             "huber=nan": dict(huber=float("nan")), "gate<huber": dict(gate=1.5), "gate=nan": dict(gate=float("nan")), "H=2": dict(H=2),
             "W=2": dict(W=2), "depth_rendered": dict(dr=None), "field": dict(fl=None), "pose_in": dict(pose=None), "K9": dict(k9=None),
             "workspace": dict(ws=None), "pose_out": dict(out=None)}
    for name, kw in cases.items():
        assert refine(**kw) == -1, name
        assert hip_lib.dim_last_error().decode().startswith("sil_refine"), name


# ------------------------------------------------------------------------------------------------------------------ pred_eval
class _FakeNet(object):
    device = "cpu"


class _FakeRefiner(object):
    """stands in for deepim.core.tester.Refiner: fixed poses per batch on CPU tensors"""

    def __init__(self, B, poses_iter, poses_sil, sil):
        self.B, self.net = B, _FakeNet()
        self._poses, self._sil = list(poses_iter), list(poses_sil)
        self.sil = sil
        self.pose_sil = None

    def load(self, image_observed, image_rendered, mask_observed, mask_rendered, src_pose, class_index, depth_observed=None,
             depth_rendered=None, K=None):
        self.pose_sil = torch.from_numpy(self._sil.pop(0)) if self.sil else None
        self._cur = torch.from_numpy(self._poses.pop(0))

    def refine(self):
        return self._cur


def _fake_run(sil, n_batches=2, B=4, test_iter=3, **test_keys):
    from deepim.core.tester import pred_eval
    from lib.dataset.evaluation import PoseEvaluator
    from lib.utils import synthetic as syn
    from scene import make_test_config

    cfg = make_test_config(test_iter=test_iter)
    cfg.dataset.class_name = ["ape", "cat"]
    cfg.TEST.SIL_ITER = 6 if sil else 0
    cfg.TEST.update(test_keys)
    rng = np.random.default_rng(5)
    pts = {c: rng.uniform(-0.05, 0.05, size=(200, 3)) for c in cfg.dataset.class_name}
    ev = PoseEvaluator(cfg.dataset.class_name, pts, {c: 0.15 for c in cfg.dataset.class_name})
    batches, iters, polished = [], [], []
    for k in range(n_batches):
        cls, gt, init = syn.sample_pairs(100 + k, B, n_classes=2)
        init = init.copy()
        if k == 1:
            init[2] = -1.0   # undetected
        iters.append(np.stack([gt + rng.normal(0, 0.02 / (it + 1), gt.shape).astype(np.float32) for it in range(test_iter)]).astype(np.float32))
        polished.append((gt + rng.normal(0, 0.001, gt.shape)).astype(np.float32))
        z = torch.zeros((B, 1, 4, 4))
        batches.append({"image_observed": z, "image_rendered": z, "mask_observed": z, "mask_rendered": z, "src_pose": torch.from_numpy(init),
                        "class_index": torch.from_numpy(cls), "pose_observed": torch.from_numpy(gt)})
    out = pred_eval(cfg, _FakeRefiner(B, iters, polished, sil), batches, ev)
    return cfg, out


def test_pred_eval_scores_sil_as_one_row_table():
    from test_icp_host import _same

    _, off = _fake_run(False)
    assert "sil" not in off
    cfg, on = _fake_run(True)
    assert int(cfg.TEST.test_iter) == 3   # the one-row scoring does not touch the config
    _same({k: v for k, v in on.items() if k != "sil"}, off)
    sl = on["sil"]
    assert set(sl) >= {"pose", "add", "arp_2d"}
    assert sl["pose"]["rot_acc"].shape == (2, 1, 10) and len(sl["pose"]["overall"]) == 1
    assert len(sl["add"]["overall"]) == 1 and len(sl["arp_2d"]["overall"]) == 1
    rot = [r for c in range(2) for r in sl["all_rot_err"][c][0]]
    assert len(rot) == 8 and sorted(rot)[-1] == 1000 and sorted(rot)[-2] < 10    # one undetected pair, scored as the loop scores it
    assert sl["add"]["overall"][0]["0.02"] >= on["add"]["overall"][2]["0.02"]
    assert sl["add"]["overall"][0]["auc"] > on["add"]["overall"][2]["auc"]
    cfg.TEST.SIL_ITER = 0


@pytest.mark.parametrize("key", ["VSD", "BOP"])
def test_pred_eval_refuses_sil_with_vsd_or_bop(key):
    with pytest.raises(ValueError, match="TEST.SIL_ITER"):
        _fake_run(True, **{key: True})
    from deepim.config.config import reset_config

    reset_config()


# ------------------------------------------------------------------------------------------------------------------ small frames
GPU_ITERS = (1, 4)


def _small_batch(H, W, n, seed):
    K0, Ks, gt, init = _pairs(H, W, n, seed)
    depth = np.stack([_depth(init[b], Ks[b], H, W)[None] for b in range(n)])
    mask = np.stack([(_depth(gt[b], Ks[b], H, W) > 0).astype(np.float32)[None] for b in range(n)])
    return {"H": H, "W": W, "K": K0, "K_per_sample": Ks, "pose_gt": gt, "pose_in": init, "depth_rendered": depth, "mask": mask}


def _tight_boxes(depth):
    out = []
    for d in depth[:, 0]:
        ys, xs = np.nonzero(d > 0)
        out.append([xs.min(), xs.max(), ys.min(), ys.max()])
    return np.asarray(out, np.int32)


@functools.lru_cache(maxsize=None)
def gpu_batches():
    """the small-frame inputs of tests/test_gpu_sil.py: B = 3 at 48x64 and B = 2 at 61x83 (W % 4 != 0).  Per batch a dict of numpy
    arrays: depth_rendered (B,1,H,W) at pose_in, mask (B,1,H,W) = the render at pose_gt, K (the first pair's, the call's K9),
    K_per_sample (B,9), bbox (B,4) int32 and field (B,H,W) int32 = the restatement's field of the mask at RADIUS.
    48x64: pair 1's box reaches past the frame on three sides (clipped like clamp_bbox); pair 2's box is the left third of its
    render, which holds fewer than 64 contour pixels (flagged with the box, not without)."""
    a = _small_batch(48, 64, 3, 11)
    box = _tight_boxes(a["depth_rendered"])
    box[1] = [-6, 70, -3, box[1][3]]
    box[2][1] = box[2][0] + (box[2][1] - box[2][0]) // 3
    a["bbox"] = box
    b = _small_batch(61, 83, 2, 12)
    b["bbox"] = _tight_boxes(b["depth_rendered"])
    for g in (a, b):
        g["field"] = sr.edge_field(g["mask"], RADIUS)
    return a, b


@functools.lru_cache(maxsize=None)
def gpu_reference(which, iters, with_bbox=True, per_sample=True):
    """the restatement on gpu_batches()[which]: pose, stats, status, per-pair extras (contour points, decision margins); computed once
    per case.  per_sample False: pair 0's camera for every pair, as the call's host K9"""
    g = gpu_batches()[which]
    return sr.sil_refine(g["depth_rendered"], g["field"], g["pose_in"], g["K_per_sample"] if per_sample else g["K"], iters, HUBER, GATE,
                         bbox=g["bbox"] if with_bbox else None, with_extra=True)


def gpu_cases():
    """(which, iters, with_bbox, per_sample) of every comparison tests/test_gpu_sil.py makes on the small frames"""
    out = [(which, iters, with_bbox, True) for which in (0, 1) for iters in GPU_ITERS for with_bbox in (True, False)]
    return out + [(which, GPU_ITERS[-1], True, False) for which in (0, 1)]


def test_gpu_batches_are_sound():
    """equal counts are a fair demand on the device only when no decision of the restatement hangs on the last bits: in every
    iteration no projected point lies within 1e-6 px of a rounding boundary, no distance within 1e-6 of the Huber knee or the gate"""
    a, b = gpu_batches()
    assert (a["H"], a["W"], len(a["pose_in"])) == (48, 64, 3) and (b["H"], b["W"], len(b["pose_in"])) == (61, 83, 2) and b["W"] % 4
    for g in (a, b):
        B = len(g["pose_in"])
        assert g["depth_rendered"].shape == (B, 1, g["H"], g["W"]) and g["field"].shape == (B, g["H"], g["W"])
        assert np.array_equal(g["K_per_sample"][0].reshape(3, 3), g["K"]) and not np.array_equal(g["K_per_sample"][1], g["K_per_sample"][0])
        assert np.array_equal(g["field"], np.stack([two_pass_field(m[0], RADIUS) for m in g["mask"]]))
    assert a["bbox"][1][0] < 0 and a["bbox"][1][1] > a["W"] - 1 and a["bbox"][1][2] < 0   # clipped by the frame
    for which, iters, with_bbox, per_sample in gpu_cases():
        g = gpu_batches()[which]
        pose, stats, status, extra = gpu_reference(which, iters, with_bbox, per_sample)
        for p in range(len(pose)):
            mg = extra[p]["margin"]
            print(which, iters, with_bbox, per_sample, p, "contour points", extra[p]["points"], "counts", stats[p, :, 0], "rms",
                  np.round(stats[p, :, 1], 3), "margins", mg)
            assert mg["round"] > 1e-6 and mg["huber"] > 1e-6 and mg["gate"] > 1e-6, (which, iters, with_bbox, per_sample, p, mg)
            if which == 0 and with_bbox and p == 2:   # the small window
                assert 0 < extra[p]["points"] < sr.MIN_POINTS and status[p] == sr.STATUS_SIL_FEW_POINTS
                assert np.array_equal(pose[p].view(np.uint32), g["pose_in"][p].view(np.uint32))
            else:
                assert status[p] == 0 and stats[p, :, 0].min() >= sr.MIN_POINTS
                assert not np.array_equal(pose[p], g["pose_in"][p])
                if iters > 1:
                    assert stats[p, -1, 1] < stats[p, 0, 1]
    # the box that reaches past the frame selects what the whole frame does
    with_box, without = gpu_reference(0, 4, True), gpu_reference(0, 4, False)
    assert np.array_equal(with_box[0][1], without[0][1]) and np.array_equal(with_box[1][1], without[1][1])
