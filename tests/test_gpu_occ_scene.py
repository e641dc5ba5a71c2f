"""Occluded, lit multi-object training scenes on the device: dim_scene_compose against the plain-loop restatement (bit-equal: the
kernel only selects and counts), the LINEMOD light rule of the rasteriser, and the batch builder that uses both."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import occ_scene_reference as ref  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402
from oracle import native  # noqa: E402

DEV = "cuda:0"
N = 3
# 24x36: 16-byte path, one workgroup; 23x37: one pixel per thread, odd tail; 40x52: 520 quads = 3 workgroups add into one count
SIZES = [(24, 36), (23, 37), (40, 52)]
OUTS = ["scene_bgr", "scene_depth", "scene_label", "vis_mask", "counts", "vis_bbox"]
_cache = {}


def make_layers(S, H, W):
    """N scenes of S layers: overlapping random blobs with sloped depth, plus (where S allows) an exact depth tie between two slots, an
    unused slot in the middle, a layer wholly hidden, an empty layer, and NaN / negative / infinite depth values."""
    rng = np.random.default_rng(100 * S + H)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.zeros((N, S, H, W), np.float32)
    bgr = rng.integers(1, 256, size=(N, S, H, W, 3)).astype(np.float32)
    label = rng.integers(1, 9, size=(N, S)).astype(np.int32)
    for n in range(N):
        for s in range(S):
            cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = rng.uniform(0.2, 0.5) * H, rng.uniform(0.2, 0.5) * W
            blob = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
            z = rng.uniform(0.5, 1.5) + 0.01 * (xx - cx) / W + 0.02 * (yy - cy) / H
            depth[n, s][blob] = z.astype(np.float32)[blob]
    if S >= 2:
        depth[0, 1, 2:H // 2, 3:W // 2] = depth[0, 0, 2:H // 2, 3:W // 2] = 0.4           # exact ties between slots 0 and 1, in front
        depth[2, 0] = 0.0
        depth[2, 0, 4:H - 4, 4:W - 4] = 0.3                                               # scene 2: slot 0 in front of ...
        depth[2, 1] = np.where(depth[2, 0] > 0, 2.0, 0.0)                                 # ... slot 1, which is wholly hidden
        for s in range(2, S):
            depth[2, s] = np.maximum(depth[2, s], np.where(depth[2, s] > 0, 0.31, 0.0))   # (nothing else in front of slot 0)
    if S >= 3:
        label[1, S // 2] = 0                                                              # an unused slot in the middle ...
        depth[1, S // 2] = 0.01                                                           # ... that would win everywhere
        label[0, 2] = -3                                                                  # (negative labels are unused too)
        depth[1, S - 1] = 0.0                                                             # an empty layer
    depth[0, 0, 0, 0] = np.nan
    depth[0, 0, 0, 1] = -0.5
    depth[0, 0, 1, 0] = np.inf
    depth[1, S - 1 if S < 3 else 0, H - 1, W - 1] = np.nan
    depth[1, 0, H - 1, W - 2] = -np.inf
    return bgr.reshape(N * S, H, W, 3), depth.reshape(N * S, 1, H, W), label.reshape(N * S)


def case(S, H, W):
    """inputs and the reference result, computed once per shape and shared (never modified)"""
    if (S, H, W) not in _cache:
        bgr, depth, label = make_layers(S, H, W)
        _cache[(S, H, W)] = (bgr, depth, label, ref.compose(bgr, depth, label, S))
    return _cache[(S, H, W)]


def garbage_outputs(S, H, W, skip=None):
    g = torch.Generator(device=DEV)
    g.manual_seed(S + H)
    shapes = {"scene_bgr": (N, H, W, 3), "scene_depth": (N, 1, H, W), "scene_label": (N, 1, H, W), "vis_mask": (N * S, 1, H, W)}
    out = {k: torch.randn(v, generator=g, device=DEV) * 1e6 for k, v in shapes.items()}
    out["counts"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (N * S, 2), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    out["vis_bbox"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (N * S, 4), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    if skip:
        out[skip] = None
    return out


def garbage_workspace(S, H, W):
    from lib.hip import ops

    ws = ops.scene_compose_workspace(N, S, H, W, DEV)
    ws.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, ws.shape, device=DEV, dtype=torch.int64).to(torch.int32))
    return ws


def assert_bits(got, want, name):
    a, b = got.cpu().numpy(), want
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (name, int((a != b).sum()))


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("S", [1, 2, 3, 8, 16])
def test_compose_bit_equal_to_restatement(hip_lib, S, H, W):
    from lib.hip import ops

    bgr, depth, label, want = case(S, H, W)
    if S >= 3:   # the case holds what it claims to
        assert want["counts"][1 * S + S // 2].tolist() == [0, 0] and want["counts"][1 * S + S - 1].tolist() == [0, 0]
    if S >= 2:
        assert want["counts"][2 * S + 1, 0] > 0 and want["counts"][2 * S + 1, 1] == 0
        assert want["vis_mask"][0][0, 2:H // 2, 3:W // 2].all() and not want["vis_mask"][1][0, 2:H // 2, 3:W // 2].any()
    t = [torch.from_numpy(x).to(DEV) for x in (bgr, depth, label)]
    status = torch.zeros(N * S, dtype=torch.int32, device=DEV)
    out = garbage_outputs(S, H, W)
    # the workspace: exactly dim_scene_compose_workspace_bytes between guards, at the documented minimum alignment (4 mod 8), NaN bits
    work = guard_arena.workspace(ops.lib().dim_scene_compose_workspace_bytes(N, S, H, W), 4, DEV)
    ops.scene_compose(t[0], t[1], t[2], S, status=status, workspace=work.view(), **out)
    work.check("dim_scene_compose workspace, S = {}, {} x {}".format(S, H, W))
    for k in OUTS:
        assert_bits(out[k], want[k], k)
    hidden = (label > 0) & (want["counts"][:, 1] == 0)
    np.testing.assert_array_equal(status.cpu().numpy(), np.where(hidden, 256, 0))
    # a second run over other garbage: identical bits
    again = garbage_outputs(S, H, W)
    for v in again.values():
        v.neg_()
    ops.scene_compose(t[0], t[1], t[2], S, workspace=garbage_workspace(S, H, W).neg_(), **again)
    for k in OUTS:
        assert_bits(again[k], out[k].cpu().numpy(), k)


@pytest.mark.parametrize("H,W", SIZES[:2])
def test_compose_each_output_null_in_turn(hip_lib, H, W):
    from lib.hip import ops

    S = 3
    bgr, depth, label, want = case(S, H, W)
    t = [torch.from_numpy(x).to(DEV) for x in (bgr, depth, label)]
    for skip in OUTS:
        out = garbage_outputs(S, H, W, skip=skip)
        ops.scene_compose(t[0], t[1], t[2], S, workspace=garbage_workspace(S, H, W), **out)
        for k in OUTS:
            if k != skip:
                assert_bits(out[k], want[k], "{} without {}".format(k, skip))
    # no colour output: the layer colours are not needed either; no counts / boxes / status: neither is the workspace
    out = garbage_outputs(S, H, W)
    ops.scene_compose(None, t[1], t[2], S, scene_depth=out["scene_depth"], scene_label=out["scene_label"])
    assert_bits(out["scene_depth"], want["scene_depth"], "scene_depth")
    assert_bits(out["scene_label"], want["scene_label"], "scene_label")


def test_compose_replayed_from_a_captured_graph(hip_lib):
    from lib.hip import ops

    S, (H, W) = 3, SIZES[2]
    bgr, depth, label, want = case(S, H, W)
    t = [torch.from_numpy(x).to(DEV) for x in (bgr, depth, label)]
    out, ws = garbage_outputs(S, H, W), garbage_workspace(S, H, W)
    call = lambda: ops.scene_compose(t[0], t[1], t[2], S, workspace=ws, **out)  # noqa: E731
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for v in out.values():
            v.fill_(-7)
        ws.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for k in OUTS:
            assert_bits(out[k], want[k], k)


def test_compose_bad_arguments(hip_lib):
    from lib.hip import ops

    S, (H, W) = 2, SIZES[0]
    bgr, depth, label, _ = case(S, H, W)
    t = [torch.from_numpy(x).to(DEV) for x in (bgr, depth, label)]
    out = garbage_outputs(S, H, W)
    ws = ops.scene_compose_workspace(N, 16, H, W, DEV)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    call = lambda d, s: hip_lib.dim_scene_compose(P(t[0]), d, P(t[2]), N, s, H, W, P(ws), P(out["scene_bgr"]), P(out["scene_depth"]),  # noqa: E731
                                                  P(out["scene_label"]), None, None, None, None, None)
    keep = out["scene_depth"].clone()
    assert call(P(t[1]), 0) == -1 and b"S must be" in hip_lib.dim_last_error()
    assert call(P(t[1]), 17) == -1 and b"S must be" in hip_lib.dim_last_error()
    assert call(None, S) == -1 and b"null pointer" in hip_lib.dim_last_error()
    torch.cuda.synchronize()
    assert torch.equal(keep, out["scene_depth"])   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- light model
LH, LW = 48, 64
LK = np.array([[110.0, 0, 31.5], [0, 110.0, 23.5], [0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def light_scene():
    """a small procedural mesh at 48x64 under both render machines, one unlit render and the pieces the cases share"""
    from lib.render_hip.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi, vertex_normals
    from lib.render_hip.render_py_light_multi_program import Render_Py_Light_MultiProgram
    from lib.render_hip.render_py_multi import Render_Py

    rng = np.random.default_rng(21)
    v, t, f = syn.make_mesh(rng, subdiv=2, diameter=0.15)   # ~30 px across at 0.5 m
    tex = syn.make_texture(rng)
    nrm = vertex_normals(v, f).astype(np.float32)
    ratios = [0.4, 1.0, 0.7]
    lm = Render_Py_Light_MultiProgram(["__background__", "obj"], None, LK, LW, LH, 0.25, 6.0, ratios, meshes=[(v, nrm, t, f, tex)])
    mn = Render_Py_Light_ModelNet_Multi(None, tex, LK, LW, LH, 0.25, 6.0, brightness_ratios=ratios, meshes=[(v, nrm, t, f)])
    un = Render_Py(None, ["obj"], LK, LW, LH, 0.25, 6.0, meshes=[(v, t, f, tex)])
    rng = np.random.default_rng(4)
    pose = np.concatenate([syn.random_rotation(rng), np.array([[0.01], [-0.02], [0.5]])], axis=1).astype(np.float32)
    lp = native.modelnet_light_position(pose.astype(np.float64), idx=1).astype(np.float32)
    return dict(mesh=(v, nrm, t, f, tex), lm=lm, mn=mn, un=un, pose=pose, lp=lp)


def _render(rm, sc, inten=None, k=0):
    cls = torch.zeros(1, dtype=torch.int32, device=DEV)
    pose = torch.from_numpy(sc["pose"][None]).to(DEV)
    bgr = torch.empty((1, LH, LW, 3), device=DEV)
    depth = torch.empty((1, 1, LH, LW), device=DEV)
    if inten is None:
        rm.render_batch(cls, pose, bgr=bgr, depth=depth)
    else:
        rm.render_batch(cls, pose, torch.from_numpy(sc["lp"][None]).to(DEV), torch.tensor([inten], dtype=torch.float32, device=DEV),
                        brightness_k=k, bgr=bgr, depth=depth)
    return bgr[0].cpu().numpy(), depth[0, 0].cpu().numpy()


def test_lm_rule_equals_modelnet_rule_for_white_light_or_ratio_one(hip_lib, light_scene):
    sc = light_scene
    a, da = _render(sc["lm"], sc, [1.0, 1.0, 1.0], k=0)
    b, db = _render(sc["mn"], sc, [1.0, 1.0, 1.0], k=0)
    assert (da > 0).sum() > 200 and a[da > 0].std() > 3.0
    assert a.tobytes() == b.tobytes() and da.tobytes() == db.tobytes()
    a, _ = _render(sc["lm"], sc, [0.3, 0.9, 1.2], k=1)   # ratio 1: no ambient term left
    b, _ = _render(sc["mn"], sc, [0.3, 0.9, 1.2], k=1)
    assert a.tobytes() == b.tobytes() and a[da > 0].std() > 3.0


def test_lm_rule_blue_light_keeps_the_ambient_term(hip_lib, light_scene):
    """I = (0,0,1), r = 0.4: R and G get no diffuse light, so they are round(0.6 * texel) of the unlit render, within one grey level;
    the ModelNet rule multiplies the whole sum by I and gives 0 there"""
    sc = light_scene
    lit, d = _render(sc["lm"], sc, [0.0, 0.0, 1.0], k=0)
    unlit, du = _render(sc["un"], sc)
    mn, _ = _render(sc["mn"], sc, [0.0, 0.0, 1.0], k=0)
    cov = d > 0
    assert cov.sum() > 200 and np.array_equal(cov, du > 0)
    for ch in (1, 2):   # bgr: G and R
        want = np.floor(np.float32(0.6) * unlit[..., ch][cov] + 0.5)
        err = np.abs(lit[..., ch][cov] - want)
        print("channel {}: max |lit - round(0.6 texel)| = {}".format(ch, err.max()))
        assert err.max() <= 1.0
        assert (mn[..., ch][cov] == 0).all()
        assert want.min() > 0
    assert lit[..., 0][cov].std() > 3.0   # B carries the shading


def lm_as_modelnet(ratio, ic):
    """(r', I') in float32 with texel * ((1-r') + r' b) * I' = texel * ((1-r) + r b ic): I' = (1-r) + r ic, r' = r ic / I'.
    Where the surface faces away from the light b is exactly 0 and the colour is texel * (1-r), which lands exactly on a half grey
    level for some texels (r = 0.7: every texel 5, 15, 25, ...); there the rounding of the ambient term alone decides the byte, so
    the pair is taken among the neighbouring floats such that the oracle's ambient term fl(fl(1 - r') * I') IS the shader's fl(1 - r),
    bit for bit.  The slope r' I' then differs from r ic by a few ulp, which moves a colour by ~1e-5 grey levels."""
    f = np.float32
    r, ic = f(ratio), f(ic)
    amb = f(1) - r
    i0 = f(amb + f(r * ic))
    r0 = f(f(r * ic) / i0)
    best = None
    for di in range(-16, 17):
        i2 = i0
        for _ in range(abs(di)):
            i2 = np.nextafter(i2, f(np.inf) if di > 0 else f(-np.inf))
        for dr in range(-16, 17):
            r2 = r0
            for _ in range(abs(dr)):
                r2 = np.nextafter(r2, f(np.inf) if dr > 0 else f(-np.inf))
            if 0 <= r2 <= 1 and f(f(f(1) - r2) * i2) == amb and (best is None or abs(di) + abs(dr) < best[0]):
                best = (abs(di) + abs(dr), float(r2), float(i2))
    assert best is not None, (ratio, ic)
    return best[1], best[2]


def lm_restatement(sc, inten, ratio):
    """The LINEMOD shader restated through the oracle's software rasteriser, the method of tests/test_gpu_render_lit.py: per channel c
    the rule texel * ((1-r) + r b I_c) is the ModelNet rule under (r', I') of lm_as_modelnet, so channel c of the oracle's render
    under (r', I') is the LINEMOD colour of that channel."""
    v, nrm, t, f, tex = sc["mesh"]
    out, depth = np.zeros((LH, LW, 3), np.float32), None
    for c in range(3):   # light_intensity is RGB, the image BGR
        r2, i2 = lm_as_modelnet(ratio, inten[c])
        bgr, depth = native.render_lit(v, nrm, t, f, tex, sc["pose"][:, :3], sc["pose"][:, 3], LK, sc["lp"], [i2, i2, i2], r2, H=LH, W=LW)
        out[..., 2 - c] = bgr[..., 2 - c]
    return out, depth


@pytest.mark.parametrize("inten,k", [([0.0, 0.0, 1.0], 0), ([1.15, 0.0, 0.85], 2), ([0.9, 1.2, 1.1], 0)])
def test_lm_rule_vs_shader_restatement(hip_lib, light_scene, inten, k):
    """tolerance of tests/test_gpu_render_lit.py: coverage within 4 pixels, depth 2e-6, integral grey levels within 1 (a rounding tie
    may fall the other way) and all but 1e-3 of them equal -- at 48x64 with ~500 covered pixels x 3 channels that allows one"""
    sc = light_scene
    ratio = sc["lm"].brightness_ratios[k]
    got, got_d = _render(sc["lm"], sc, inten, k=k)
    want, want_d = lm_restatement(sc, inten, ratio)
    cov = (got_d > 0) != (want_d > 0)
    assert cov.sum() <= 4, cov.sum()
    both = (got_d > 0) & (want_d > 0)
    assert both.sum() > 200
    np.testing.assert_allclose(got_d[both], want_d[both], rtol=2e-6)
    diff = np.abs(got[both] - want[both])
    print("max grey-level difference {}, share of unequal values {:.2e}".format(diff.max(), (diff > 0).mean()))
    assert diff.max() <= 1.0, diff.max()
    assert (diff > 0).mean() < 1e-3, (diff > 0).mean()
    assert want[both].std() > 3.0 and got[both].max() <= 255.0
    # the reference-signature single render returns the same picture as uint8
    img, d = sc["lm"].render(sc["pose"][:, :3], sc["pose"][:, 3], sc["lp"], inten, "obj", brightness_k=k, r_type="mat")
    assert img.dtype == np.uint8 and img.shape == (LH, LW, 3)
    np.testing.assert_array_equal(img.astype(np.float32), got)
    np.testing.assert_array_equal(d, got_d)


# -------------------------------------------------------------------------------------------------------------- batch builder
B_, K_ = 4, 3


@pytest.fixture(scope="module")
def built():
    """full-size batches, B = 4, k = 3 other-class distractors: today's batch, the occluded one, the lit occluded one, and one with a
    pair forced over the limit"""
    from lib.render_hip.render_py_light_multi_program import Render_Py_Light_MultiProgram
    from lib.render_hip.render_py_multi import Render_Py

    models = syn.make_models(seed=2333, n_models=4, subdiv=3)
    names = ["c{}".format(i) for i in range(4)]
    rm = Render_Py(None, names, syn.LINEMOD_K, meshes=models)
    lm = Render_Py_Light_MultiProgram(names, None, syn.LINEMOD_K, brightness_ratios=syn.LM_BRIGHTNESS_RATIOS,
                                      meshes=[(v, None, t, f, tex) for v, t, f, tex in models])
    kw = dict(models=models, n_classes=4)
    plain = syn.build_device_train_batch(rm, B_, 5, **kw)
    off = syn.build_device_train_batch(rm, B_, 5, occluders=0, lit=False, occ_max_rate=0.85, **kw)
    occ = syn.build_device_train_batch(rm, B_, 5, occluders=K_, **kw)
    lit = syn.build_device_train_batch(rm, B_, 5, occluders=K_, lit=True, light_machine=lm, **kw)
    # pair 1: its first distractor is the target's own mesh at the target's rotation, 20 % nearer on the same ray -- exactly in front
    cls, gt = plain["class_index"].cpu().numpy(), plain["pose_gt"].cpu().numpy()
    dc, dp = syn.sample_distractors(5 + 29, cls, gt, models, K_, n_classes=4)
    dc[1, 0] = cls[1]
    dp[1, 0] = gt[1]
    dp[1, 0, :, 3] *= 0.8
    forced = syn.build_device_train_batch(rm, B_, 5, occluders=K_, distractors=(dc, dp), **kw)
    return dict(rm=rm, lm=lm, models=models, plain=plain, off=off, occ=occ, lit=lit, forced=forced)


def test_builder_defaults_are_todays_batch(hip_lib, built):
    assert set(built["off"]) == set(built["plain"])
    for k, v in built["plain"].items():
        assert torch.equal(v, built["off"][k]), k
    assert "depth_observed" not in built["plain"] and "scene_label" not in built["plain"]


@pytest.mark.parametrize("which", ["occ", "lit"])
def test_builder_occluded_batch(hip_lib, built, which):
    b, plain = built[which], built["plain"]
    kept = b["occ_kept"].cpu().numpy()
    cnt = b["occ_counts"].cpu().numpy()
    target = (plain["class_index"] + 1).float().view(B_, 1, 1, 1)
    full_mask = plain["mask_gt_observed"]
    assert kept.any()
    print("{}: target pixels {} visible {} kept {}".format(which, cnt[:, 0], cnt[:, 1], kept))
    np.testing.assert_array_equal(cnt[:, 0], full_mask.sum(dim=(1, 2, 3)).cpu().numpy().astype(np.int64))
    # every kept pair is at most 85 % hidden: the rule itself, visible < (1 - 0.85) * full drops the pair
    np.testing.assert_array_equal(kept, ~(cnt[:, 1].astype(np.float64) < (1.0 - 0.85) * cnt[:, 0].astype(np.float64)))
    assert (cnt[kept, 1] >= 0.15 * cnt[kept, 0] - 1e-9).all()
    m = b["mask_gt_observed"]
    assert bool(((m == 1) | (m == 0)).all()) and bool((m <= full_mask).all())          # a subset of the unoccluded mask
    assert torch.equal(m, (b["scene_label"] == target).float())                        # = label == mask_idx
    assert float(m.sum()) < float(full_mask.sum())                                     # something is occluded
    for i in range(B_):
        if kept[i]:
            assert int(m[i].sum()) == cnt[i, 1]
    # the observed image equals the target layer wherever the target is visible; unlit, that layer is today's observed image
    if which == "occ":
        vis = (m > 0).expand(-1, 3, -1, -1)
        assert torch.equal(b["image_observed"][vis], plain["image_observed"][vis])
        bg = (b["scene_label"] == 0).expand(-1, 3, -1, -1)
        assert torch.equal(b["image_observed"][bg], plain["image_observed"][bg])       # and the same noise behind the scene
    else:
        lm, lp_draws = built["lm"], [syn.lm_light_draw((5, i), i, plain["pose_gt"][i].cpu().numpy(), 5) for i in range(B_)]
        bgr = torch.empty((B_, 480, 640, 3), device=DEV)
        lm.render_batch(plain["class_index"], plain["pose_gt"], torch.tensor(np.stack([d[0] for d in lp_draws]), dtype=torch.float32, device=DEV),
                        torch.tensor(np.stack([d[1] for d in lp_draws]), dtype=torch.float32, device=DEV), brightness_k=lp_draws[0][2], bgr=bgr)
        pm = torch.from_numpy(syn.plane_means()).to(DEV).view(1, 3, 1, 1)
        layer = bgr.permute(0, 3, 1, 2).flip(1) - pm
        vis = (m > 0).expand(-1, 3, -1, -1)
        assert torch.equal(b["image_observed"][vis], layer[vis])
        assert not torch.equal(b["image_observed"][vis], plain["image_observed"][vis])   # lit is not unlit
    # depth: the target's own layer stays in depth_gt_observed, the scene in depth_observed
    assert torch.equal(b["depth_gt_observed"], plain["depth_gt_observed"])
    vis1 = m > 0
    assert torch.equal(b["depth_observed"][vis1], plain["depth_gt_observed"][vis1])
    assert bool((b["depth_observed"][b["scene_label"] > 0] > 0).all())
    for k in ("image_rendered", "mask_rendered", "src_pose", "flow", "rot", "trans", "point_cloud_observed"):
        assert torch.equal(b[k], plain[k]), k


def test_builder_pair_over_the_limit_comes_back_unoccluded(hip_lib, built):
    b, plain, occ = built["forced"], built["plain"], built["occ"]
    kept = b["occ_kept"].cpu().numpy()
    cnt = b["occ_counts"].cpu().numpy()
    print("forced: target pixels {} visible {} kept {}".format(cnt[:, 0], cnt[:, 1], kept))
    assert not kept[1] and cnt[1, 1] < 0.15 * cnt[1, 0]
    assert torch.equal(b["image_observed"][1], plain["image_observed"][1])
    assert torch.equal(b["mask_gt_observed"][1], plain["mask_gt_observed"][1])
    assert torch.equal(b["depth_observed"][1], plain["depth_gt_observed"][1])
    for i in (0, 2, 3):   # the other pairs are those of the unforced batch
        assert torch.equal(b["image_observed"][i], occ["image_observed"][i])
        assert torch.equal(b["mask_gt_observed"][i], occ["mask_gt_observed"][i])


def test_builder_batch_trains(hip_lib, built):
    from deepim.core.module import MutableModule
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from scene import make_train_config

    cfg = make_train_config()
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=True)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    mod = MutableModule(cfg, params, B_)
    mod.forward_backward(built["lit"])
    assert torch.isfinite(mod.loss_sums).all(), mod.loss_sums
    assert float(mod.loss_sums.abs().sum()) > 0
