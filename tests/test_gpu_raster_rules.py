"""The rasteriser's pixel rules, held to equality on the hand-built scenes of tests/raster_rules_reference.py: 8-bit snapping, the top-left
rule, z ties to the lower face, the frame clamp and the dropped far-out face, per-fragment depth discard, both texel filters with the
flipped row, and the cut along the near plane.  Every exact scene is one class of one mesh table and one sample of one render_batch
(identity poses), through the one-pass resolve (30x37), the two-pass resolve (32x48), the two-pass resolve with a clean_bbox hint and
the two-pass render without colour.  Expected values come from `render_rules` (pinned to oracle/raster.c by
tests/test_raster_rules_host.py); no comparison leaves a pixel out, and apart from depth (rtol 2e-6, the suite's bar for rasteriser
depth) and the band of the near-plane cut every assert is an equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import raster_rules_reference as rr  # noqa: E402
from lib.utils import synthetic as syn  # noqa: E402
from oracle import native  # noqa: E402

DEV = "cuda:0"
SCENES = rr.exact_scenes()
NAMES = [s["name"] for s in SCENES]
B = len(SCENES)
PM = syn.plane_means()
COLOUR, PLAIN = ("image", "bgr"), ("depth", "mask", "bbox", "status")


def _machine(scenes, H, W, bil=False, K=rr.RK, znear=rr.ZNEAR, zfar=rr.ZFAR):
    from lib.render_hip.render_py_multi import Render_Py

    return Render_Py(None, [s["name"] for s in scenes], K, W, H, znear, zfar, meshes=[(s["verts"], s["uvs"], s["faces"], s["tex"]) for s in scenes],
                     tex_bilinear=bil)


def _planes(n, H, W, colour=True, aligned=True):
    """zeroed output planes; aligned=False shifts each by one float, which forces the one-pass resolve at any width"""
    def plane(*shape):
        if aligned:
            return torch.zeros(shape, dtype=torch.float32, device=DEV)
        return torch.zeros((int(np.prod(shape)) + 1,), dtype=torch.float32, device=DEV)[1:].view(*shape)

    o = {"depth": plane(n, 1, H, W), "mask": plane(n, 1, H, W), "bbox": torch.zeros((n, 4), dtype=torch.int32, device=DEV),
         "status": torch.zeros((n,), dtype=torch.int32, device=DEV)}
    if colour:
        o.update(image=plane(n, 3, H, W), bgr=plane(n, H, W, 3))
    return o


def _render(rm, classes, H, W, poses=None, into=None, colour=True, aligned=True, **kw):
    n = len(classes)
    o = _planes(n, H, W, colour, aligned) if into is None else into
    if poses is None:
        poses = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))
    if colour:
        kw["plane_means"] = PM
    rm.render_batch(torch.tensor(classes, dtype=torch.int32, device=DEV), torch.from_numpy(poses).to(DEV), mask_thr=rr.MASK_THR,
                    **dict({k: v for k, v in o.items()}, **kw))
    return o


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check_sample(o, b, name, H, W, bil=False, colour=True):
    """sample b of host outputs `o` against render_rules of scene `name`: every pixel of every plane"""
    want = rr.expected(name, H, W, bil)
    covered = want.owner >= 0
    depth = o["depth"][b, 0]
    tag = (name, H, W)
    np.testing.assert_array_equal(depth > 0, covered, err_msg=str(tag))
    np.testing.assert_allclose(depth[covered], want.depth[covered], rtol=2e-6, err_msg=str(tag))
    np.testing.assert_array_equal(depth[~covered], 0.0, err_msg=str(tag))
    np.testing.assert_array_equal(o["mask"][b, 0], want.mask, err_msg=str(tag))
    assert o["bbox"][b].tolist() == want.bbox, tag
    assert o["status"][b] == 0, tag
    if colour:
        if rr.scene(name)["per_face"]:
            np.testing.assert_array_equal(rr.owner_from_bgr(o["bgr"][b]), want.owner, err_msg=str(tag))
        np.testing.assert_array_equal(o["bgr"][b], want.bgr, err_msg=str(tag))
        np.testing.assert_array_equal(o["image"][b], syn.bgr_to_blob(o["bgr"][b])[0], err_msg=str(tag))
        rgb = want.bgr[:, :, ::-1].transpose(2, 0, 1)
        np.testing.assert_array_equal(o["image"][b], rgb - PM.astype(np.float32)[:, None, None], err_msg=str(tag))


class World(object):
    """one machine over all exact scenes per frame size, and its batch render, rendered once and kept unchanged"""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.rm = _machine(SCENES, H, W)
        self.dev = _render(self.rm, list(range(B)), H, W)
        self.batch = _host(self.dev)


_worlds = {}


@pytest.fixture(params=rr.FRAMES, ids=["{}x{}".format(*f) for f in rr.FRAMES])
def world(request, hip_lib):
    if request.param not in _worlds:
        _worlds[request.param] = World(*request.param)
    return _worlds[request.param]


def test_batch_equals_rules(world):
    """30x37: the one-pass resolve (W % 4 != 0); 32x48: the two-pass resolve"""
    for b, name in enumerate(NAMES):
        _check_sample(world.batch, b, name, world.H, world.W)
    assert world.batch["bbox"][NAMES.index("nothing")].tolist() == [world.W, -1, world.H, -1]


def test_two_pass_with_clean_bbox_hint(hip_lib):
    """the scenes rendered in another order into planes that hold the first render, with that render's bbox as the hint: a pixel the
    first render drew and the second does not must be cleared, one outside both boxes must still be background"""
    H, W = rr.FRAMES[1]
    rm = _machine(SCENES, H, W)
    first = _render(rm, list(range(B)), H, W)
    same = _host(_render(rm, list(range(B)), H, W, into=first, clean_bbox=first["bbox"].clone()))
    for b, name in enumerate(NAMES):   # the same batch again, hinted with its own bbox
        _check_sample(same, b, name, H, W)
    order = [(b + 2) % B for b in range(B)]
    hint = first["bbox"].clone()
    second = _host(_render(rm, order, H, W, into=first, clean_bbox=hint))
    for b, c in enumerate(order):
        _check_sample(second, b, NAMES[c], H, W)
    again = _host(_render(rm, list(range(B)), H, W, into=first, clean_bbox=torch.from_numpy(second["bbox"]).to(DEV)))
    for b, name in enumerate(NAMES):   # and back, with the hint of the permuted render
        _check_sample(again, b, name, H, W)


def test_two_pass_without_colour(world):
    """only depth, mask and bbox asked for: at 32x48 the SHADE = false pass of the two-pass resolve"""
    o = _host(_render(world.rm, list(range(B)), world.H, world.W, colour=False))
    for b, name in enumerate(NAMES):
        _check_sample(o, b, name, world.H, world.W, colour=False)
    for k in PLAIN:
        np.testing.assert_array_equal(o[k], world.batch[k])


def test_one_pass_at_the_two_pass_size(hip_lib):
    """32x48 through the one-pass resolve (planes off 16-byte alignment): the same pixels"""
    H, W = rr.FRAMES[1]
    o = _host(_render(_machine(SCENES, H, W), list(range(B)), H, W, aligned=False))
    for b, name in enumerate(NAMES):
        _check_sample(o, b, name, H, W)


def test_each_sample_alone(world):
    """B = 1 gives the bits of the sample's row in the batch"""
    for b in range(B):
        solo = _render(world.rm, [b], world.H, world.W)
        for k in COLOUR + PLAIN:
            assert torch.equal(solo[k][0], world.dev[k][b]), (NAMES[b], k)


def test_texels_bilinear(world):
    """the texel scene under the bilinear filter: at texel centres the texel itself, between them the floored blend, clamped at the edge"""
    tex = [rr.scene("texels")]
    for bil in (True, False):
        o = _host(_render(_machine(tex, world.H, world.W, bil=bil), [0], world.H, world.W))
        _check_sample(o, 0, "texels", world.H, world.W, bil=bil)
    assert not np.array_equal(rr.expected("texels", world.H, world.W, True).bgr, rr.expected("texels", world.H, world.W, False).bgr)


def test_per_sample_cameras_equal_to_the_uniform_one(world):
    """K as (B,9) device rows all equal to the machine's K: the uniform render, bit for bit (fill_rule is sample 0 of the batch)"""
    K = torch.from_numpy(np.tile(rr.RK.reshape(1, 9), (B, 1))).to(DEV)
    o = _render(world.rm, list(range(B)), world.H, world.W, K=K)
    assert NAMES[0] == "fill_rule"
    for k in COLOUR + PLAIN:
        assert torch.equal(o[k], world.dev[k]), k
    _check_sample(_host(o), 0, "fill_rule", world.H, world.W)


@pytest.mark.parametrize("aligned", [True, False], ids=["two-pass", "one-pass"])
def test_near_cut(hip_lib, aligned):
    """a flat patch across the near plane, both poses in one batch: no hole among the pixels whose whole 3x3 neighbourhood of rays meets
    the patch, nothing drawn where no neighbouring ray does, and the oracle's depth where both draw"""
    nc = rr.near_cut()
    H, W = rr.NEAR_H, rr.NEAR_W
    rm = _machine([dict(nc, name="patch")], H, W, K=rr.NEAR_K, znear=rr.NEAR_ZNEAR, zfar=rr.NEAR_ZFAR)
    o = _host(_render(rm, [0, 0], H, W, poses=nc["poses"], aligned=aligned))
    assert o["status"].tolist() == [0, 0]
    for b in range(2):
        gd = o["depth"][b, 0]
        holes, stray = rr.near_cut_faults(gd, b)
        print("pose {}: {} interior pixels, {} drawn, {} holes, {} stray".format(b, nc["interior"][b].sum(), (gd > 0).sum(), holes, stray))
        assert holes == 0 and stray == 0
        assert gd[gd > 0].min() >= rr.NEAR_ZNEAR
        P = nc["poses"][b]
        rb, rd = native.render(nc["verts"], nc["uvs"], nc["faces"], nc["tex"], P[:, :3], P[:, 3], rr.NEAR_K, H=H, W=W, znear=rr.NEAR_ZNEAR,
                               zfar=rr.NEAR_ZFAR)
        band = ~nc["interior"][b] & nc["allowed"][b]
        assert ((gd > 0) != (rd > 0))[band].sum() <= 4       # the band along the cut and the rim: the suite's bar against the oracle
        assert not ((gd > 0) != (rd > 0))[~band].any()
        both = (gd > 0) & (rd > 0)
        assert both.sum() >= 400
        np.testing.assert_allclose(gd[both], rd[both], rtol=2e-6)
        np.testing.assert_array_equal(o["mask"][b, 0], (gd > rr.MASK_THR).astype(np.float32))
