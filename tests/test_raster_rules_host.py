"""Host side of the exact rasteriser rules: oracle/raster.c against the numpy restatement of the conventions in csrc/raster.hip's header
(tests/raster_rules_reference.py) on every hand-built scene and both frame sizes of tests/test_gpu_raster_rules.py -- equality, not
"a few pixels" -- the analytic near-plane properties for the oracle, and negative controls that show each scene notices the wrong rule
it was built for.  Every builder asserts its own conditions (edge-centre counts, the depth band, interior >= 400) when it runs."""
import numpy as np
import pytest

import raster_rules_reference as rr
from oracle import native

EYE, ZERO = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
CASES = [(s["name"], H, W, bil) for s in rr.exact_scenes() for H, W in rr.FRAMES for bil in ((False, True) if s["name"] == "texels" else (False,))]


def _bbox(depth, H, W):
    ys, xs = np.nonzero(depth > rr.MASK_THR)
    return [int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())] if len(xs) else [W, -1, H, -1]


@pytest.mark.parametrize("name,H,W,bil", CASES, ids=["{}-{}x{}-{}".format(n, h, w, "bilinear" if b else "nearest") for n, h, w, b in CASES])
def test_oracle_equals_rules(name, H, W, bil):
    s, want = rr.scene(name), rr.expected(name, H, W, bil)
    bgr, depth = native.render(s["verts"], s["uvs"], s["faces"], s["tex"], EYE, ZERO, rr.RK, H=H, W=W, znear=rr.ZNEAR, zfar=rr.ZFAR,
                               tex_bilinear=bil)
    covered = want.owner >= 0
    print("{}: {} covered pixels, {} coverage differences, {} colour differences".format(
        name, covered.sum(), ((depth > 0) != covered).sum(), (bgr != want.bgr).any(axis=-1).sum()))
    np.testing.assert_array_equal(depth > 0, covered)
    np.testing.assert_array_equal(bgr, want.bgr)
    if s["per_face"]:
        np.testing.assert_array_equal(rr.owner_from_bgr(bgr), want.owner)
    np.testing.assert_array_equal((depth > rr.MASK_THR).astype(np.float32), want.mask)
    assert _bbox(depth, H, W) == want.bbox
    np.testing.assert_allclose(depth[covered], want.depth[covered], rtol=2e-6)
    np.testing.assert_array_equal(depth[~covered], 0.0)


def test_scenes_differ_in_size():
    """the GPU test renders them as the classes of one mesh table: vmax, fmax and the table's offsets only matter if the sizes differ"""
    sizes = [(len(s["verts"]), len(s["faces"])) for s in rr.exact_scenes()]
    assert len(set(sizes)) >= 5 and len(sizes) <= 8, sizes
    assert max(f for _, f in sizes) <= 400


def test_face_colours_round_trip():
    v, uv, f, tex = rr.per_face_texels(np.zeros((4, 3), np.float32), np.array([[0, 1, 2]] * 450))
    assert np.array_equal(rr.owner_from_bgr(tex[0, :, ::-1].astype(np.float32)), np.arange(450))
    assert rr.owner_from_bgr(np.zeros(3, np.float32)) == -1 and tex.min() > 0


@pytest.mark.parametrize("name,wrong", [("fill_rule", dict(fill="bottom-right")), ("z_ties", dict(tie="higher")), ("fill_rule", dict(snap="floor")),
                                        ("texels", dict(flip_rows=False))], ids=["bottom-right", "ties-to-higher", "snap-floor", "rows-unflipped"])
def test_negative_control(name, wrong):
    """the scene built for a rule changes at at least 5 pixels when the reference applies the wrong variant of that rule"""
    for H, W in rr.FRAMES:
        good, bad = rr.expected(name, H, W), rr.expected(name, H, W, **wrong)
        changed = int(((good.bgr != bad.bgr).any(axis=-1) | (good.owner != bad.owner)).sum())
        print("{} {}: {} pixels change at {}x{}".format(name, wrong, changed, H, W))
        assert changed >= 5, (name, wrong, changed)


def test_exactness_guard_refuses_an_inexact_scene():
    v = rr.scene("fill_rule")["verts"].copy()
    v[0, 0] += 1e-4
    with pytest.raises(AssertionError):
        rr.projection_is_exact(v, rr.RK)
    v = rr.scene("fill_rule")["verts"].copy()
    v[:, 2] = 0.75          # x / 0.75 is not exact in f32
    with pytest.raises(AssertionError):
        rr.projection_is_exact(v, rr.RK)


def test_near_cut_oracle():
    """both poses cut the patch at the near plane: no interior pixel is missed and nothing is drawn where no neighbouring ray meets it"""
    nc = rr.near_cut()
    for b in range(2):
        P = nc["poses"][b]
        bgr, depth = native.render(nc["verts"], nc["uvs"], nc["faces"], nc["tex"], P[:, :3], P[:, 3], rr.NEAR_K, H=rr.NEAR_H, W=rr.NEAR_W,
                                   znear=rr.NEAR_ZNEAR, zfar=rr.NEAR_ZFAR)
        holes, stray = rr.near_cut_faults(depth, b)
        print("pose {}: {} interior pixels, {} drawn, {} holes, {} stray".format(b, nc["interior"][b].sum(), (depth > 0).sum(), holes, stray))
        assert nc["interior"][b].sum() >= 400
        assert holes == 0 and stray == 0
        assert depth[depth > 0].min() >= rr.NEAR_ZNEAR
