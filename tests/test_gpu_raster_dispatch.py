"""Every dispatch arm of the rasteriser at the smallest shape that can go wrong: (two-pass | one-pass resolve) x (no colour output |
unlit | ModelNet lit | LINEMOD lit) x (one camera | one camera per sample), through render_batch only, at 48x64 with B = 3 and both
texel filters.  One sample straddles the near plane, so the clipped-face branch of the shader -- the only place the resolve reads K --
runs in every shaded cell.  All comparisons between cells are bit-exact; the unlit and the ModelNet-lit two-pass uniform cells are
pinned to the oracle's software rasteriser under the bars of tests/test_gpu_ops.py (test_rasteriser_vs_oracle and the lit part of
test_rasteriser_near_plane_clipping_vs_oracle), and every other cell is chained to one of those two."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lib.utils import synthetic as syn  # noqa: E402
from oracle import native  # noqa: E402

DEV = "cuda:0"
B, LH, LW = 3, 48, 64
LK = np.array([[110.0, 0, 31.5], [0, 110.0, 23.5], [0, 0, 1]], np.float32)   # the scene of tests/test_gpu_occ_scene.py
RATIO = 0.4
WHITE, TINTED = (1.0, 1.0, 1.0), (0.3, 0.9, 1.2)
KEYS = ("image", "depth", "mask", "bgr", "bbox", "status")
SHADINGS = ("none", "unlit", "modelnet", "linemod")


def _cam(s, dx, dy):
    K = LK.copy()
    K[0, 0] *= s
    K[1, 1] *= s
    K[0, 2] += dx
    K[1, 2] += dy
    return K


KS = np.stack([_cam(1.2, 3.0, -2.0), LK, _cam(0.8, -2.5, 3.5)])   # three different cameras; sample 1 keeps LK


def _poses():
    """two samples wholly behind the near plane and one at t_z = 0.27 whose vertices span z = 0.20 .. 0.33 around it (0.25 m).  The
    oracle covers 574 / 354 / 1897 pixels under LK and 826 / 354 / 1287 under KS (checked on the host before the poses were fixed;
    test_every_cell_is_clean_and_covered holds the device to > 100)."""
    rng = np.random.default_rng(4)
    T = [[0.01, -0.02, 0.5], [-0.03, 0.015, 0.6], [0.0, 0.0, 0.27]]
    return np.stack([np.concatenate([syn.random_rotation(rng), np.array(t)[:, None]], axis=1) for t in T]).astype(np.float32)


def _outputs(n, aligned, colour):
    """image / depth / mask / bgr planes; aligned=False shifts every plane by one float, which forces the one-thread-per-pixel resolve
    (as _outputs of tests/test_gpu_per_pair_intrinsics.py does)"""
    def plane(*shape):
        if aligned:
            return torch.zeros(shape, dtype=torch.float32, device=DEV)
        return torch.zeros((int(np.prod(shape)) + 1,), dtype=torch.float32, device=DEV)[1:].view(*shape)

    o = {"depth": plane(n, 1, LH, LW), "mask": plane(n, 1, LH, LW), "bbox": torch.zeros((n, 4), dtype=torch.int32, device=DEV),
         "status": torch.zeros((n,), dtype=torch.int32, device=DEV)}
    if colour:
        o.update(image=plane(n, 3, LH, LW), bgr=plane(n, LH, LW, 3))
    return o


class World(object):
    """the three render machines over one mesh for one texel filter, and every cell of the matrix rendered once and kept unchanged"""

    def __init__(self, bil):
        from lib.render_hip.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi, vertex_normals
        from lib.render_hip.render_py_light_multi_program import Render_Py_Light_MultiProgram
        from lib.render_hip.render_py_multi import Render_Py

        rng = np.random.default_rng(21)
        v, t, f = syn.make_mesh(rng, subdiv=2, diameter=0.15)
        tex = syn.make_texture(rng)
        nrm = vertex_normals(v, f).astype(np.float32)
        self.bil, self.mesh = bil, (v, nrm, t, f, tex)
        self.new_unlit = lambda: Render_Py(None, ["obj"], LK, LW, LH, 0.25, 6.0, meshes=[(v, t, f, tex)], tex_bilinear=bil)
        self.rm = {"none": self.new_unlit(), "modelnet": Render_Py_Light_ModelNet_Multi(None, tex, LK, LW, LH, 0.25, 6.0, brightness_ratios=[RATIO],
                                                                                       meshes=[(v, nrm, t, f)], tex_bilinear=bil),
                   "linemod": Render_Py_Light_MultiProgram(["__background__", "obj"], None, LK, LW, LH, 0.25, 6.0, [RATIO],
                                                           meshes=[(v, nrm, t, f, tex)], tex_bilinear=bil)}
        self.rm["unlit"] = self.rm["none"]
        self.poses = _poses()
        self.lp = np.stack([native.modelnet_light_position(p.astype(np.float64), idx=1) for p in self.poses]).astype(np.float32)
        self.pm = syn.plane_means()
        self.cells = {}

    def render(self, shading, aligned, K, inten=WHITE, rows=slice(0, B), poses=None, rm=None):
        """one render_batch of samples `rows` -> its outputs.  K: None, one 3x3, or a (n,9) device tensor"""
        poses = (self.poses if poses is None else poses)[rows]
        n = poses.shape[0]
        o = _outputs(n, aligned, shading != "none")
        kw = dict(o, K=K, mask_thr=0.2)
        if shading != "none":
            kw["plane_means"] = self.pm
        if shading in ("modelnet", "linemod"):
            kw["light_position"] = torch.from_numpy(self.lp[rows]).to(DEV)
            kw["light_intensity"] = torch.tensor([inten] * n, dtype=torch.float32, device=DEV)
        (self.rm[shading] if rm is None else rm).render_batch(torch.zeros(n, dtype=torch.int32, device=DEV), torch.from_numpy(poses).to(DEV), **kw)
        return o

    def cell(self, shading, resolve, camera, inten=WHITE):
        """camera: "uniform" (the machine's LK), "same" ((B,9) device rows all LK) or "own" ((B,9) device rows KS)"""
        key = (shading, resolve, camera, inten)
        if key not in self.cells:
            K = {"uniform": None, "same": np.tile(LK.reshape(1, 9), (B, 1)), "own": KS.reshape(B, 9)}[camera]
            self.cells[key] = self.render(shading, resolve == "two-pass", None if K is None else torch.from_numpy(K).to(DEV), inten)
        return self.cells[key]


_worlds = {}


@pytest.fixture(params=[False, True], ids=["nearest", "bilinear"])
def world(request, hip_lib):
    if request.param not in _worlds:
        _worlds[request.param] = World(request.param)
    return _worlds[request.param]


def _assert_equal(a, b, tag, keys=None):
    for k in (keys or [k for k in KEYS if k in a and k in b]):
        assert torch.equal(a[k], b[k]), (tag, k)


def test_unlit_two_pass_uniform_vs_oracle(world):
    """the bars of tests/test_gpu_ops.py::test_rasteriser_vs_oracle (its minimum of 500 pixels seen by both is 100 at this size)"""
    v, nrm, t, f, tex = world.mesh
    o = world.cell("unlit", "two-pass", "uniform")
    for b in range(B):
        rb, rd = native.render(v, t, f, tex, world.poses[b][:, :3], world.poses[b][:, 3], LK, H=LH, W=LW, tex_bilinear=world.bil)
        gd = o["depth"][b, 0].cpu().numpy()
        cov_diff = ((gd > 0) != (rd > 0)).sum()
        assert cov_diff <= 4, cov_diff
        both = (gd > 0) & (rd > 0)
        assert both.sum() > 100
        np.testing.assert_allclose(gd[both], rd[both], rtol=2e-6)
        gb = o["bgr"][b].cpu().numpy()
        bad = (np.abs(gb - rb).max(axis=-1) > (1.0 if world.bil else 0.0)) & both
        print("sample {}: coverage differs at {} pixels, colour at {} of {}".format(b, cov_diff, bad.sum(), both.sum()))
        assert bad.sum() <= (20 if world.bil else 8), bad.sum()  # texel flips on cell borders
        np.testing.assert_array_equal(o["mask"][b, 0].cpu().numpy(), (gd > 0.2).astype(np.float32))
        ys, xs = np.nonzero(gd > 0.2)
        assert o["bbox"][b].tolist() == [xs.min(), xs.max(), ys.min(), ys.max()]
        np.testing.assert_allclose(o["image"][b].cpu().numpy(), syn.bgr_to_blob(gb)[0], atol=1e-4)
    zc = v @ world.poses[2][2, :3] + world.poses[2][2, 3]   # the last sample: cut by the near plane, nothing drawn in front of it
    assert zc.min() < 0.25 < zc.max() and gd[gd > 0].min() >= 0.25 and rd[rd > 0].min() >= 0.25


def test_modelnet_two_pass_uniform_vs_oracle(world):
    """the lit bars of tests/test_gpu_ops.py::test_rasteriser_near_plane_clipping_vs_oracle; the geometry is the unlit cell's"""
    v, nrm, t, f, tex = world.mesh
    o = world.cell("modelnet", "two-pass", "uniform", TINTED)
    for b in range(B):
        rb, rd = native.render_lit(v, nrm, t, f, tex, world.poses[b][:, :3], world.poses[b][:, 3], LK, world.lp[b], TINTED, RATIO, H=LH, W=LW,
                                   tex_bilinear=world.bil)
        gd, gb = o["depth"][b, 0].cpu().numpy(), o["bgr"][b].cpu().numpy()
        assert ((gd > 0) != (rd > 0)).sum() <= 4
        both = (gd > 0) & (rd > 0)
        assert both.sum() > 100
        bad = (np.abs(gb - rb).max(axis=-1)[both] > 1.0).sum()
        print("sample {}: more than one grey level off at {} of {} pixels".format(b, bad, both.sum()))
        assert bad <= 8
    _assert_equal(o, world.cell("unlit", "two-pass", "uniform"), "lit geometry", keys=("depth", "mask", "bbox", "status"))


@pytest.mark.parametrize("camera", ["uniform", "same", "own"])
@pytest.mark.parametrize("shading,inten", [("none", WHITE), ("unlit", WHITE), ("modelnet", WHITE), ("modelnet", TINTED), ("linemod", WHITE),
                                           ("linemod", TINTED)])
def test_one_pass_equals_two_pass(world, shading, inten, camera):
    """the two resolves share the shader, the background value and the empty-box convention"""
    _assert_equal(world.cell(shading, "one-pass", camera, inten), world.cell(shading, "two-pass", camera, inten), (shading, camera))


@pytest.mark.parametrize("resolve", ["two-pass", "one-pass"])
@pytest.mark.parametrize("shading,inten", [("none", WHITE), ("unlit", WHITE), ("modelnet", TINTED), ("linemod", TINTED)])
def test_per_sample_camera(world, shading, inten, resolve):
    """rows all equal to the machine's K: the uniform render; three different cameras: each sample as it renders alone under its own"""
    _assert_equal(world.cell(shading, resolve, "same", inten), world.cell(shading, resolve, "uniform", inten), (shading, resolve))
    own = world.cell(shading, resolve, "own", inten)
    for b in range(B):
        solo = world.render(shading, resolve == "two-pass", KS[b], inten, rows=slice(b, b + 1))
        for k in solo:
            assert torch.equal(own[k][b], solo[k][0]), (shading, resolve, b, k)
    for b in (0, 2):   # the cameras do matter
        assert not torch.equal(own["mask"][b], world.cell(shading, resolve, "uniform", inten)["mask"][b])


@pytest.mark.parametrize("camera", ["uniform", "own"])
@pytest.mark.parametrize("resolve", ["two-pass", "one-pass"])
def test_linemod_rule_reaches_the_kernel(world, resolve, camera):
    """white light: both light rules give the same bits; a tinted light at ratio 0.4 does not"""
    _assert_equal(world.cell("linemod", resolve, camera, WHITE), world.cell("modelnet", resolve, camera, WHITE), (resolve, camera))
    lm, mn = world.cell("linemod", resolve, camera, TINTED), world.cell("modelnet", resolve, camera, TINTED)
    _assert_equal(lm, mn, (resolve, camera), keys=("depth", "mask", "bbox", "status"))
    covered = (lm["depth"] > 0).permute(0, 2, 3, 1).expand(-1, -1, -1, 3)
    assert bool((lm["bgr"][covered] != mn["bgr"][covered]).any())
    assert not torch.equal(lm["bgr"], world.cell("linemod", resolve, camera, WHITE)["bgr"])


@pytest.mark.parametrize("camera", ["uniform", "own"])
@pytest.mark.parametrize("resolve", ["two-pass", "one-pass"])
def test_render_without_colour(world, resolve, camera):
    """depth, mask and bbox are the unlit render's, and the z-buffer is left clear: an unlit render of other poses into the same
    workspace equals that render by a machine whose workspace is new"""
    aligned = resolve == "two-pass"
    _assert_equal(world.cell("none", resolve, camera), world.cell("unlit", resolve, camera), (resolve, camera), keys=("depth", "mask", "bbox", "status"))
    K = None if camera == "uniform" else torch.from_numpy(KS.reshape(B, 9)).to(DEV)
    moved = world.poses.copy()
    moved[:, 0, 3] += 0.012
    moved[:, 1, 3] -= 0.007
    world.render("none", aligned, K)                                   # leaves the machine's workspace for B = 3 behind
    after = world.render("unlit", aligned, K, poses=moved)
    fresh = world.render("unlit", aligned, K, poses=moved, rm=world.new_unlit())
    _assert_equal(after, fresh, (resolve, camera))
    assert not torch.equal(after["depth"], world.cell("unlit", resolve, camera)["depth"])


@pytest.mark.parametrize("camera", ["uniform", "same", "own"])
@pytest.mark.parametrize("resolve", ["two-pass", "one-pass"])
def test_every_cell_is_clean_and_covered(world, resolve, camera):
    """no comparison above is background against background"""
    for shading, inten in (("none", WHITE), ("unlit", WHITE), ("modelnet", WHITE), ("modelnet", TINTED), ("linemod", WHITE), ("linemod", TINTED)):
        o = world.cell(shading, resolve, camera, inten)
        assert o["status"].tolist() == [0] * B, (shading, o["status"].tolist())
        covered = (o["depth"] > 0).sum(dim=(1, 2, 3)).tolist()
        assert min(covered) > 100, (shading, covered)
        if shading != "none":
            assert float(o["bgr"][0][o["depth"][0, 0] > 0].std()) > 3.0
