"""GPU: dim_vis_overlay (csrc/vis.hip) against tests/vis_reference.py, byte for byte (everything behind the base colour is integer
arithmetic: np.array_equal, no tolerance anywhere), its argument errors, and TEST.VISUALIZE end to end through pred_eval: the files
written, every picture against the reference on planes the test renders itself, and the tables untouched by the feature.

The kernel's tile is 64 x 32 pixels (VIS_TW x VIS_TH): the shapes sit below, on and above it, and the layers put an edge on a tile's
last row and column, let the radius-3 marks cross into the next tile and its corner, and touch every frame border and corner."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard_arena  # noqa: E402
import vis_reference as vr  # noqa: E402
from scene import make_scene, make_test_config  # noqa: E402

DEV = "cuda:0"
TW, TH = 64, 32
MEANS = np.array([103.939, 116.779, 123.68], dtype=np.float32)   # B, G, R
SHAPES = [(1, 1, 1), (1, 1, 9), (2, 7, 1), (2, 17, 70), (3, 33, 130), (1, 65, 257),
          (1, TH - 1, TW - 1), (1, TH, TW), (1, TH + 1, TW + 1), (2, TH + 1, TW - 1), (1, TH - 1, TW + 4)]
COLOURS = [(191, 191, 191), (0, 0, 255), (0, 255, 0), (255, 0, 0), (13, 200, 77), (255, 255, 255), (0, 0, 0), (90, 17, 240)]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def _disc(H, W, cy, cx, r):
    y, x = np.mgrid[:H, :W]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def _rect(H, W, y0, y1, x0, x1):
    """rows y0..y1, columns x0..x1, both ends included, clipped to the frame"""
    m = np.zeros((H, W), dtype=bool)
    m[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
    return m


def make_layers(B, H, W, L, seed, empty=None):
    """(L,B,H,W) float32 depth-like planes (inside: 0.3..2, outside: 0, negatives and NaNs) and what they are built for"""
    rng = np.random.default_rng(seed)
    masks = np.zeros((L, B, H, W), dtype=bool)
    for b in range(B):
        shapes = [
            # its last row and column are a tile's last row and column: the edge lies there, and the marks of radius >= 1 cross into the
            # tile to the right, the tile below and the tile at the corner
            _rect(H, W, TH - 9 + b, TH - 1, TW - 21, TW - 1),
            # a disc about the frame's first corner: touches the top and the left border and that corner
            _disc(H, W, 0, 0, 2 + min(H, W) // 3 + b),
            # the other three corners and, between them, the bottom and the right border
            _rect(H, W, H - 3, H - 1, 0, 2) | _rect(H, W, 0, 1, W - 4, W - 1) | _rect(H, W, H - 2 - b, H - 1, W - 3, W - 1)
            | _rect(H, W, H - 1, H - 1, W // 3, 2 * W // 3) | _rect(H, W, H // 3, 2 * H // 3, W - 2, W - 1),
            # across the second tile boundary in x and the first in y
            _disc(H, W, TH + 2, 2 * TW - 1, 7),
        ]
        for l in range(L):
            m = shapes[l] if l < len(shapes) else np.zeros((H, W), dtype=bool)
            if l >= len(shapes):
                for _ in range(2):
                    m = m | _disc(H, W, rng.integers(0, H), rng.integers(0, W), rng.integers(1, 3 + max(H, W) // 5))
            masks[l, b] = m
    if empty is not None and empty < L:
        masks[empty] = False
    values = rng.uniform(0.3, 2.0, size=masks.shape).astype(np.float32)
    outside = rng.choice(np.array([0.0, 0.0, 0.0, -0.5, np.nan, -0.0], dtype=np.float32), size=masks.shape)
    return np.where(masks, values, outside).astype(np.float32)


def make_image(B, H, W, seed):
    """an image_observed blob: grey levels from below 0 to above 255 (both clamps), halves, a few NaNs, minus the means"""
    rng = np.random.default_rng(seed)
    grey = np.round(rng.uniform(-20.0, 280.0, size=(B, 3, H, W)) * 2.0) / 2.0
    grey[rng.uniform(size=grey.shape) < 0.01] = np.nan
    img = grey.astype(np.float32)
    for c in range(3):
        img[:, c] -= MEANS[2 - c]
    return img


def styles(L, edge_alpha, fill_alpha):
    return np.asarray([COLOURS[l] + (edge_alpha if l % 3 else 256, fill_alpha if l % 2 == 0 else 0) for l in range(L)], dtype=np.int32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().copy()


def run_overlay(image, layers, style, radius, out_phase=0, counts=True):
    """one call into guarded outputs, the inputs checked to be unchanged -> out (B,H,W,3), counts (B,L,2) or None (numpy)"""
    from lib.hip import ops

    B, _, H, W = image.shape
    L = layers.shape[0]
    d_img, d_lay = _dev(image), _dev(layers)
    img0, lay0 = _bits(d_img), _bits(d_lay)
    out = guard_arena.GuardArena(B * H * W * 3, dtype=torch.uint8, device=DEV, fill=guard_arena.SENTINEL_WORD, phase=out_phase)
    cnt = guard_arena.GuardArena(B * L * 2, dtype=torch.int32, device=DEV, fill=guard_arena.SENTINEL_WORD) if counts else None
    ops.vis_overlay(d_img, d_lay, style, radius, MEANS, out=out.view((B, H, W, 3)), counts=cnt.view((B, L, 2)) if counts else None)
    out.check("vis_overlay out {}".format((B, H, W, L, radius)))
    if counts:
        cnt.check("vis_overlay counts")
    assert np.array_equal(_bits(d_img), img0) and np.array_equal(_bits(d_lay), lay0), "an input was written"
    return out.view((B, H, W, 3)).cpu().numpy().copy(), cnt.view((B, L, 2)).cpu().numpy().copy() if counts else None


def _compare(image, layers, style, radius, what, **kw):
    got, got_counts = run_overlay(image, layers, style, radius, **kw)
    want, want_counts = vr.overlay(image, MEANS, layers, style, radius)
    differ = int((got != want).any(-1).sum())
    print(what, "pixels that differ:", differ, "counts", got_counts.reshape(-1).tolist() if got_counts is not None else None)
    assert np.array_equal(got, want), "{}: {} pixels differ, first at {}".format(what, differ, np.argwhere((got != want).any(-1))[:1].tolist())
    if got_counts is not None:
        assert np.array_equal(got_counts, want_counts), "{}: counts {} != {}".format(what, got_counts.tolist(), want_counts.tolist())
    return want_counts


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_overlay_matches_reference(hip_lib, shape):
    B, H, W = shape
    image = make_image(B, H, W, seed=11)
    for L in (1, 3, 8):
        layers = make_layers(B, H, W, L, seed=100 + L)
        for radius in range(4):
            for fill in (0, 64):
                _compare(image, layers, styles(L, 200, fill), radius, "{} L {} radius {} fill {}".format(shape, L, radius, fill))


def test_overlay_marks_reach_the_neighbouring_tiles(hip_lib):
    """what the layers of make_layers are built for, stated on the reference: at (3,33,130) layer 0's edge lies on row 31 and column
    63, and at radius 3 its marks are in the tile to the right, the tile below and the tile at the corner"""
    B, H, W = 3, 33, 130
    layers = make_layers(B, H, W, 3, seed=103)
    ins = vr.inside(layers[0, 0])
    e = vr.edge(ins)
    assert e[TH - 1, TW - 21:TW].all() and e[TH - 9:TH, TW - 1].all()
    m = vr.marked(e, 3)
    assert m[TH - 1, TW + 2] and m[TH, TW - 5] and m[TH, TW + 2] and not m[TH - 1, TW + 3]
    # the other layers touch every border and corner of the frame
    both = vr.inside(layers[1, 0]) | vr.inside(layers[2, 0])
    assert both[0, 0] and both[0, W - 1] and both[H - 1, 0] and both[H - 1, W - 1]
    assert both[0].any() and both[H - 1].any() and both[:, 0].any() and both[:, W - 1].any()


def test_overlay_full_size(hip_lib):
    B, H, W = 1, 480, 640
    _compare(make_image(B, H, W, seed=12), make_layers(B, H, W, 3, seed=7), styles(3, 256, 64), 3, "full size")


def test_overlay_one_empty_layer_and_widths_off_four(hip_lib):
    for B, H, W in ((2, 37, 70), (1, 35, 67), (1, 33, 66)):
        image = make_image(B, H, W, seed=13)
        for empty in (0, 1, 2):
            counts = _compare(image, make_layers(B, H, W, 3, seed=5, empty=empty), styles(3, 256, 64), 2, "empty layer {}".format(empty))
            assert counts[:, empty].tolist() == [[0, 0]] * B and counts[:, (empty + 1) % 3, 0].min() > 0


def test_overlay_unaligned_output_and_no_counts(hip_lib):
    """W % 4 == 0 with the output at an odd address takes the one-pixel path; counts may be NULL"""
    B, H, W = 2, 33, 68
    image, layers = make_image(B, H, W, seed=14), make_layers(B, H, W, 3, seed=9)
    for phase in (0, 1, 2):
        _compare(image, layers, styles(3, 256, 64), 3, "out at phase {}".format(phase), out_phase=phase)
    _compare(image, layers, styles(3, 256, 64), 1, "no counts", counts=False)


def test_counts_do_not_depend_on_what_they_held(hip_lib):
    from lib.hip import ops

    B, H, W, L = 2, 40, 100, 3
    image, layers = make_image(B, H, W, seed=15), make_layers(B, H, W, L, seed=3)
    _, want = vr.overlay(image, MEANS, layers, styles(L, 256, 0), 1)
    counts = torch.full((B, L, 2), 12345, dtype=torch.int32, device=DEV)
    d_img, d_lay = _dev(image), _dev(layers)
    for _ in range(2):   # the second call starts from the first one's numbers
        ops.vis_overlay(d_img, d_lay, styles(L, 256, 0), 1, MEANS, counts=counts)
        assert np.array_equal(counts.cpu().numpy(), want)


def test_argument_errors_write_nothing(hip_lib):
    from lib.hip import capi

    B, H, W, L = 2, 9, 12, 2
    image, layers = _dev(make_image(B, H, W, seed=16)), _dev(make_layers(B, H, W, L, seed=1))
    out = guard_arena.GuardArena(B * H * W * 3, dtype=torch.uint8, device=DEV, fill=guard_arena.SENTINEL_WORD)
    cnt = guard_arena.GuardArena(B * L * 2, dtype=torch.int32, device=DEV, fill=guard_arena.SENTINEL_WORD)
    out0, cnt0, img0, lay0 = out.view().cpu().numpy().copy(), cnt.view().cpu().numpy().copy(), _bits(image), _bits(layers)
    means = np.ascontiguousarray(MEANS)
    good_style = np.ascontiguousarray(styles(L, 256, 64))
    stream = capi.current_stream()
    good = dict(image=image.data_ptr(), means=means.ctypes.data, layers=layers.data_ptr(), L=L, style=good_style.ctypes.data, radius=1, B=B,
                H=H, W=W, out=out.address(), counts=cnt.address())

    def call(**change):
        a = dict(good, **change)
        return hip_lib.dim_vis_overlay(a["image"], a["means"], a["layers"], a["L"], a["style"], a["radius"], a["B"], a["H"], a["W"], a["out"],
                                       a["counts"], stream)

    def bad_style(row, col, value):
        s = good_style.copy()
        s[row, col] = value
        return s

    bad_styles = [bad_style(0, 0, 256), bad_style(1, 1, -1), bad_style(0, 2, 1000), bad_style(1, 3, 257), bad_style(0, 3, -1),
                  bad_style(1, 4, 257), bad_style(0, 4, -2)]
    cases = [dict(L=0), dict(L=9), dict(L=-1), dict(radius=-1), dict(radius=4), dict(B=0), dict(B=65536), dict(H=0), dict(H=32768),
             dict(W=0), dict(W=32768), dict(H=-3), dict(image=None), dict(means=None), dict(layers=None), dict(style=None), dict(out=None),
             dict(out=image.data_ptr()), dict(out=layers.data_ptr() + 4 * (B * H * W * L - 1)), dict(image=out.address()),
             dict(layers=out.address() + B * H * W * 3 - 1)]
    cases += [dict(style=s.ctypes.data) for s in bad_styles]
    for change in cases:
        assert call(**change) == -1, change
        assert len(hip_lib.dim_last_error()) > 0 and b"vis_overlay" in hip_lib.dim_last_error(), change
    torch.cuda.synchronize()
    out.check("argument errors")
    cnt.check("argument errors")
    assert np.array_equal(out.view().cpu().numpy(), out0) and np.array_equal(cnt.view().cpu().numpy(), cnt0), "a refused call wrote"
    assert np.array_equal(_bits(image), img0) and np.array_equal(_bits(layers), lay0)
    assert call() == 0 and call(counts=None) == 0   # and the good call goes through
    torch.cuda.synchronize()


# ---- TEST.VISUALIZE end to end

@pytest.fixture(scope="module")
def e2e(hip_lib):
    from deepim.core.tester import Predictor
    from deepim.symbols.deepIM_flownet import deepIM_flownet
    from lib.dataset.evaluation import PoseEvaluator
    from lib.render_hip.render_py_multi import Render_Py

    cfg = make_test_config(test_iter=2)
    sym = deepIM_flownet()
    sym.get_symbol(cfg, is_train=False)
    params = sym.init_weights(cfg, {}, {}, seed=0)
    B = 2
    scene = make_scene(B=B)
    rm = Render_Py(None, cfg.dataset.class_name, scene["K"], meshes=scene["models"])
    pred = Predictor(cfg, params, B)
    pts = scene["models"][0][0].astype(np.float64)
    name = cfg.dataset.class_name[0]
    ev = PoseEvaluator(cfg.dataset.class_name, {name: pts}, {name: float(np.linalg.norm(pts.max(0) - pts.min(0)))})
    batch = dict(scene["blobs"], pose_observed=scene["pose_gt"].astype(np.float32))
    yield cfg, scene, rm, pred, ev, batch
    from deepim.config.config import reset_config

    reset_config()


def _run(e2e, vis_dir=None, graph=False, batch=None, **keys):
    """pred_eval on the scene's batch -> (out, refiner); vis_dir switches TEST.VISUALIZE on"""
    from deepim.core.tester import Refiner, pred_eval

    cfg, scene, rm, pred, ev, default_batch = e2e
    old = {k: cfg.TEST.get(k) for k in list(keys) + ["VISUALIZE", "VIS_DIR"]}
    cfg.TEST.update(keys)
    cfg.TEST.VISUALIZE, cfg.TEST.VIS_DIR = vis_dir is not None, vis_dir or ""
    try:
        ref = Refiner(cfg, pred, rm, 2, capture_graph=graph)
        out = pred_eval(cfg, ref, [batch if batch is not None else default_batch], ev)
        torch.cuda.synchronize()
        return out, ref
    finally:
        cfg.TEST.update(old)


def _same(a, b, path="out"):
    """bit-identical, through dicts, lists and arrays"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], "{}[{!r}]".format(path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "{}[{}]".format(path, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), path
    else:
        assert a == b, path


def _depth_at(rm, cls, pose):
    """the test's own render -> depth (B,1,H,W), bbox (B,4) on the device"""
    B = pose.shape[0]
    depth = torch.zeros((B, 1, int(rm.height), int(rm.width)), dtype=torch.float32, device=DEV)
    bbox = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    rm.render_batch(cls, pose.to(DEV, torch.float32).contiguous(), depth=depth, bbox=bbox, mask_thr=0.0)
    return depth, bbox


def _read_png(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1]


DEFAULT_STYLE = [[191, 191, 191, 256, 0], [0, 0, 255, 256, 0], [0, 255, 0, 256, 0]]


def _check_pictures(e2e, ref, root, frames):
    """every picture under root against the reference.  frames: [(name, [pose of layer 1, pose of layer 2 or None])]"""
    from lib.hip import ops

    cfg, scene, rm, pred, ev, batch = e2e
    B, H, W = 2, int(rm.height), int(rm.width)
    means = np.asarray(cfg.network.PIXEL_MEANS, dtype=np.float32)
    image = np.asarray(batch["image_observed"], dtype=np.float32)
    d_image = _dev(image)
    cls = ref.batch["class_index"]
    d_gt, box_gt = _depth_at(rm, cls, torch.from_numpy(batch["pose_observed"]))
    d_init, box_init = _depth_at(rm, cls, ref.pose_init)
    zf = ops.zoom_factor(box_gt, box_init, ref.pose_init, ref.net.K, H, W)
    z_image = ops.zoom_planes(d_image, zf, add3=ref.net.plane_means).cpu().numpy()
    zoomed = lambda d: ops.zoom_planes(d, zf, pre=1, post=1)  # noqa: E731
    names = sorted(os.listdir(root))
    assert names == ["pair_000000_ape", "pair_000001_ape"]
    want_files = sorted(["info.json"] + [n + s for n, _ in frames for s in (".png", "_zoom.png")])
    for name, (first, second) in frames:
        planes = [d_gt, _depth_at(rm, cls, first)[0]] + ([_depth_at(rm, cls, second)[0]] if second is not None else [])
        L = len(planes)
        full = torch.cat(planes, dim=1).permute(1, 0, 2, 3).contiguous().cpu().numpy()
        zoom = torch.cat([zoomed(p) for p in planes], dim=1).permute(1, 0, 2, 3).contiguous().cpu().numpy()
        want, want_counts = vr.overlay(image, means, full, DEFAULT_STYLE[:L], 1)
        want_z, want_z_counts = vr.overlay(z_image, means, zoom, DEFAULT_STYLE[:L], 1)
        # the scene's ground truth is in the frame; a pose of the seeded (untrained) head or of a stage behind it may leave it: count 0
        assert want_counts[:, 0, 0].min() > 0
        for b in range(B):
            d = os.path.join(root, names[b])
            assert sorted(os.listdir(d)) == want_files
            got, got_z = _read_png(os.path.join(d, name + ".png")), _read_png(os.path.join(d, name + "_zoom.png"))
            print(name, "pair", b, "pixels that differ:", int((got != want[b]).any(-1).sum()), "zoomed:", int((got_z != want_z[b]).any(-1).sum()))
            assert np.array_equal(got, want[b]), (name, b)
            assert np.array_equal(got_z, want_z[b]), (name, b, "zoom")
            info = json.load(open(os.path.join(d, "info.json")))
            who = ["gt", "start", "result"][:L]
            assert info["marked_pixels"][name] == {w: int(want_counts[b, l, 0]) for l, w in enumerate(who)}
            assert info["marked_pixels_zoom"][name] == {w: int(want_z_counts[b, l, 0]) for l, w in enumerate(who)}
            assert info["frames"] == [n for n, _ in frames] and len(info["rot_err"]) == len(frames) == len(info["trans_err"])
            assert np.array_equal(np.asarray(info["zoom_factor"], dtype=np.float32), zf[b].cpu().numpy())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_visualize_end_to_end(e2e, tmp_path, graph):
    off, ref_off = _run(e2e, graph=graph)
    poses_off = ref_off.poses_iter.cpu().numpy().copy()
    root = str(tmp_path / "vis")
    on, ref = _run(e2e, vis_dir=root, graph=graph)
    _same(on, off)
    assert ref.poses_iter.cpu().numpy().tobytes() == poses_off.tobytes()
    frames = [("iter_00", (ref.pose_init, None)), ("iter_01", (ref.pose_init, ref.poses_iter[0])), ("iter_02", (ref.pose_init, ref.poses_iter[1]))]
    _check_pictures(e2e, ref, root, frames)
    info = json.load(open(os.path.join(root, "pair_000000_ape", "info.json")))
    assert info["rot_err"][1:] == [float(v) for v in (on["all_rot_err"][0][0][0], on["all_rot_err"][0][1][0])]


def test_visualize_writes_the_icp_frame(e2e, tmp_path):
    cfg, scene, rm, pred, ev, batch = e2e
    cls = torch.from_numpy(np.asarray(batch["class_index"])).to(DEV, torch.int32)
    depth = _depth_at(rm, cls, torch.from_numpy(batch["pose_observed"]))[0].cpu().numpy()
    with_depth = dict(batch, depth_observed=depth)
    off, _ = _run(e2e, batch=with_depth, ICP_ITER=2)
    root = str(tmp_path / "vis")
    on, ref = _run(e2e, vis_dir=root, batch=with_depth, ICP_ITER=2)
    _same(on, off)
    last = ref.poses_iter[1]
    frames = [("iter_00", (ref.pose_init, None)), ("iter_01", (ref.pose_init, ref.poses_iter[0])), ("iter_02", (ref.pose_init, last)),
              ("icp", (last, ref.pose_icp))]
    _check_pictures(e2e, ref, root, frames)


def test_visualize_skips_undetected_pairs_and_stops_at_max_pairs(e2e, tmp_path):
    cfg, scene, rm, pred, ev, batch = e2e
    lost = dict(batch, src_pose=np.array(batch["src_pose"], copy=True))
    lost["src_pose"][0] = -1.0
    root = str(tmp_path / "lost")
    _run(e2e, vis_dir=root, batch=lost, VIS_ZOOM=False)
    assert os.listdir(root) == ["pair_000001_ape"]
    assert sorted(os.listdir(os.path.join(root, "pair_000001_ape"))) == ["info.json", "iter_00.png", "iter_01.png", "iter_02.png"]
    root = str(tmp_path / "first")
    _run(e2e, vis_dir=root, VIS_MAX_PAIRS=1, VIS_VIDEO=True, VIS_VIDEO_ZOOM=True)
    assert os.listdir(root) == ["pair_000000_ape"]
    files = set(os.listdir(os.path.join(root, "pair_000000_ape")))
    assert {"iters.gif", "iters_zoom.gif"} <= files and len(files) == 1 + 2 * 3 + 2
    from PIL import Image
    from deepim.core.visualize import GIF_MS

    def shown_ms(path):   # the writer stores a picture that repeats as one frame shown for the sum of the durations
        g, total = Image.open(path), 0
        for i in range(g.n_frames):
            g.seek(i)
            total += g.info["duration"]
        assert g.size == (640, 480)
        return total

    assert shown_ms(os.path.join(root, "pair_000000_ape", "iters.gif")) == (5 + 1 + 5) * GIF_MS
    assert shown_ms(os.path.join(root, "pair_000000_ape", "iters_zoom.gif")) == (3 + 5 + 1 + 5) * GIF_MS
