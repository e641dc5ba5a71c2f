"""Contour overlays of the initial, the refined and the true pose for `test.py --vis` (TEST.VISUALIZE).

The reference draws them with toolkit/gen_video_iter_zoom_with_factor.py on the host: per pair and iteration the observed frame with
the outline of the initial pose in red, of the ground truth in grey 0.75 and of the refined pose in green, the same zoomed to the object,
and a short zoom-in in front of a video.  Here everything a picture needs is on the device after Refiner.refine(): PoseVisualizer
renders depth at the poses into planes of its own, dim_vis_overlay (csrc/vis.hip) turns the planes into outlines blended over the
observed blob, and the finished 8-bit frames of a batch reach the host in ONE copy.  It runs eagerly, outside the captured graph, and
only reads the Refiner's buffers.  Text labels and legends are left out: the numbers are in each pair's info.json.

    <VIS_DIR>/pair_<index:06d>_<class>/iter_<k:02d>.png        k = 0 (ground truth + initial pose) .. test_iter (+ refined pose k)
                                      /iter_<k:02d>_zoom.png   the same in the pair's zoom window (TEST.VIS_ZOOM)
                                      /<stage>.png [_zoom]     icp / photo / sil when on: ground truth, the loop's last pose, the stage's
                                      /info.json               errors per frame, the zoom factor, the marked-pixel counts
                                      /iters.gif, iters_zoom.gif   TEST.VIS_VIDEO / TEST.VIS_VIDEO_ZOOM (test.py --vis_video[_zoom])
"""
from __future__ import print_function, division
from collections import namedtuple
import json
import os

import numpy as np

from deepim.core.pose_stages import POST_LOOP, int_setting, stages_on

STYLE_GT, STYLE_INIT, STYLE_REFINED = (191, 191, 191), (0, 0, 255), (0, 255, 0)   # B, G, R: grey 0.75, red, green
HOLD = 5            # a video holds its first and its last frame this many times
ZOOM_IN_STEPS = 3   # frames of the zoom-in in front of a zoomed video
GIF_MS = 400        # per frame
VisSettings = namedtuple("VisSettings", "dir max_pairs radius edge_alpha fill_alpha zoom video video_zoom")


def _bool_setting(T, key, default):
    v = T.get(key, default)
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("TEST.{} must be True or False, got {!r}".format(key, v))
    return bool(v)


def vis_settings(cfg):
    """-> VisSettings of cfg.TEST, every key checked whether VISUALIZE is on or not; ValueError names the bad key.  With VISUALIZE on,
    HYP_NUM > 1 and COARSE_VIEWS > 0 are refused (which hypothesis to draw is not defined), naming both keys."""
    T = cfg.TEST
    d = T.get("VIS_DIR", "")
    if not isinstance(d, str):
        raise ValueError("TEST.VIS_DIR must be a string ('' = <output path>/vis), got {!r}".format(d))
    s = VisSettings(d, int_setting("VIS_MAX_PAIRS", T.get("VIS_MAX_PAIRS", 64), 0, None, "an integer >= 0 (the first pairs; 0 = all)"),
                    int_setting("VIS_RADIUS", T.get("VIS_RADIUS", 1), 0, 3, "an integer in 0..3"),
                    int_setting("VIS_EDGE_ALPHA", T.get("VIS_EDGE_ALPHA", 256), 0, 256, "an integer in 0..256"),
                    int_setting("VIS_FILL_ALPHA", T.get("VIS_FILL_ALPHA", 0), 0, 256, "an integer in 0..256 (0 = no fill)"),
                    _bool_setting(T, "VIS_ZOOM", True), _bool_setting(T, "VIS_VIDEO", False), _bool_setting(T, "VIS_VIDEO_ZOOM", False))
    if bool(T.get("VISUALIZE", False)):
        if int(T.get("HYP_NUM", 1) or 1) > 1:
            raise ValueError("TEST.VISUALIZE cannot be combined with TEST.HYP_NUM > 1 (which hypothesis to draw is not defined)")
        if int(T.get("COARSE_VIEWS", 0) or 0) > 0:
            raise ValueError("TEST.VISUALIZE cannot be combined with TEST.COARSE_VIEWS > 0 (which candidate to draw is not defined)")
        if s.video_zoom and not s.zoom:
            raise ValueError("TEST.VIS_VIDEO_ZOOM needs TEST.VIS_ZOOM (the zoomed frames are its pictures)")
    return s


def vis_dir(cfg):
    """TEST.VIS_DIR, '' meaning <output path>/vis"""
    return cfg.TEST.get("VIS_DIR", "") or os.path.join(cfg.get("output_path", "") or ".", "vis")


def frame_names(test_iter, stages):
    """the frames of a pair in their order: iter_00 .. iter_<test_iter>, then one per post-loop stage that is on, named after it"""
    return ["iter_{:02d}".format(k) for k in range(int(test_iter) + 1)] + [s for s in POST_LOOP if s in stages]


def pair_dir_name(index, class_name):
    return "pair_{:06d}_{}".format(int(index), class_name)


def frame_file(name, zoom=False):
    return "{}{}.png".format(name, "_zoom" if zoom else "")


def zoom_in_name(step):
    return "zoom_in_{}".format(int(step))


def gif_frame_order(names, zoom_in=()):
    """the pictures of a video in their order: the zoom-in (if any), then the frames with the first and the last held HOLD times"""
    names = list(names)
    if not names:
        return list(zoom_in)
    if len(names) == 1:
        return list(zoom_in) + names * HOLD
    return list(zoom_in) + [names[0]] * HOLD + names[1:-1] + [names[-1]] * HOLD


def zoom_in_factors(zf, steps=ZOOM_IN_STEPS):
    """the tool's zoom-in (gen_video_iter_zoom_with_factor.py:261-308): window s of `steps` on the way from the identity window
    (1, 1, 0, 0) to zf = (wx, wy, tx, ty): both sides 1 - s (1 - wx) / steps, the centre (tx, ty) s / steps.  zf (P,4) -> (steps,P,4)"""
    zf = np.asarray(zf, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((steps,) + zf.shape, dtype=np.float64)
    for s in range(1, steps + 1):
        out[s - 1, :, 0] = out[s - 1, :, 1] = 1.0 - s * (1.0 - zf[:, 0]) / steps
        out[s - 1, :, 2:] = zf[:, 2:] * s / steps
    return out.astype(np.float32)


def layer_styles(settings, with_gt, n):
    """style rows {B, G, R, edge_alpha, fill_alpha} of the first n layers of a frame, in paint order: [ground truth,] start, result.
    The fill sits under the result's outline only."""
    rows = ([STYLE_GT + (settings.edge_alpha, 0)] if with_gt else []) + [STYLE_INIT + (settings.edge_alpha, 0),
                                                                         STYLE_REFINED + (settings.edge_alpha, settings.fill_alpha)]
    return np.asarray(rows[:n], dtype=np.int32)


def write_gif(path, frames_bgr):
    from PIL import Image

    imgs = [Image.fromarray(np.ascontiguousarray(f[..., ::-1])) for f in frames_bgr]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=GIF_MS, loop=0)


class PoseVisualizer(object):
    """pred_eval builds one when TEST.VISUALIZE is on and calls draw(batch) behind every refine()."""

    def __init__(self, config, refiner, evaluator):
        import torch
        from lib.hip import ops
        from deepim.symbols.deepIM_flownet import FlowNetHip

        self.torch, self.ops = torch, ops
        self.s = vis_settings(config)
        if int(getattr(refiner, "N", 1)) > 1 or getattr(refiner, "coarse", None) is not None:
            raise ValueError("TEST.VISUALIZE cannot be combined with TEST.HYP_NUM > 1 or TEST.COARSE_VIEWS > 0")
        self.cfg, self.refiner, self.rm = config, refiner, refiner.render_machine
        self.classes = list(evaluator.classes)
        self.dir = vis_dir(config)
        self.stages = [s for s in POST_LOOP if s in stages_on(config)]
        self.names = frame_names(refiner.test_iter, self.stages)
        self.means_bgr = np.asarray(config.network.PIXEL_MEANS, dtype=np.float32).reshape(3)
        P, d = refiner.P, refiner.net.device
        H, W = int(self.rm.height), int(self.rm.width)
        self.size, self.net_size = (H, W), (FlowNetHip.H, FlowNetHip.W)
        Hn, Wn = self.net_size
        F, f32, i32 = len(self.names), torch.float32, torch.int32
        self.P, self.F = P, F
        self.layers = torch.zeros((3, P, H, W), dtype=f32, device=d)
        self.bbox = torch.zeros((3, P, 4), dtype=i32, device=d)
        n_zoom = F if self.s.zoom else 0
        n_zin = ZOOM_IN_STEPS if self.s.video_zoom else 0
        if self.s.zoom:
            self.zlayers = torch.zeros((3, P, Hn, Wn), dtype=f32, device=d)
            self.zimage = torch.zeros((P, 3, Hn, Wn), dtype=f32, device=d)
            self.zf_step = torch.zeros((P, 4), dtype=f32, device=d)
            self.status = torch.zeros((P,), dtype=i32, device=d)
        # one flat buffer = one copy per batch: [counts | zoom factor | frames | zoomed frames | zoom-in frames]
        self.n_counts = (F + n_zoom) * P * 3 * 2 * 4
        parts = [self.n_counts, P * 4 * 4, F * P * H * W * 3, n_zoom * P * Hn * Wn * 3, n_zin * P * Hn * Wn * 3]
        self.off = [int(v) for v in np.concatenate([[0], np.cumsum(parts)])]
        self.flat = torch.zeros((int(self.off[-1]),), dtype=torch.uint8, device=d)
        self.zf = self.flat[self.off[1]:self.off[2]].view(f32).view(P, 4)
        self.frames = self.flat[self.off[2]:self.off[3]].view(F, P, H, W, 3)
        self.zframes = self.flat[self.off[3]:self.off[4]].view(n_zoom, P, Hn, Wn, 3)
        self.zin = self.flat[self.off[4]:self.off[5]].view(n_zin, P, Hn, Wn, 3)
        self.rm.reserve(P)
        self.seen = 0   # pairs behind us: the index of a pair in its directory's name

    def _counts(self, slot, L):
        """the (P,L,2) counts of frame slot `slot` (the full frames, then the zoomed ones): the head of its (P,3,2) area"""
        at = slot * self.P * 3 * 2 * 4
        return self.flat[at:at + self.P * L * 2 * 4].view(self.torch.int32).view(self.P, L, 2)

    def _render(self, pose, slot):
        r = self.refiner
        extra = {"light_intensity": r.light_int[0]} if r.lit else ({"K": r.K_pair} if r.per_pair_K else {})
        P, H, W = self.P, self.size[0], self.size[1]
        self.rm.render_batch(r.batch["class_index"], pose, depth=self.layers[slot].view(P, 1, H, W), bbox=self.bbox[slot], mask_thr=0.0,
                             **extra)

    def _zoom(self, x, zf, out, **kw):
        if self.size == self.net_size:
            return self.ops.zoom_planes(x, zf, out=out, **kw)
        return self.ops.zoom_planes_src(x, zf, out=out, **kw)

    def _zoom_layer(self, slot):
        P, (H, W), (Hn, Wn) = self.P, self.size, self.net_size
        self._zoom(self.layers[slot].view(P, 1, H, W), self.zf, self.zlayers[slot].view(P, 1, Hn, Wn), pre=1, post=1)

    def _paint(self, f, L, with_gt):
        """frame f from the first L layer slots, and its zoomed twin from their zoomed planes"""
        ops, style = self.ops, layer_styles(self.s, with_gt, L)
        image = self.refiner.batch["image_observed"]
        ops.vis_overlay(image, self.layers[:L], style, self.s.radius, self.means_bgr, out=self.frames[f], counts=self._counts(f, L))
        if self.s.zoom:
            ops.vis_overlay(self.zimage, self.zlayers[:L], style, self.s.radius, self.means_bgr, out=self.zframes[f],
                            counts=self._counts(self.F + f, L))

    def draw(self, batch):
        """the frames of the batch that refiner.refine() has just run on -> the directories written (one per drawn pair)"""
        torch, ops, r, s = self.torch, self.ops, self.refiner, self.s
        P, n_it = self.P, r.test_iter
        first, self.seen = self.seen, self.seen + P
        src = torch.as_tensor(batch["src_pose"]).cpu().numpy().astype(np.float64).reshape(P, -1)
        todo = [b for b in range(P) if src[b].sum() != -12 and (s.max_pairs == 0 or first + b < s.max_pairs)]
        if not todo:
            return []
        with_gt = batch.get("pose_observed") is not None
        g = 1 if with_gt else 0          # the slots: [ground truth,] start, result
        start, result = g, g + 1
        if with_gt:
            self._render(torch.as_tensor(batch["pose_observed"]).to(self.layers.device, torch.float32).contiguous(), 0)
        self._render(r.pose_init, start)
        if s.zoom:   # one window per pair for all its frames, from the boxes of the ground truth and the initial render
            ops.zoom_factor(self.bbox[0 if with_gt else start], self.bbox[start], r.pose_init, r.net.K, self.size[0], self.size[1],
                            out=self.zf, status=self.status)
            self._zoom(r.batch["image_observed"], self.zf, self.zimage, add3=r.net.plane_means)
            for slot in range(start + 1):
                self._zoom_layer(slot)
        self._paint(0, start + 1, with_gt)
        poses = [r.pose_init] + [r.poses_iter[k] for k in range(n_it)] + [self.refiner.stages[name].pose for name in self.stages]
        for f in range(1, self.F):
            if f == n_it + 1:   # the stages' frames start from the loop's last pose
                self._render(r.poses_iter[n_it - 1], start)
                if s.zoom:
                    self._zoom_layer(start)
            self._render(poses[f], result)
            if s.zoom:
                self._zoom_layer(result)
            self._paint(f, result + 1, with_gt)
        if s.video_zoom:   # the zoom-in: the plain image in windows on the way from the whole frame to the pair's window
            steps = torch.from_numpy(zoom_in_factors(self.zf.cpu().numpy())).to(self.zf.device)
            none = np.zeros((1, 5), dtype=np.int32)   # alpha 0: the layer leaves every pixel as it is
            for i in range(ZOOM_IN_STEPS):
                self._zoom(r.batch["image_observed"], steps[i].contiguous(), self.zimage, add3=r.net.plane_means)
                ops.vis_overlay(self.zimage, self.zlayers[:1], none, 0, self.means_bgr, out=self.zin[i])
        host = self.flat.cpu().numpy()   # the batch's one copy of frames
        return self._write(batch, host, todo, first, with_gt, torch.stack(poses).cpu().numpy().astype(np.float64))

    def _write(self, batch, host, todo, first, with_gt, poses):
        from PIL import Image
        from lib.utils.pose_error import calc_rt_dist_m

        torch, s, P, F, off = self.torch, self.s, self.P, self.F, self.off
        (H, W), (Hn, Wn) = self.size, self.net_size
        areas = host[:self.n_counts].view(np.int32).reshape(-1, P * 3 * 2)   # per frame slot; its head is the frame's (P,L,2)
        marked = lambda slot, L: areas[slot, :P * L * 2].reshape(P, L, 2)[:, :, 0]  # noqa: E731
        zf = host[off[1]:off[2]].view(np.float32).reshape(P, 4)
        frames = host[off[2]:off[3]].reshape(F, P, H, W, 3)
        zframes = host[off[3]:off[4]].reshape(-1, P, Hn, Wn, 3)
        zin = host[off[4]:off[5]].reshape(-1, P, Hn, Wn, 3)
        cls = torch.as_tensor(batch["class_index"]).cpu().numpy().astype(int)
        gt = torch.as_tensor(batch["pose_observed"]).cpu().numpy().astype(np.float64) if with_gt else None
        who = (["gt"] if with_gt else []) + ["start", "result"]
        written = []
        for b in todo:
            d = os.path.join(self.dir, pair_dir_name(first + b, self.classes[cls[b]]))
            os.makedirs(d, exist_ok=True)
            info = {"pair": first + b, "class": self.classes[cls[b]], "frames": list(self.names), "radius": s.radius,
                    "rot_err": None, "trans_err": None, "zoom_factor": [float(v) for v in zf[b]] if s.zoom else None,
                    "marked_pixels": {}, "marked_pixels_zoom": {} if s.zoom else None}
            if with_gt:
                errs = [calc_rt_dist_m(poses[f, b], gt[b]) for f in range(F)]
                info["rot_err"], info["trans_err"] = [float(e[0]) for e in errs], [float(e[1]) for e in errs]
            for f, name in enumerate(self.names):
                L = len(who) - (1 if f == 0 else 0)
                Image.fromarray(np.ascontiguousarray(frames[f, b, :, :, ::-1])).save(os.path.join(d, frame_file(name)))
                info["marked_pixels"][name] = {w: int(marked(f, L)[b, l]) for l, w in enumerate(who[:L])}   # 0: the pose left the frame
                if s.zoom:
                    Image.fromarray(np.ascontiguousarray(zframes[f, b, :, :, ::-1])).save(os.path.join(d, frame_file(name, zoom=True)))
                    info["marked_pixels_zoom"][name] = {w: int(marked(F + f, L)[b, l]) for l, w in enumerate(who[:L])}
            with open(os.path.join(d, "info.json"), "w") as fh:
                json.dump(info, fh, indent=1, sort_keys=True)
            index = {name: f for f, name in enumerate(self.names)}
            if s.video:
                write_gif(os.path.join(d, "iters.gif"), [frames[index[n], b] for n in gif_frame_order(self.names)])
            if s.video_zoom:
                zoom_in = [zoom_in_name(i + 1) for i in range(ZOOM_IN_STEPS)]
                index.update({n: -(i + 1) for i, n in enumerate(zoom_in)})
                order = gif_frame_order(self.names, zoom_in)
                write_gif(os.path.join(d, "iters_zoom.gif"), [zin[-index[n] - 1, b] if index[n] < 0 else zframes[index[n], b] for n in order])
            written.append(d)
        return written
