"""Seeded synthetic video for the pose tracker (deepim/core/tracker.py): P objects of lib.utils.synthetic.make_models move along smooth
trajectories in front of one camera.  The pose tables are host arithmetic (sequence_poses); a frame is the P objects rendered by the
HIP rasteriser, composed front to back by dim_scene_compose over a seeded textured background, and quantised as a camera would
deliver it: uint8 BGR and uint16 depth (metres * dataset.DEPTH_FACTOR, 0 = no reading).

Trajectories: constant angular velocity in the camera frame, R_k = exp(k [w]) R_0; (u, v) = (tx / tz, ty / tz) linear in k and log tz
linear in k -- the motion dim_track_predict's "velocity" model with damping 1 extrapolates exactly.  Events break them on purpose:
    ("teleport", frame, object, du_px, dv_px)   from `frame` on the object's projected centre is shifted by that many pixels
    ("leave", frame, object)                    from `frame` on the object is outside the image
    ("occluder", frame0, frame1, object, dz, du_px, class)
                                                an untracked extra object in frames [frame0, frame1): of class `class`, at a fixed
                                                rotation, dz metres nearer than `object` and its projected centre du_px pixels beside
                                                the object's.  No trajectory changes, and sequence_poses ignores it

Colours: by default the object textures are uniform in 40..255 and the background in 0..255 per channel -- the two share nearly every
colour, the hard case for colour statistics (TEST.TRACK_SEG).  object_colors / background_colors restrict either to a range per
channel: one (lo, hi) for all three channels or three of them in the frame's B, G, R order; every byte v becomes
lo + round(v (hi - lo) / 255).  None leaves today's bytes.
"""
import numpy as np
import torch

from lib.utils import synthetic as syn

LEAD = 2   # poses in front of frame 0: what Tracker.reset(pose, pose_prev) wants
MAX_LAYERS = 16   # dim_scene_compose's layers per scene: the tracked objects and the occluders of a frame share them


def _so3_exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    K = K / th
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def sequence_poses(num_frames, num_objects, seed, K=syn.LINEMOD_K, W=640, H=480, n_classes=1, events=()):
    """-> class_index (P,) int32 and poses (LEAD + num_frames, P, 3, 4) float32: rows 0 and 1 precede the first frame (row LEAD).
    The objects start side by side (column j of P + 1 across the image, 0.7-1.0 m away), turn 0.2-0.6 degrees and drift up to half
    a pixel per frame in x and y, and change their distance by up to 0.2 % per frame (a hand-held object at video rate).  numpy
    only: the same arguments give the same bytes"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    P, n = int(num_objects), LEAD + int(num_frames)
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_classes, size=P).astype(np.int32)
    poses = np.zeros((n, P, 3, 4), np.float64)
    for j in range(P):
        R0 = syn.random_rotation(rng)
        axis = rng.normal(size=3)
        w = axis / np.linalg.norm(axis) * np.radians(rng.uniform(0.2, 0.6))
        z0, zr = rng.uniform(0.7, 1.0), 1.0 + rng.uniform(-0.002, 0.002)
        px = np.array([W * (j + 1.0) / (P + 1.0) + rng.uniform(-10, 10), H / 2.0 + rng.uniform(-40, 40)])
        dpx = rng.uniform(-0.5, 0.5, size=2)
        for k in range(n):
            shift = np.zeros(2)
            for ev in events:
                if ev[0] == "teleport" and int(ev[2]) == j and k - LEAD >= int(ev[1]):
                    shift += (float(ev[3]), float(ev[4]))
                elif ev[0] == "leave" and int(ev[2]) == j and k - LEAD >= int(ev[1]):
                    shift += (2.0 * W, 0.0)
                elif ev[0] not in ("teleport", "leave", "occluder"):
                    raise ValueError("SyntheticSequence: unknown event {!r} (teleport | leave | occluder)".format(ev[0]))
            u = (px[0] + k * dpx[0] + shift[0] - K[0, 2]) / K[0, 0]
            v = (px[1] + k * dpx[1] + shift[1] - K[1, 2]) / K[1, 1]
            z = z0 * zr ** k
            poses[k, j, :, :3] = _so3_exp(k * w) @ R0
            poses[k, j, :, 3] = (u * z, v * z, z)
    return cls, poses.astype(np.float32)


def occluder_layers(events, t, pose_gt_t, K, seed=0):
    """the occluder events active in frame t -> (class (n,) int32, pose (n,3,4) float32), from the frame's ground-truth poses
    (P,3,4).  An occluder's rotation is fixed over its frames (seeded by its place in `events`)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    cls, poses = [], []
    for i, ev in enumerate(events):
        if ev[0] != "occluder" or not int(ev[1]) <= t < int(ev[2]):
            continue
        obj = np.asarray(pose_gt_t[int(ev[3])], np.float64)
        z = obj[2, 3] - float(ev[4])
        u = obj[0, 3] / obj[2, 3] + float(ev[5]) / K[0, 0]
        v = obj[1, 3] / obj[2, 3]
        R = syn.random_rotation(np.random.default_rng([int(seed), 101, i]))
        poses.append(np.concatenate([R, np.array([[u * z], [v * z], [z]])], axis=1))
        cls.append(int(ev[6]))
    return np.asarray(cls, np.int32), np.asarray(poses, np.float32).reshape(-1, 3, 4)


def background(seed, H, W, cell=4):
    """(H,W,3) uint8: seeded random colour cells of `cell` pixels under a smooth gradient"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=((H + cell - 1) // cell, (W + cell - 1) // cell, 3))
    img = np.kron(base, np.ones((cell, cell, 1), dtype=np.int64))[:H, :W]
    gy, gx = np.linspace(0, 40, H).astype(np.int64), np.linspace(0, 40, W).astype(np.int64)
    return np.clip(img - gy[:, None, None] + gx[None, :, None] // 2, 0, 255).astype(np.uint8)


def color_ranges(ranges, what):
    """None, (lo, hi) or ((lo, hi),) * 3 in B, G, R order -> None or a (3,2) int64 array with 0 <= lo <= hi <= 255"""
    if ranges is None:
        return None
    a = np.asarray(ranges, np.int64)
    if a.shape == (2,):
        a = np.tile(a, (3, 1))
    if a.shape != (3, 2) or (a < 0).any() or (a > 255).any() or (a[:, 0] > a[:, 1]).any():
        raise ValueError("SyntheticSequence: {} must be (lo, hi) or three of them (B, G, R) with 0 <= lo <= hi <= 255, got {!r}".format(
            what, ranges))
    return a


def restrict_colors(img, ranges):
    """uint8 (...,3) whose channels are in the order of `ranges` (3,2): every byte v -> lo + round(v (hi - lo) / 255)"""
    lo, span = ranges[:, 0], ranges[:, 1] - ranges[:, 0]
    return (lo + (np.asarray(img, np.uint8).astype(np.int64) * span + 127) // 255).astype(np.uint8)


class SyntheticSequence(object):
    def __init__(self, config, num_frames, num_objects, seed, device="cuda:0", events=(), subdiv=4, model_seed=None, object_colors=None,
                 background_colors=None):
        """seed: of the trajectories, the background and (model_seed None) the meshes; model_seed: the meshes' own seed, so that
        several videos show the same objects; object_colors / background_colors: the colour ranges of the textures and the background"""
        from deepim.symbols.deepIM_flownet import source_size

        self.config, self.device = config, device
        self.num_frames, self.P, self.seed, self.events = int(num_frames), int(num_objects), seed, tuple(events)
        self.classes = list(config.dataset.class_name)
        self.K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float32).reshape(3, 3)
        self.height, self.width = source_size(config)
        self.depth_factor = float(config.dataset.DEPTH_FACTOR)
        self.subdiv, self.model_seed = subdiv, seed if model_seed is None else model_seed
        self.object_colors = color_ranges(object_colors, "object_colors")
        self.background_colors = color_ranges(background_colors, "background_colors")
        self.class_index, self.poses = sequence_poses(self.num_frames, self.P, seed, K=self.K, W=self.width, H=self.height,
                                                      n_classes=len(self.classes), events=self.events)
        self.pose_gt = self.poses[LEAD:]        # (T,P,3,4): the pose of every object in every frame
        self.pose_start = self.poses[:LEAD]     # (2,P,3,4): the two poses before frame 0, oldest first
        for ev in self.events:
            if ev[0] == "occluder" and not (0 <= int(ev[3]) < self.P and 0 <= int(ev[6]) < len(self.classes)):
                raise ValueError("SyntheticSequence: occluder event {!r} names an object outside 0..{} or a class outside 0..{}".format(
                    ev, self.P - 1, len(self.classes) - 1))
        for t in range(self.num_frames):
            n = self.P + len(occluder_layers(self.events, t, self.pose_gt[t], self.K, seed)[0])
            if n > MAX_LAYERS:
                raise ValueError("SyntheticSequence: {} tracks and occluders in frame {}: dim_scene_compose takes {} layers".format(
                    n, t, MAX_LAYERS))
        self._models = self._rm = self._bg = None

    def __len__(self):
        return self.num_frames

    @property
    def models(self):
        if self._models is None:
            self._models = syn.make_models(seed=self.model_seed, n_models=len(self.classes), subdiv=self.subdiv)
            if self.object_colors is not None:   # the textures are R, G, B
                self._models = [(v, t, f, restrict_colors(tex, self.object_colors[::-1])) for v, t, f, tex in self._models]
        return self._models

    @property
    def render_machine(self):
        if self._rm is None:
            from lib.render_hip.render_py_multi import Render_Py

            cfg = self.config
            self._rm = Render_Py(None, self.classes, self.K, width=self.width, height=self.height, zNear=cfg.dataset.ZNEAR,
                                 zFar=cfg.dataset.ZFAR, device=self.device, meshes=self.models)
        return self._rm

    def frame(self, t):
        """-> dict(frame_bgr (H,W,3) uint8, depth_raw (H,W) uint16, pose_gt (P,3,4) float32), on the device"""
        from lib.hip import ops

        d, P, H, W = torch.device(self.device), self.P, self.height, self.width
        rm = self.render_machine
        if self._bg is None:
            bg = background(self.seed + 7, H, W)
            if self.background_colors is not None:
                bg = restrict_colors(bg, self.background_colors)
            self._bg = torch.from_numpy(bg).to(d)
            self._cls = torch.from_numpy(self.class_index).to(d)
        pose = torch.from_numpy(np.ascontiguousarray(self.pose_gt[t])).to(d)
        cls, layer_pose, S = self._cls, pose, P
        occ_cls, occ_pose = occluder_layers(self.events, t, self.pose_gt[t], self.K, self.seed)
        if len(occ_cls):   # untracked extra layers behind the tracked ones
            cls = torch.cat([cls, torch.from_numpy(occ_cls).to(d)])
            layer_pose = torch.cat([pose, torch.from_numpy(occ_pose).to(d)])
            S = P + len(occ_cls)
        layer_bgr = torch.empty((S, H, W, 3), device=d)
        layer_depth = torch.empty((S, 1, H, W), device=d)
        rm.render_batch(cls, layer_pose, bgr=layer_bgr, depth=layer_depth)
        scene_bgr = torch.empty((1, H, W, 3), device=d)
        scene_depth = torch.empty((1, 1, H, W), device=d)
        ops.scene_compose(layer_bgr, layer_depth, cls + 1, S, scene_bgr=scene_bgr, scene_depth=scene_depth)
        drawn = scene_depth[0, 0] > 0
        bgr = torch.where(drawn[..., None], scene_bgr[0].round().clamp(0, 255).to(torch.uint8), self._bg).contiguous()
        mm = (scene_depth[0, 0] * self.depth_factor).round().clamp(0, 32767).to(torch.int16)   # (no uint16 arithmetic: the same bytes)
        return {"frame_bgr": bgr, "depth_raw": mm.contiguous().view(torch.uint16), "pose_gt": pose}

    def frames(self, reinit_from_gt=False):
        """the frames as Tracker.run takes them; reinit_from_gt: every frame offers the ground truth as its re-initialisation pose"""
        for t in range(self.num_frames):
            f = self.frame(t)
            if reinit_from_gt:
                f["reinit_pose"] = f["pose_gt"]
            yield f
