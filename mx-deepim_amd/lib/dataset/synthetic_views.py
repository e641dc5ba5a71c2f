"""Seeded synthetic rig for TEST.VIEWS > 1 (deepim/core/views.py, deepim/multiview.py): V calibrated cameras on a ring look at G objects
near the rig origin.  The tables are host arithmetic (ring_rig, rig_samples: the same arguments give the same bytes); the blobs are
built on the device from the render machine, as lib/dataset/synthetic_pairs.py builds its pairs.

Frames: the rig frame has y down and the ring in its x-z plane.  Camera v stands at c_v = radius (sin a_v, 0, -cos a_v) and looks at
the origin with its x axis in the ring's plane; a_v spreads the V cameras evenly over `span_deg` (the default 90: the principal axes
of a two-camera rig are at right angles, so one camera's depth direction is the other's image x).  cam_T_rig[v] = [R_v | -R_v c_v].
Sample b = g V + v shows object g in camera v: pose_gt[b] = cam_T_rig[v] T_g."""
import numpy as np
import torch

from lib.utils import synthetic as syn


def ring_rig(V, radius=0.8, span_deg=90.0, seed=0, K=syn.LINEMOD_K):
    """-> cam_T_rig (V,3,4) float32, K_view (V,3,3) float32: the focal lengths differ by up to 2 %, the principal points by up to 4
    pixels from K (seeded)"""
    V = int(V)
    rng = np.random.default_rng([int(seed), 77])
    az = np.radians(span_deg) * (np.arange(V) / (V - 1.0) - 0.5) if V > 1 else np.zeros(1)
    X, Ks = np.zeros((V, 3, 4)), np.tile(np.asarray(K, np.float64).reshape(1, 3, 3), (V, 1, 1))
    for v, a in enumerate(az):
        c = radius * np.array([np.sin(a), 0.0, -np.cos(a)])
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])   # rows: the camera's axes in the rig frame
        X[v, :, :3], X[v, :, 3] = R, -R @ c
        f = 1.0 + rng.uniform(-0.02, 0.02)
        Ks[v, 0, 0] *= f
        Ks[v, 1, 1] *= f
        Ks[v, :2, 2] += rng.uniform(-4.0, 4.0, 2)
    return X.astype(np.float32), Ks.astype(np.float32)


def rig_samples(G, V, seed, radius=0.8, span_deg=90.0, K=syn.LINEMOD_K, n_classes=1, spread=0.05, noise=None):
    """-> dict of host arrays for B = G V samples: class_index (B,) int32, cam_T_rig (B,3,4), K (B,3,3), pose_rig_gt (G,3,4), pose_gt
    (B,3,4) = cam_T_rig pose_rig_gt, pose_init (B,3,4) = pose_gt perturbed independently per view (noise: keyword arguments of
    lib.utils.synthetic.perturb_pose; the default is a few degrees and millimetres, a pose the loop has already refined).  The objects
    lie within `spread` metres of the rig origin"""
    G, V = int(G), int(V)
    X, Ks = ring_rig(V, radius, span_deg, seed, K)
    rng = np.random.default_rng([int(seed), 78])
    cls = rng.integers(0, n_classes, size=G).astype(np.int32)
    rig_gt = np.stack([np.concatenate([syn.random_rotation(rng), rng.uniform(-spread, spread, (3, 1))], axis=1) for _ in range(G)])
    noise = dict(angle_std=2.0, angle_max=6.0, xy_std=0.002, z_std=0.005) if noise is None else noise
    gt, init = np.zeros((G * V, 3, 4), np.float32), np.zeros((G * V, 3, 4), np.float32)
    for g in range(G):
        for v in range(V):
            Xv = X[v].astype(np.float64)
            T = np.concatenate([Xv[:, :3] @ rig_gt[g][:, :3], (Xv[:, :3] @ rig_gt[g][:, 3] + Xv[:, 3])[:, None]], axis=1)
            gt[g * V + v] = T
            init[g * V + v] = syn.perturb_pose(rng, T, **noise)
    return dict(class_index=np.repeat(cls, V), cam_T_rig=np.tile(X, (G, 1, 1)), K=np.tile(Ks, (G, 1, 1)), pose_rig_gt=rig_gt.astype(np.float32),
                pose_gt=gt, pose_init=init)


class SyntheticViews(object):
    """the samples of rig_samples as Refiner.load takes them.  batch(): dict of CUDA tensors with the blob names of
    lib.utils.synthetic.build_device_batch plus K (B,9), cam_T_rig, pose_gt, pose_rig_gt, depth_observed (the render at the
    ground-truth pose, 0 off the object) and mask_segmentation (B,1,H,W) = the drawn pixels of that render"""

    def __init__(self, config, num_objects, num_views, seed=2333, subdiv=4, device="cuda:0", radius=0.8, span_deg=90.0, noise=None):
        from deepim.symbols.deepIM_flownet import source_size
        from lib.render_hip.render_py_multi import Render_Py

        self.config, self.device, self.seed = config, device, int(seed)
        self.G, self.V = int(num_objects), int(num_views)
        self.classes = list(config.dataset.class_name)
        self.models = syn.make_models(seed=seed, n_models=len(self.classes), subdiv=subdiv)
        self.K = np.asarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float32).reshape(3, 3)
        self.height, self.width = source_size(config)
        self.render_machine = Render_Py(None, self.classes, self.K, width=self.width, height=self.height, zNear=config.dataset.ZNEAR,
                                        zFar=config.dataset.ZFAR, device=device, meshes=self.models)
        self.samples = rig_samples(self.G, self.V, seed, radius=radius, span_deg=span_deg, K=self.K, n_classes=len(self.classes), noise=noise)

    def batch(self, pose_init=None):
        """pose_init: other starting poses (B,3,4) than the samples' own"""
        from lib.hip import ops

        s, d, rm = self.samples, torch.device(self.device), self.render_machine
        B, H, W = self.G * self.V, self.height, self.width
        pm = syn.plane_means(self.config.network.PIXEL_MEANS)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
        cls, K, gt = dev(s["class_index"]), dev(s["K"].reshape(B, 9)), dev(s["pose_gt"])
        init = dev(np.asarray(s["pose_init"] if pose_init is None else pose_init, np.float32))
        img, depth_gt = torch.empty((B, 3, H, W), device=d), torch.empty((B, 1, H, W), device=d)
        rm.render_batch(cls, gt, K=K, image=img, depth=depth_gt, plane_means=pm)
        g = torch.Generator(device=d)
        g.manual_seed(self.seed)
        noise = torch.randint(0, 256, (B, 3, H, W), generator=g, device=d).float() - torch.from_numpy(pm).to(d).view(1, 3, 1, 1)
        image_observed = torch.where(depth_gt > 0, img, noise).contiguous()
        image_rendered, mask_rendered = torch.empty((B, 3, H, W), device=d), torch.empty((B, 1, H, W), device=d)
        mask_observed, bbox = torch.empty((B, 1, H, W), device=d), torch.empty((B, 4), dtype=torch.int32, device=d)
        rm.render_batch(cls, init, K=K, image=image_rendered, mask=mask_rendered, bbox=bbox, plane_means=pm)
        ops.box_mask(bbox, mask_observed)
        return {"image_observed": image_observed, "image_rendered": image_rendered, "mask_observed": mask_observed,
                "mask_rendered": mask_rendered, "src_pose": init, "class_index": cls, "K": K, "cam_T_rig": dev(s["cam_T_rig"]),
                "pose_gt": gt, "pose_rig_gt": dev(s["pose_rig_gt"]), "depth_observed": depth_gt,
                "mask_segmentation": (depth_gt > 0).float().contiguous()}
