"""Synthetic LINEMOD-shaped inputs (no dataset offline).  numpy only, no rendering here.

Definition follows SURVEY.md 8(d): procedurally generated closed meshes (displaced icospheres,
diameter 0.1-0.3 m) with a seeded texture; GT pose uniform on SO(3), z ~ U(0.6,1.2) m with the
projected centre >= 16 px inside the image; initial pose = GT (+) noise with the reference's
training-pair distribution (toolkit/LM6d_1_gen_rendered_pose.py:59,98-117: Euler N(0,15 deg) per
axis rejected above 45 deg, dx,dy ~ N(0,0.01 m), dz ~ N(0,0.05 m)).
"""
import numpy as np

LINEMOD_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], dtype=np.float32)  # config.py:63-65
PIXEL_MEANS = np.array([123.68, 116.779, 103.939], dtype=np.float32)  # cfgs/*.yaml network.PIXEL_MEANS


def icosphere(subdiv):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int32)


def make_mesh(rng, subdiv=4, diameter=0.2):
    """closed star-shaped mesh: icosphere displaced by a few low-order lobes, anisotropically scaled."""
    v, f = icosphere(subdiv)
    r = np.ones(len(v))
    for _ in range(4):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        r += rng.uniform(0.05, 0.25) * np.cos(rng.integers(2, 5) * np.arccos(np.clip(v @ d, -1, 1)))
    p = v * r[:, None] * rng.uniform(0.6, 1.0, size=3)[None, :]
    p -= p.mean(axis=0, keepdims=True)
    ext = np.linalg.norm(p[:, None, :] - p[None, ::7, :], axis=2).max() if len(p) < 4000 else 2 * np.linalg.norm(p, axis=1).max()
    p *= diameter / ext
    # spherical texture coordinates in [0,1]
    u = 0.5 + np.arctan2(v[:, 1], v[:, 0]) / (2 * np.pi)
    w = 0.5 + np.arcsin(np.clip(v[:, 2], -1, 1)) / np.pi
    return p.astype(np.float32), np.stack([u, w], axis=1).astype(np.float32), f


def make_texture(rng, size=512, cells=32):
    """blocky random colours with a smooth gradient: distinct texels, no pure-black (mask = depth, not colour)."""
    base = rng.integers(40, 256, size=(cells, cells, 3))
    tex = np.kron(base, np.ones((size // cells, size // cells, 1), dtype=np.int64))
    g = np.linspace(0, 30, size).astype(np.int64)
    tex = np.clip(tex - g[:, None, None] + g[None, :, None] // 2, 1, 255)
    return tex.astype(np.uint8)


def make_models(seed=2333, n_models=1, subdiv=4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_models):
        v, t, f = make_mesh(rng, subdiv=subdiv, diameter=float(rng.uniform(0.1, 0.3)))
        out.append((v, t, f, make_texture(rng)))
    return out


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def euler_xyz(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def sample_gt_pose(rng, K=LINEMOD_K, W=640, H=480, margin=120):
    """margin keeps the whole (<=0.3 m) object inside the frame at z >= 0.6 m."""
    R = random_rotation(rng)
    z = rng.uniform(0.6, 1.2)
    u = rng.uniform(margin, W - margin)
    v = rng.uniform(margin, H - margin)
    x = (u - K[0, 2]) * z / K[0, 0]
    y = (v - K[1, 2]) * z / K[1, 1]
    return np.concatenate([R, np.array([[x], [y], [z]])], axis=1).astype(np.float32)


def perturb_pose(rng, pose, angle_std=15.0, angle_max=45.0, xy_std=0.01, z_std=0.05):
    while True:
        e = np.deg2rad(rng.normal(0, angle_std, size=3))
        Rn = euler_xyz(*e)
        ang = np.rad2deg(np.arccos(np.clip((np.trace(Rn) - 1) / 2, -1, 1)))
        if ang <= angle_max:
            break
    out = np.array(pose, dtype=np.float64)
    out[:, :3] = Rn @ out[:, :3]
    out[:, 3] += np.array([rng.normal(0, xy_std), rng.normal(0, xy_std), rng.normal(0, z_std)])
    return out.astype(np.float32)


def sample_pairs(seed, B, n_classes=1, frame=None, **noise):
    """-> class_index (B,) int32, pose_gt (B,3,4), pose_init (B,3,4), background seeds.
    frame: None (the 640x480 LINEMOD camera) or (K, W, H) of another image size (config.SCALES): the same draws place the object in
    that frame, the margin scaled with its width.
    noise: keyword arguments of perturb_pose (angle_std, angle_max, xy_std, z_std) for pairs with another initial error."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_classes, size=B).astype(np.int32)
    where = {} if frame is None else dict(K=np.asarray(frame[0], np.float64).reshape(3, 3), W=frame[1], H=frame[2], margin=120.0 * frame[1] / 640.0)
    gt = np.stack([sample_gt_pose(rng, **where) for _ in range(B)])
    init = np.stack([perturb_pose(rng, gt[i], **noise) for i in range(B)])
    return cls, gt, init


def bgr_to_blob(bgr_uint8, pixel_means=PIXEL_MEANS):
    """lib/utils/image.py:709-720 transform(): plane c = im[:,:,2-c] - pixel_means[2-c]  ((1,3,H,W) f32)."""
    im = np.asarray(bgr_uint8, dtype=np.float32)
    out = np.zeros((1, 3, im.shape[0], im.shape[1]), dtype=np.float32)
    for i in range(3):
        out[0, i] = im[:, :, 2 - i] - pixel_means[2 - i]
    return out


def plane_means(pixel_means=PIXEL_MEANS):
    """per-plane constants of the network blobs: PIXEL_MEANS reversed (zoom_image_with_factor.py:94)."""
    return np.asarray(pixel_means, dtype=np.float32).reshape(3)[::-1].copy()


def box_from_mask(mask):
    """filled END-EXCLUSIVE bbox rectangle of a binary mask (lib/utils/image.py:437-460, data_pair.py:103-114)."""
    out = np.zeros(mask.shape, dtype=np.float32)
    nz_x = np.nonzero(mask.max(axis=0))[0]
    nz_y = np.nonzero(mask.max(axis=1))[0]
    if len(nz_x) and len(nz_y):
        out[nz_y.min():nz_y.max(), nz_x.min():nz_x.max()] = 1.0
    return out


def compose_observed(bgr_render, depth_render, rng):
    """observed image = render at the GT pose over a seeded uniform-noise background, uint8."""
    bg = rng.integers(0, 256, size=bgr_render.shape).astype(np.float32)
    fg = (depth_render > 0)[..., None]
    return np.where(fg, bgr_render, bg).astype(np.uint8)


def build_device_batch(render_machine, B, seed, n_classes=1, pixel_means=PIXEL_MEANS, device="cuda:0", noise=None, with_depth=False):
    """Synthetic test batch built ON the GPU with the HIP rasteriser (bench / smoke inputs):
    observed = render at the GT pose over seeded uniform noise, uint8-quantised; rendered = render at the
    perturbed pose; mask_rendered = depth > 0.2; mask_observed = bbox rectangle of it (TEST.INIT_MASK box_rendered).
    Returns dict of CUDA tensors with the reference's blob names + pose_gt.
    with_depth: also depth_gt_observed (the render at the GT pose: zero off the object) and depth_rendered (the render at the initial
    pose), the two planes par_generate_gt reads for the test-time flow error (deepim/core/tester.py:681-704)."""
    import torch

    from lib.hip import ops

    d = torch.device(device)
    H, W = render_machine.height, render_machine.width
    frame = None if (H, W) == (480, 640) else (render_machine.K, W, H)   # another image size (config.SCALES): its own camera
    cls, gt, init = sample_pairs(seed, B, n_classes, frame=frame, **(noise or {}))
    pm = plane_means(pixel_means)
    cls_t = torch.from_numpy(cls).to(d)
    img = torch.empty((B, 3, H, W), device=d)
    depth = torch.empty((B, 1, H, W), device=d)
    render_machine.render_batch(cls_t, torch.from_numpy(gt).to(d), image=img, depth=depth, plane_means=pm)
    g = torch.Generator(device=d)
    g.manual_seed(seed)
    noise = torch.randint(0, 256, (B, 3, H, W), generator=g, device=d).float() - torch.from_numpy(pm).to(d).view(1, 3, 1, 1)
    image_observed = torch.where(depth > 0, img, noise).contiguous()
    depth_gt = depth.clone() if with_depth else None
    image_rendered = torch.empty((B, 3, H, W), device=d)
    mask_rendered = torch.empty((B, 1, H, W), device=d)
    mask_observed = torch.empty((B, 1, H, W), device=d)
    bbox = torch.empty((B, 4), dtype=torch.int32, device=d)
    render_machine.render_batch(cls_t, torch.from_numpy(init).to(d), image=image_rendered, depth=depth, mask=mask_rendered, bbox=bbox,
                                plane_means=pm)
    ops.box_mask(bbox, mask_observed)
    out = {"image_observed": image_observed, "image_rendered": image_rendered, "mask_observed": mask_observed,
           "mask_rendered": mask_rendered, "src_pose": torch.from_numpy(init).to(d), "class_index": cls_t,
           "pose_gt": torch.from_numpy(gt).to(d)}
    if with_depth:
        out.update(depth_gt_observed=depth_gt, depth_rendered=depth)
    return out


def build_device_train_batch(render_machine, B, seed, models, n_classes=1, pixel_means=PIXEL_MEANS, npts=3000, device="cuda:0", noise=None,
                             occluders=0, lit=False, occ_max_rate=0.85, light_machine=None, distractors=None):
    """build_device_batch + the training blobs/labels (reference names, deepim/core/loader.py:164-193): mask_gt_observed, tgt_pose,
    depth_gt_observed, rot/trans labels, flow/flow_weights (depth->flow kernel), point clouds.
    occluders = k > 0 and / or lit: the observed side becomes an occluded and / or lit scene (build_device_scene_batch, which
    documents the remaining arguments); with both at their defaults nothing else is launched or allocated."""
    import torch

    from lib.hip import ops

    b = build_device_batch(render_machine, B, seed, n_classes=n_classes, pixel_means=pixel_means, device=device, noise=noise)
    d = torch.device(device)
    H, W = render_machine.height, render_machine.width
    K = render_machine.K
    gt, init = b["pose_gt"], b["src_pose"]
    depth_gt = torch.empty((B, 1, H, W), device=d)
    depth_r = torch.empty((B, 1, H, W), device=d)
    mask_gt = torch.empty((B, 1, H, W), device=d)
    render_machine.render_batch(b["class_index"], gt, depth=depth_gt, mask=mask_gt, mask_thr=0.0)
    render_machine.render_batch(b["class_index"], init, depth=depth_r)
    z3, o3 = np.zeros(3, np.float32), np.ones(3, np.float32)
    rot, trans = ops.se3_delta(init, gt, "CAMERA", z3, o3)
    KT = ops.pose_to_KT(init, gt, K)
    flow, valid = ops.depth_to_flow(depth_r, depth_gt, KT, np.linalg.inv(K).astype(np.float32))
    rng = np.random.default_rng(seed + 17)
    cls = b["class_index"].cpu().numpy()
    gt_np = gt.cpu().numpy()
    pm, po = [], []
    for i in range(B):
        v = models[int(cls[i])][0]
        P = np.ascontiguousarray(v[rng.integers(0, v.shape[0], size=npts)].T.astype(np.float32))
        pm.append(P[None])
        po.append((gt_np[i][:, :3] @ P + gt_np[i][:, 3:4]).astype(np.float32)[None])
    b.update(mask_gt_observed=mask_gt, tgt_pose=gt.clone(), depth_gt_observed=depth_gt, rot=rot, trans=trans, flow=flow,
             flow_weights=valid.repeat(1, 2, 1, 1).contiguous(), point_cloud_model=torch.from_numpy(np.concatenate(pm)).to(d),
             point_cloud_weights=torch.ones((B, 3, npts), device=d), point_cloud_observed=torch.from_numpy(np.concatenate(po)).to(d))
    if int(occluders) > 0 or lit:
        b.update(build_device_scene_batch(render_machine, b, seed, models, occluders=int(occluders), lit=bool(lit), n_classes=n_classes,
                                          pixel_means=pixel_means, device=device, occ_max_rate=occ_max_rate, light_machine=light_machine,
                                          distractors=distractors))
    return b


# toolkit/LM6d_occ_dsm_1_gen_observed_light.py:98, :130-156
LM_BRIGHTNESS_RATIOS = [0.2, 0.25, 0.3, 0.35, 0.4]
LM_LIGHT_DIRS = [[1, 0, 1], [1, 1, 1], [0, 1, 1], [-1, 1, 1], [-1, 0, 1], [0, 0, 1]]
LM_LIGHT_COLORS = [[0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]


def lm_light_draw(seed, idx, pose_0, n_ratios=len(LM_BRIGHTNESS_RATIOS)):
    """The light of one "deep synthetic" LINEMOD scene (toolkit/LM6d_occ_dsm_1_gen_observed_light.py:130-162, :187-192).
    -> light_position (3,) f64 in GL camera coordinates, light_intensity (3,) f64, brightness ratio index.
      position  = LM_LIGHT_DIRS[idx % 6] * 0.5 + (tx, -ty, -tz) of pose_0, the scene's first pose (3x4)
      intensity = LM_LIGHT_COLORS[c] * U(0.8, 1.2)^3
    Draws, in this order, from np.random.default_rng(seed) (the reference draws from the global numpy / random state):
      1. intensity factors  rng.uniform(0.8, 1.2, size=3)
      2. colour row         c = rng.integers(0, 7)
      3. ratio index        rng.integers(0, n_ratios)"""
    rng = np.random.default_rng(seed)
    factors = rng.uniform(0.8, 1.2, size=3)
    c = int(rng.integers(0, len(LM_LIGHT_COLORS)))
    k = int(rng.integers(0, n_ratios))
    pose_0 = np.asarray(pose_0, dtype=np.float64)
    lp = np.array(LM_LIGHT_DIRS[idx % 6], dtype=np.float64) * 0.5
    lp[0] += pose_0[0, 3]
    lp[1] -= pose_0[1, 3]
    lp[2] -= pose_0[2, 3]
    return lp, np.array(LM_LIGHT_COLORS[c], dtype=np.float64) * factors, k


def target_box(verts, pose, K=LINEMOD_K, W=640, H=480):
    """(x0, x1, y0, y1) of the projected model vertices, clipped to the image (host side: no device round trip)"""
    P = np.asarray(verts, np.float64) @ np.asarray(pose[:, :3], np.float64).T + np.asarray(pose[:, 3], np.float64)
    u = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2]
    v = K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
    return (float(np.clip(u.min(), 0, W - 1)), float(np.clip(u.max(), 0, W - 1)), float(np.clip(v.min(), 0, H - 1)),
            float(np.clip(v.max(), 0, H - 1)))


def sample_distractors(seed, cls, gt, models, k, n_classes=1, K=LINEMOD_K, W=640, H=480, z_min=0.4):
    """k occluding objects per pair -> classes (B,k) int32, poses (B,k,3,4) f32.  Draws from np.random.default_rng(seed), per pair
    and distractor in order: class (another one than the target's: rng.integers(0, n_classes - 1), skipping the target's; the same
    class when there is only one), rotation (random_rotation: 4 normals), depth z = z_target + U(-0.3, 0.3) (not below z_min), projected
    centre u ~ U(x0, x1), v ~ U(y0, y1) inside the target's box (target_box)."""
    rng = np.random.default_rng(seed)
    B = len(cls)
    dc = np.zeros((B, k), np.int32)
    dp = np.zeros((B, k, 3, 4), np.float32)
    for b in range(B):
        x0, x1, y0, y1 = target_box(models[int(cls[b])][0], gt[b], K, W, H)
        for j in range(k):
            if n_classes > 1:
                c = int(rng.integers(0, n_classes - 1))
                c += int(c >= int(cls[b]))
            else:
                c = int(cls[b])
            R = random_rotation(rng)
            z = max(float(gt[b][2, 3]) + rng.uniform(-0.3, 0.3), z_min)
            u, v = rng.uniform(x0, x1), rng.uniform(y0, y1)
            t = np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z])
            dc[b, j] = c
            dp[b, j] = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
    return dc, dp


def build_device_scene_batch(render_machine, batch, seed, models, occluders=0, lit=False, n_classes=1, pixel_means=PIXEL_MEANS,
                             device="cuda:0", occ_max_rate=0.85, light_machine=None, distractors=None):
    """The observed side of a training batch as an occluded, lit multi-object scene, composed on the device (stands in for
    toolkit/LM6d_occ_dsm_1_gen_observed_light.py and LM6d_occ_dsm_3_remove_low_visible.py).  `batch`: what build_device_train_batch
    built for the same seed (class_index, pose_gt, depth_gt_observed, mask_gt_observed).  Per pair the target is layer 0 at the
    ground-truth pose and `occluders` distractors (sample_distractors, seed + 29; or `distractors` = (classes (B,k), poses
    (B,k,3,4)) host arrays) are layers 1..k; all B*(k+1) layers are rendered in one render_batch -- by `light_machine` (a
    Render_Py_Light_MultiProgram over the same meshes) under lm_light_draw((seed, b), b, target pose) when lit; the brightness ratio
    of the batch is pair 0's draw, being one kernel argument -- and composed by dim_scene_compose.
    -> the blobs to replace, with the reference's meaning:
       image_observed    the scene over the seeded noise background of build_device_batch
       mask_gt_observed  the target's visible mask (the reference: label == mask_idx)
       depth_observed    the scene depth           (depth_gt_observed stays the target's own unoccluded render)
    plus scene_label (B,1,H,W), occ_counts (B,2) int32 {full, visible} of the target and occ_kept (B,) bool.
    A pair whose target has visible < (1 - occ_max_rate) * full keeps its unoccluded image, mask and depth; the choice is made on
    the device from the counts (no host round trip)."""
    import torch

    from lib.hip import ops

    d = torch.device(device)
    k = int(occluders)
    S = k + 1
    rm = light_machine if lit else render_machine
    if lit and light_machine is None:
        raise ValueError("lit scenes need light_machine (lib.render_hip.render_py_light_multi_program.Render_Py_Light_MultiProgram)")
    H, W = rm.height, rm.width
    B = batch["pose_gt"].shape[0]
    cls = batch["class_index"].cpu().numpy()
    gt = batch["pose_gt"].cpu().numpy()
    if k > 0:
        dc, dp = distractors if distractors is not None else sample_distractors(seed + 29, cls, gt, models, k, n_classes, rm.K, W, H)
        lc = np.concatenate([cls.reshape(B, 1), np.asarray(dc, np.int32).reshape(B, k)], axis=1)
        lp = np.concatenate([gt.reshape(B, 1, 3, 4), np.asarray(dp, np.float32).reshape(B, k, 3, 4)], axis=1)
    else:
        lc, lp = cls.reshape(B, 1), gt.reshape(B, 1, 3, 4)
    cls_l = torch.from_numpy(np.ascontiguousarray(lc.reshape(B * S).astype(np.int32))).to(d)
    pose_l = torch.from_numpy(np.ascontiguousarray(lp.reshape(B * S, 3, 4).astype(np.float32))).to(d)
    layer_bgr = torch.empty((B * S, H, W, 3), device=d)
    layer_depth = torch.empty((B * S, 1, H, W), device=d)
    if lit:
        draws = [lm_light_draw((seed, b), b, gt[b], len(rm.brightness_ratios)) for b in range(B)]
        pos = np.repeat(np.stack([x[0] for x in draws]), S, axis=0).astype(np.float32)
        inten = np.repeat(np.stack([x[1] for x in draws]), S, axis=0).astype(np.float32)
        rm.render_batch(cls_l, pose_l, torch.from_numpy(pos).to(d), torch.from_numpy(inten).to(d), brightness_k=draws[0][2], bgr=layer_bgr,
                        depth=layer_depth)
    else:
        rm.render_batch(cls_l, pose_l, bgr=layer_bgr, depth=layer_depth)
    scene_bgr = torch.empty((B, H, W, 3), device=d)
    scene_depth = torch.empty((B, 1, H, W), device=d)
    scene_label = torch.empty((B, 1, H, W), device=d)
    vis = torch.empty((B * S, 1, H, W), device=d)
    counts = torch.empty((B * S, 2), dtype=torch.int32, device=d)
    ops.scene_compose(layer_bgr, layer_depth, cls_l + 1, S, scene_bgr=scene_bgr, scene_depth=scene_depth, scene_label=scene_label,
                      vis_mask=vis, counts=counts)
    cnt = counts.view(B, S, 2)[:, 0].contiguous()
    kept = ~(cnt[:, 1].double() < (1.0 - float(occ_max_rate)) * cnt[:, 0].double())
    sel = kept.view(B, 1, 1, 1)
    pm = torch.from_numpy(plane_means(pixel_means)).to(d).view(1, 3, 1, 1)
    g = torch.Generator(device=d)
    g.manual_seed(seed)   # the background of build_device_batch, bit for bit
    noise = torch.randint(0, 256, (B, 3, H, W), generator=g, device=d).float() - pm
    layer0_bgr = layer_bgr.view(B, S, H, W, 3)[:, 0]
    layer0_depth = layer_depth.view(B, S, 1, H, W)[:, 0]
    to_blob = lambda bgr: bgr.permute(0, 3, 1, 2).flip(1) - pm  # noqa: E731  (plane c = bgr[..., 2 - c] - plane mean c)
    occluded = torch.where(scene_depth > 0, to_blob(scene_bgr), noise)
    alone = torch.where(layer0_depth > 0, to_blob(layer0_bgr), noise)
    return {"image_observed": torch.where(sel, occluded, alone).contiguous(),
            "mask_gt_observed": torch.where(sel, vis.view(B, S, 1, H, W)[:, 0], batch["mask_gt_observed"]).contiguous(),
            "depth_observed": torch.where(sel, scene_depth, layer0_depth).contiguous(),
            "scene_label": torch.where(sel, scene_label, (layer0_depth > 0).float() * (cls_l.view(B, S)[:, :1] + 1).float().view(B, 1, 1, 1)),
            "occ_counts": cnt, "occ_kept": kept}
