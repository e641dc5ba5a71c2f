"""Coarse pose from a 2-D detection box: the front stage of a pipeline that starts from a detector (class and box per object).

Per pair, M = COARSE_VIEWS x COARSE_INPLANE candidate rotations on a viewpoint grid, each with the translation at which the projected
model fills the box (dim_pose_from_box); all P*M candidates are rendered and scored against the pair's one observed frame
(dim_pose_score_indexed: no copy of the frame per candidate, no network) and the k best of each pair kept (dim_hyp_topk).  The
Refiner feeds them to its loop as hyp_poses.  Restated in float64 numpy by tests/coarse_reference.py.
"""
from __future__ import print_function, division

import numpy as np
import torch

from lib.hip import ops

COARSE_SCORES = ("rgb", "depth")
MAX_CANDIDATES = 65535   # dim_pose_from_box / dim_hyp_topk: candidates per pair


def coarse_rotations(n_views, n_inplane):
    """(M,3,3) float64, M = n_views * n_inplane, entry m = v * n_inplane + j.  View v looks at the object from direction d_v of a
    Fibonacci sphere (z = 1 - (2v+1)/n_views, r = sqrt(1-z^2), phi = v pi (3 - sqrt 5), d = (r cos phi, r sin phi, z): the sphere of
    hypothesis_rotations); the rows of R_view are the camera axes in the object frame, z_c = -d, x_c = normalise(up x z_c),
    y_c = z_c x x_c, up = (0,0,1) or (0,1,0) when |d_z| > 0.999; R = Rz(2 pi j / n_inplane) R_view turns the image about the optical axis."""
    R = np.zeros((n_views * n_inplane, 3, 3))
    for v in range(n_views):
        z = 1.0 - (2.0 * v + 1.0) / n_views
        r, phi = np.sqrt(max(0.0, 1.0 - z * z)), v * np.pi * (3.0 - np.sqrt(5.0))
        d = np.array([r * np.cos(phi), r * np.sin(phi), z])
        zc = -d
        up = np.array([0.0, 1.0, 0.0]) if abs(d[2]) > 0.999 else np.array([0.0, 0.0, 1.0])
        xc = np.cross(up, zc)
        xc /= np.linalg.norm(xc)
        yc = np.cross(zc, xc)
        Rv = np.stack([xc, yc, zc])
        for j in range(n_inplane):
            a = 2.0 * np.pi * j / n_inplane
            Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            R[v * n_inplane + j] = Rz @ Rv
    return R


def _int_key(T, key, default, least):
    v = T.get(key, default)
    if v is None or isinstance(v, (bool, str)) or not np.isfinite(float(v)) or not float(v).is_integer() or int(v) < least:
        raise ValueError("TEST.{} must be an integer >= {}, got {!r}".format(key, least, v))
    return int(v)


def _pos_key(T, key, default, what):
    v = T.get(key, default)
    if v is None or isinstance(v, (bool, str)) or not (np.isfinite(float(v)) and float(v) > 0):
        raise ValueError("TEST.{} must be a finite {} > 0, got {!r}".format(key, what, v))
    return float(v)


def coarse_settings(cfg):
    """-> (COARSE_VIEWS (0 = off), COARSE_INPLANE, COARSE_BOX_ITER, COARSE_Z_INIT, COARSE_SCORE, COARSE_DEPTH_TAU, COARSE_CHUNK) of
    cfg.TEST, checked; ValueError names the bad key"""
    T = cfg.TEST
    views = _int_key(T, "COARSE_VIEWS", 0, 0)
    inplane = _int_key(T, "COARSE_INPLANE", 1, 1)
    if views * inplane > MAX_CANDIDATES:
        raise ValueError("TEST.COARSE_VIEWS x TEST.COARSE_INPLANE = {} candidates per pair, at most {}".format(views * inplane, MAX_CANDIDATES))
    iters = _int_key(T, "COARSE_BOX_ITER", 8, 1)
    z_init = _pos_key(T, "COARSE_Z_INIT", 1.0, "distance (metres)")
    score = T.get("COARSE_SCORE", "rgb")
    if score not in COARSE_SCORES:
        raise ValueError("TEST.COARSE_SCORE must be one of {}, got {!r}".format(COARSE_SCORES, score))
    tau = _pos_key(T, "COARSE_DEPTH_TAU", 0.02, "distance (metres)")
    chunk = _int_key(T, "COARSE_CHUNK", 256, 1)
    return views, inplane, iters, z_init, score, tau, chunk


def boxes_from_int(bbox):
    """inclusive int boxes (P,4) {min_x,max_x,min_y,max_y} (dim_mask_bbox's convention) -> the continuous extents {x0,x1,y0,y1} that
    dim_pose_from_box takes: pixel centres lie at integers, so a pixel reaches half a pixel to each side.  Tensor in, f32 tensor out."""
    half = torch.tensor([-0.5, 0.5, -0.5, 0.5], dtype=torch.float32, device=bbox.device)
    return bbox.to(torch.float32) + half


def mesh_point_tables(render_machine):
    """the vertices of the render machine's meshes as the point tables of dim_pose_from_box: (points (Vtot,3) float64, table_off
    (n_classes+1,) int32), for a caller without an evaluator's model points"""
    mt = render_machine.mesh_table.cpu().numpy()
    assert all(int(mt[c, 0]) == int(mt[:c, 1].sum()) for c in range(len(mt))), "mesh table: the classes' vertices are not consecutive"
    off = np.concatenate([[0], np.cumsum(mt[:, 1])]).astype(np.int32)
    return render_machine.verts.to(torch.float64).contiguous(), torch.from_numpy(off).to(render_machine.verts.device)


class CoarseInit(object):
    """The coarse stage for P pairs, keeping the k best candidates of each.  Owns the resident buffers of one chunk of candidates
    (image, depth, bbox, the score workspace, the rasteriser's reserve) and the per-candidate arrays (poses, score, status).
    evaluator: a lib.dataset.evaluation.PoseEvaluator whose model points the box fit projects (device_tables), or None: the vertices
    of the render machine's meshes."""

    def __init__(self, config, render_machine, evaluator, P, k):
        cfg = config
        views, inplane, self.iters, self.z_init, self.score_mode, self.tau, chunk = coarse_settings(cfg)
        if views < 1:
            raise ValueError("CoarseInit needs TEST.COARSE_VIEWS > 0")
        if hasattr(render_machine, "normals"):
            raise ValueError("TEST.COARSE_VIEWS > 0 is not supported with the lit ModelNet renderer")
        self.P, self.M, self.k = int(P), views * inplane, int(k)
        if not 1 <= self.k <= min(self.M, ops.HYP_TOPK_MAX):
            raise ValueError("the coarse stage keeps k = {} poses per pair (TEST.HYP_NUM): must be 1 .. min(COARSE_VIEWS x COARSE_INPLANE "
                             "= {}, {})".format(self.k, self.M, ops.HYP_TOPK_MAX))
        self.render_machine = rm = render_machine
        d = rm.device
        H, W = rm.height, rm.width   # the frame is the render machine's
        B = self.B = self.P * self.M
        self.chunk = C = min(chunk, B)
        self.K = np.asarray(cfg.dataset.INTRINSIC_MATRIX, dtype=np.float64).reshape(3, 3)
        self.plane_means = np.asarray(cfg.network.PIXEL_MEANS, dtype=np.float32).reshape(3)[::-1].copy()
        tables = evaluator.device_tables(d) if evaluator is not None else mesh_point_tables(rm)
        self.points, self.table_off = tables[0], tables[1]
        self.rotations = coarse_rotations(views, inplane)
        self.rot_table = torch.from_numpy(self.rotations.astype(np.float32).reshape(self.M, 9)).to(d)
        self.obs_row = (torch.arange(B, dtype=torch.int32, device=d) // self.M).to(torch.int32).contiguous()   # b // M
        self.cls_s = torch.zeros((B,), dtype=torch.int32, device=d)
        self.K_s = torch.zeros((B, 9), dtype=torch.float32, device=d)
        self.poses_all = torch.zeros((B, 3, 4), dtype=torch.float32, device=d)
        self.score_all = torch.zeros((B,), dtype=torch.float32, device=d)
        self.status_all = torch.zeros((B,), dtype=torch.int32, device=d)
        self.image = torch.zeros((C, 3, H, W), dtype=torch.float32, device=d)
        self.depth = torch.zeros((C, 1, H, W), dtype=torch.float32, device=d)
        self.bbox = torch.zeros((C, 4), dtype=torch.int32, device=d)
        self.score_work = ops.pose_score_workspace(C, H, W, d)
        self.poses = torch.zeros((self.P, self.k, 3, 4), dtype=torch.float32, device=d)
        self.idx = torch.zeros((self.P, self.k), dtype=torch.int32, device=d)
        self.score = torch.zeros((self.P, self.k), dtype=torch.float32, device=d)
        self.status = torch.zeros((self.P, self.k), dtype=torch.int32, device=d)
        # a candidate with one of these bits is no candidate: the box fit's, the render's and the score's
        self.reject_mask = (ops.STATUS_COARSE_BAD_BOX | ops.STATUS_BAD_CLASS | ops.STATUS_BAD_FACE | ops.STATUS_BAD_K
                            | ops.STATUS_HYP_NO_SCORE)
        for n in {C, B % C} - {0}:   # the rasteriser's workspace of a full chunk and of the short last one
            rm.reserve(n)

    def chunks(self):
        """the contiguous sample ranges [a, e) one render + score covers; a range may cross pair boundaries"""
        return [(a, min(a + self.chunk, self.B)) for a in range(0, self.B, self.chunk)]

    def fit(self, boxes, class_index, K=None):
        """the candidates of every pair: poses_all (P*M,3,4), status_all reset to the fit's bits; class and K of every sample"""
        ops.fill(self.status_all, 0)
        ops.pose_from_box(self.points, self.table_off, class_index, self.rot_table, boxes, self.K, self.iters, self.z_init,
                          K_per_sample=K, pose_out=self.poses_all, status=self.status_all)
        ops.hyp_broadcast(self.cls_s, class_index, self.M)
        if K is not None:
            ops.hyp_broadcast(self.K_s, K, self.M)

    def render(self, a, e, per_pair_K):
        n = e - a
        self.render_machine.render_batch(self.cls_s[a:e], self.poses_all[a:e], K=self.K_s[a:e] if per_pair_K else None, image=self.image[:n],
                                         depth=self.depth[:n], bbox=self.bbox[:n], plane_means=self.plane_means, mask_thr=0.0,
                                         status=self.status_all[a:e])

    def score_chunk(self, a, e, image_observed, depth_observed):
        n = e - a
        ops.pose_score(image_observed, self.image[:n], self.depth[:n], self.score_mode, self.tau,
                       depth_observed=depth_observed if self.score_mode == "depth" else None, bbox=self.bbox[:n],
                       score=self.score_all[a:e], status=self.status_all[a:e], workspace=self.score_work, obs_row=self.obs_row[a:e])

    def topk(self):
        ops.hyp_topk(self.score_all, self.M, self.k, self.poses_all, status_in=self.status_all, reject_mask=self.reject_mask,
                     idx_out=self.idx, score_out=self.score, poses_out=self.poses, status_out=self.status)

    def run(self, image_observed, boxes, class_index, depth_observed=None, K=None):
        """image_observed (P,3,H,W) as the network reads it (plane means subtracted), boxes (P,4) {x0,x1,y0,y1} continuous pixel
        extents, class_index (P,), depth_observed (P,1,H,W) for COARSE_SCORE 'depth', K None or the camera of each pair ((P,3,3) /
        (P,9)); any device.  -> (poses (P,k,3,4), idx (P,k) int32: the m of each kept candidate, score (P,k), status (P,k) int32),
        resident on the device and overwritten by the next run; poses_all / score_all / status_all hold all P*M candidates."""
        d, P = self.render_machine.device, self.P
        H, W = self.render_machine.height, self.render_machine.width
        image_observed = torch.as_tensor(image_observed).to(d, torch.float32).contiguous()
        if tuple(image_observed.shape) != (P, 3, H, W):
            raise ValueError("coarse: image_observed must be ({},3,{},{}), got {}".format(P, H, W, tuple(image_observed.shape)))
        boxes = torch.as_tensor(boxes).to(d, torch.float32).contiguous()
        if tuple(boxes.shape) != (P, 4):
            raise ValueError("coarse: det_boxes must be ({},4) = {{x0, x1, y0, y1}} per pair, got {}".format(P, tuple(boxes.shape)))
        class_index = torch.as_tensor(class_index).to(d, torch.int32).contiguous()
        if self.score_mode == "depth":
            if depth_observed is None:
                raise ValueError("TEST.COARSE_SCORE 'depth': the coarse score needs depth_observed")
            depth_observed = torch.as_tensor(depth_observed).to(d, torch.float32).contiguous()
        if K is not None:
            K = torch.as_tensor(K).to(d, torch.float32).reshape(-1, 9).contiguous()
            if K.shape[0] != P:
                raise ValueError("coarse: per-pair K must be ({0},3,3) or ({0},9)".format(P))
        self.fit(boxes, class_index, K)
        for a, e in self.chunks():
            self.render(a, e, K is not None)
            self.score_chunk(a, e, image_observed, depth_observed)
        self.topk()
        return self.poses, self.idx, self.score, self.status
