"""Thin torch-tensor front-ends of the C ABI (one function per entry point of include/deepim_hip.h).

Every function only enqueues HIP kernels on torch's current stream; outputs are written into
caller-provided tensors when given, so the refinement loop can run allocation-free inside a
hipGraph capture.  No CPU fallback: non-CUDA tensors raise DeepIMHipError.
"""
import struct

import numpy as np

import torch

from . import capi
from .capi import check, current_stream, dptr, host_f32, lib

f32 = torch.float32
i32 = torch.int32
bf16 = torch.bfloat16


def to_bf16(src, out=None):
    """element-wise f32 -> bf16 (round to nearest even) as a kernel launch: the packed weight arrays of the bf16 convolution
    entry points, the flat gradient bucket"""
    out = out if out is not None else torch.empty(src.shape, dtype=bf16, device=src.device)
    check(lib().dim_f32_to_bf16(dptr(src, f32), dptr(out, bf16), src.numel(), current_stream()))
    return out


def from_bf16(src, out=None):
    out = out if out is not None else torch.empty(src.shape, dtype=f32, device=src.device)
    check(lib().dim_bf16_to_f32(dptr(src, bf16), dptr(out, f32), src.numel(), current_stream()))
    return out


def _wp(w):
    """(device pointer, is_bf16) of a packed weight array: bf16 arrays select the bf16 matrix-pipe twin of the entry point"""
    if w.dtype == bf16:
        return dptr(w, bf16), True
    return dptr(w, f32), False


def _new(shape, like, dtype=f32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def mask_bbox(x, thr, mode=0, means3=None, out=None):
    """bbox (B,4) int32 = {min_x,max_x,min_y,max_y} of the predicate; empty = {W,-1,H,-1}."""
    B, C, H, W = x.shape
    out = out if out is not None else _new((B, 4), x, i32)
    keep, mp = host_f32(means3, 3) if means3 is not None else (None, None)
    check(lib().dim_mask_bbox(dptr(x, f32), B, C, H, W, mode, float(thr), mp, dptr(out, i32), current_stream()))
    return out


def zoom_factor(bbox_obs, bbox_ren, src_pose, K, H, W, out=None, status=None):
    B = src_pose.shape[0]
    out = out if out is not None else _new((B, 4), src_pose)
    keep, kp = host_f32(K, 9)
    check(lib().dim_zoom_factor(dptr(bbox_obs, i32), dptr(bbox_ren, i32), dptr(src_pose, f32), kp, B, H, W, dptr(out, f32),
                                dptr(status, i32), current_stream()))
    return out


def zoom_planes(x, zf, inverse=False, pre=0, post=0, add3=None, scale_mode=0, out=None):
    B, C, H, W = x.shape
    out = out if out is not None else torch.empty_like(x)
    keep, ap = host_f32(add3, 3) if add3 is not None else (None, None)
    check(lib().dim_zoom_planes(dptr(x, f32), dptr(zf, f32), dptr(out, f32), B, C, H, W, int(inverse), pre, post, ap, scale_mode,
                                current_stream()))
    return out


def zoom_net_input(img_obs, img_ren, mask_obs, mask_ren, zf, plane_means3, X=None, nchw_out=None):
    """X (B,H,W,8) NHWC network input.  nchw_out: optional (z_img_obs, z_img_ren, z_mask_obs, z_mask_ren)."""
    B, _, H, W = img_obs.shape
    X = X if X is not None else _new((B, H, W, 8), img_obs)
    keep, mp = host_f32(plane_means3, 3)
    z = nchw_out if nchw_out is not None else (None, None, None, None)
    check(lib().dim_zoom_net_input(dptr(img_obs, f32), dptr(img_ren, f32), dptr(mask_obs, f32), dptr(mask_ren, f32), dptr(zf, f32),
                                   dptr(X, f32), B, H, W, mp, dptr(z[0], f32), dptr(z[1], f32), dptr(z[2], f32), dptr(z[3], f32),
                                   current_stream()))
    return X


def zoom_net_input_ex(img_obs, img_ren, extra_obs, extra_ren, zf, plane_means3, mode, X=None):
    """the other input arities of the first layer: mode 1 = images only, mode 2 = depth planes in place of the masks (see the header)"""
    B, _, H, W = img_obs.shape
    X = X if X is not None else _new((B, H, W, 8), img_obs)
    keep, mp = host_f32(plane_means3, 3)
    check(lib().dim_zoom_net_input_ex(dptr(img_obs, f32), dptr(img_ren, f32), dptr(extra_obs, f32), dptr(extra_ren, f32), dptr(zf, f32),
                                      dptr(X, f32), B, H, W, mp, int(mode), current_stream()))
    return X


def _net_size(out, net_size, what):
    """the network size (Hn, Wn) of a `_src` sampler: the explicit argument, else the output tensor's (`what` = its rows, cols axes)"""
    if net_size is None:
        if out is None:
            raise ValueError("pass the output tensor or net_size=(Hn, Wn)")
        return int(out.shape[what[0]]), int(out.shape[what[1]])
    return int(net_size[0]), int(net_size[1])


def _same_shape(t, shape, name):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("{} must have shape {}, got {}".format(name, tuple(shape), tuple(t.shape)))


def _zoom_planes_two_sizes(entry, tail, x, zf, pre, post, add3, out, net_size):
    B, C, Hs, Ws = x.shape
    Hn, Wn = _net_size(out, net_size, (2, 3))
    out = out if out is not None else _new((B, C, Hn, Wn), x)
    _same_shape(out, (B, C, Hn, Wn), "out")
    _same_shape(zf, (B, 4), "zoom_factor")
    keep, ap = host_f32(add3, 3) if add3 is not None else (None, None)
    check(entry(dptr(x, f32), dptr(zf, f32), dptr(out, f32), B, C, Hs, Ws, Hn, Wn, pre, post, ap, *tail, current_stream()))
    return out


def _zoom_net_input_two_sizes(entry, tail, img_obs, img_ren, extra_obs, extra_ren, zf, plane_means3, mode, X, nchw_out, net_size):
    B, _, Hs, Ws = img_obs.shape
    Hn, Wn = _net_size(X, net_size, (1, 2))
    X = X if X is not None else _new((B, Hn, Wn, 8), img_obs)
    _same_shape(X, (B, Hn, Wn, 8), "X")
    _same_shape(zf, (B, 4), "zoom_factor")
    _same_shape(img_obs, (B, 3, Hs, Ws), "image_observed")
    _same_shape(img_ren, (B, 3, Hs, Ws), "image_rendered")
    _same_shape(extra_obs, (B, 1, Hs, Ws), "the observed extra plane")
    _same_shape(extra_ren, (B, 1, Hs, Ws), "the rendered extra plane")
    z = nchw_out if nchw_out is not None else (None, None, None, None)
    for t, c in zip(z, (3, 3, 1, 1)):
        _same_shape(t, (B, c, Hn, Wn), "an NCHW output")
    keep, mp = host_f32(plane_means3, 3)
    check(entry(dptr(img_obs, f32), dptr(img_ren, f32), dptr(extra_obs, f32), dptr(extra_ren, f32), dptr(zf, f32), dptr(X, f32), B, Hs, Ws,
                Hn, Wn, mp, int(mode), dptr(z[0], f32), dptr(z[1], f32), dptr(z[2], f32), dptr(z[3], f32), *tail, current_stream()))
    return X


def zoom_planes_src(x, zf, pre=0, post=0, add3=None, out=None, net_size=None):
    """dim_zoom_planes_src: x (B,C,Hs,Ws) sampled into out (B,C,Hn,Wn), forward direction only.  The source size is x's; the network
    size out's, or net_size=(Hn, Wn) when out is allocated here."""
    return _zoom_planes_two_sizes(lib().dim_zoom_planes_src, (), x, zf, pre, post, add3, out, net_size)


def zoom_net_input_src(img_obs, img_ren, extra_obs, extra_ren, zf, plane_means3, mode=0, X=None, nchw_out=None, net_size=None):
    """dim_zoom_net_input_src: the blobs (B,.,Hs,Ws) sampled into X (B,Hn,Wn,8), modes as zoom_net_input_ex.  The source size is the
    blobs'; the network size X's, or net_size=(Hn, Wn) when X is allocated here.  nchw_out (mode 0): the four (B,.,Hn,Wn) op outputs."""
    return _zoom_net_input_two_sizes(lib().dim_zoom_net_input_src, (), img_obs, img_ren, extra_obs, extra_ren, zf, plane_means3, mode, X,
                                     nchw_out, net_size)


def zoom_planes_area(x, zf, pre=0, post=0, add3=None, out=None, net_size=None, max_taps=4):
    """dim_zoom_planes_area: zoom_planes_src with the area filter -- every output the mean of its n_y x n_x bilinear sub-samples, the
    counts per pair and axis from the window's size (zoom_area_taps), at most max_taps (1..8) per axis"""
    return _zoom_planes_two_sizes(lib().dim_zoom_planes_area, (int(max_taps),), x, zf, pre, post, add3, out, net_size)


def zoom_net_input_area(img_obs, img_ren, extra_obs, extra_ren, zf, plane_means3, mode=0, X=None, nchw_out=None, net_size=None,
                        max_taps=4):
    """dim_zoom_net_input_area: zoom_net_input_src (same arguments, same lanes) with the area filter of zoom_planes_area"""
    return _zoom_net_input_two_sizes(lib().dim_zoom_net_input_area, (int(max_taps),), img_obs, img_ren, extra_obs, extra_ren, zf,
                                     plane_means3, mode, X, nchw_out, net_size)


def zoom_area_taps(zf, src_size, net_size, max_taps=4, out=None):
    """dim_zoom_area_taps: (B,2) int32 (n_x, n_y), the sub-samples per axis the area samplers take for every pair's window"""
    B = zf.shape[0]
    _same_shape(zf, (B, 4), "zoom_factor")
    out = out if out is not None else _new((B, 2), zf, i32)
    _same_shape(out, (B, 2), "out")
    check(lib().dim_zoom_area_taps(dptr(zf, f32), B, int(src_size[0]), int(src_size[1]), int(net_size[0]), int(net_size[1]), int(max_taps),
                                   dptr(out, i32), current_stream()))
    return out


def zoom_trans(zf, t, mode, out=None):
    B = t.shape[0]
    out = out if out is not None else torch.empty_like(t)
    check(lib().dim_zoom_trans(dptr(zf, f32), dptr(t, f32), dptr(out, f32), B, mode, current_stream()))
    return out


def se3_compose(pose_src, se3, rot_coord, T_means, T_stds, out=None, out_f64=None):
    B = pose_src.shape[0]
    out = out if out is not None else torch.empty_like(pose_src)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_se3_compose(dptr(pose_src, f32), dptr(se3, f32), dptr(out, f32), dptr(out_f64, torch.float64), B,
                                capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return out


def se3_delta(pose_src, pose_tgt, rot_coord, T_means, T_stds):
    B = pose_src.shape[0]
    rot = _new((B, 4), pose_src)
    trans = _new((B, 3), pose_src)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_se3_delta(dptr(pose_src, f32), dptr(pose_tgt, f32), dptr(rot, f32), dptr(trans, f32), B,
                              capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return rot, trans


def se3_delta_matrix(pose_src, pose_tgt, rot_coord, T_means, T_stds):
    """-> (rotation residual (B,3,3), translation residual (B,3)): calc_RT_delta(..., rot_type="MATRIX")"""
    B = pose_src.shape[0]
    rot = _new((B, 3, 3), pose_src)
    trans = _new((B, 3), pose_src)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_se3_delta_matrix(dptr(pose_src, f32), dptr(pose_tgt, f32), dptr(rot, f32), dptr(trans, f32), B,
                                     capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return rot, trans


def se3_compose_euler(pose_src, euler_trans6, rot_coord, T_means, T_stds, out=None, out_f64=None):
    """RT_transform with a 3-number EULER rotation delta: euler_trans6 (B,6) = [ai, aj, ak, t]"""
    B = pose_src.shape[0]
    out = out if out is not None else torch.empty_like(pose_src)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_se3_compose_euler(dptr(pose_src, f32), dptr(euler_trans6, f32), dptr(out, f32), dptr(out_f64, torch.float64), B,
                                      capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return out


def se3_delta_euler(pose_src, pose_tgt, rot_coord, T_means, T_stds):
    """-> (static-xyz Euler angles (B,3), translation residual (B,3)): calc_RT_delta(..., rot_type="EULER")"""
    B = pose_src.shape[0]
    rot = _new((B, 3), pose_src)
    trans = _new((B, 3), pose_src)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_se3_delta_euler(dptr(pose_src, f32), dptr(pose_tgt, f32), dptr(rot, f32), dptr(trans, f32), B,
                                    capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return rot, trans


def transform3d_fwd(points, rot, trans, pose_src, rot_coord, T_means, T_stds, out=None):
    B = points.shape[0]
    npts = points.numel() // (B * 3) if B else 0
    out = out if out is not None else torch.empty_like(points)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_transform3d_fwd(dptr(points, f32), dptr(rot, f32), dptr(trans, f32), dptr(pose_src, f32), dptr(out, f32), B, npts,
                                    capi.rot_coord_id(rot_coord), mp, sp, current_stream()))
    return out


def transform3d_bwd(out_grad, points, rot, trans, pose_src, rot_coord, T_means, T_stds):
    B = points.shape[0]
    npts = points.numel() // (B * 3) if B else 0
    d_rot = torch.empty_like(rot)
    d_trans = torch.empty_like(trans)
    k1, mp = host_f32(T_means, 3)
    k2, sp = host_f32(T_stds, 3)
    check(lib().dim_transform3d_bwd(dptr(out_grad, f32), dptr(points, f32), dptr(rot, f32), dptr(trans, f32), dptr(pose_src, f32),
                                    dptr(d_rot, f32), dptr(d_trans, f32), B, npts, capi.rot_coord_id(rot_coord), mp, sp,
                                    current_stream()))
    return d_rot, d_trans


def depth_to_flow(depth_src, depth_tgt, KT, Kinv, flow=None, valid=None):
    B, _, H, W = depth_src.shape
    flow = flow if flow is not None else _new((B, 2, H, W), depth_src)
    valid = valid if valid is not None else _new((B, 1, H, W), depth_src)
    keep, kp = host_f32(Kinv, 9)
    check(lib().dim_depth_to_flow(dptr(depth_src, f32), dptr(depth_tgt, f32), dptr(KT, f32), kp, B, H, W, dptr(flow, f32),
                                  dptr(valid, f32), current_stream()))
    return flow, valid


def flow_epe_sums(flow_pred, flow_gt, visible, depth_rendered, sums=None, accumulate=False, workspace=None):
    """per-sample sums of calc_EPE_one_pair (reference deepim/core/tester.py:719-736): sums (B,5) float64 =
    [epe_all, epe_viz, epe_vizbg, num_viz, num_vizbg]; flow_pred is rounded to float16 first as tester.py:485-487 stores it"""
    B, _, H, W = flow_pred.shape
    assert flow_gt.shape == flow_pred.shape and visible.shape == (B, 1, H, W) and depth_rendered.shape == (B, 1, H, W)
    if sums is None:
        assert not accumulate
        sums = torch.empty((B, 5), dtype=torch.float64, device=flow_pred.device)
    if workspace is None:
        workspace = torch.empty((lib().dim_flow_epe_workspace_bytes(B) // 8,), dtype=torch.float64, device=flow_pred.device)
    check(lib().dim_flow_epe_sums(dptr(flow_pred, f32), dptr(flow_gt, f32), dptr(visible, f32), dptr(depth_rendered, f32), B, H, W,
                                  dptr(workspace, torch.float64), dptr(sums, torch.float64), int(bool(accumulate)), current_stream()))
    return sums


def _opt(t, dt=f32):
    """device pointer of an optional tensor (None -> a null pointer)"""
    return dptr(t, dt) if t is not None else None


def _host_k9_f64(K):
    """the host 3x3 K -> nine contiguous float64 (the caller keeps the array alive through the call)"""
    keep = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(-1))
    if keep.size != 9:
        raise ValueError("expected a 3x3 K, got {} numbers".format(keep.size))
    return keep


def _kps_f64(K_per_sample, B, dev, who):
    """K_per_sample ((B,3,3) / (B,9), host array or CUDA tensor) -> None or a contiguous (B,9) float64 tensor on dev"""
    if K_per_sample is None:
        return None
    kps = torch.as_tensor(K_per_sample).to(dev, torch.float64).reshape(-1, 9).contiguous()
    if kps.shape[0] != B:
        raise ValueError("{2} K_per_sample must be ({0},3,3) or ({0},9), got {1}".format(B, tuple(torch.as_tensor(K_per_sample).shape), who))
    return kps


def _workspace_f64(nbytes, device):
    """a float64 tensor of at least nbytes (never empty: its pointer is passed as the workspace)"""
    return torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=device)


def _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace, nbytes):
    """what the wrappers of the four Gauss-Newton stages share -> (pose_out, keep, ptr): pose_out and a workspace of the stage's nbytes
    made when not given; keep: what has to outlive the call; ptr: the shared C arguments by name (None = a null pointer)"""
    B = pose_in.shape[0]
    pose_out = pose_out if pose_out is not None else _new((B, 3, 4), pose_in)
    workspace = workspace if workspace is not None else _workspace_f64(nbytes, pose_in.device)
    assert workspace.numel() * workspace.element_size() >= nbytes
    kps = intrinsics_per_sample(K_per_sample, B, pose_in.device)
    keep, kp = host_f32(K, 9)
    return pose_out, (keep, kps, workspace), dict(pose_in=dptr(pose_in, f32), K9=kp, kps=_opt(kps), bbox=_opt(bbox, i32),
                                                  workspace=dptr(workspace, torch.float64), pose_out=dptr(pose_out, f32),
                                                  stats=_opt(stats), status=_opt(status, i32))


STATUS_ICP_FEW_POINTS = 32   # DIM_STATUS_ICP_FEW_POINTS: an ICP iteration found < 64 inliers or a singular system (no update)


def icp_workspace(B, H, W, device):
    return _workspace_f64(lib().dim_icp_workspace_bytes(B, H, W), device)


def icp_refine(depth_rendered, depth_observed, pose_in, K, iters, max_dist, mask_observed=None, bbox=None, K_per_sample=None,
               pose_out=None, stats=None, status=None, workspace=None):
    """projective point-to-plane ICP of dim_icp_refine (restated by tests/icp_reference.py): depth_rendered (B,1,H,W) rendered at
    pose_in (B,3,4), depth_observed (B,1,H,W) metres; K: the host 3x3 used for every pair unless K_per_sample ((B,3,3) / (B,9),
    as render_batch takes it) is given; bbox (B,4) int32 of the render (None = whole frame).  -> pose_out (B,3,4);
    stats (B,iters,2) = (inliers, rms residual) per iteration, status (B,) int32: DIM_STATUS_ICP_FEW_POINTS is OR-ed in."""
    B, _, H, W = depth_rendered.shape
    assert depth_observed.shape == depth_rendered.shape and tuple(pose_in.shape) == (B, 3, 4)
    assert mask_observed is None or mask_observed.shape == depth_rendered.shape
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace, lib().dim_icp_workspace_bytes(B, H, W))
    check(lib().dim_icp_refine(dptr(depth_rendered, f32), dptr(depth_observed, f32), _opt(mask_observed), p["bbox"], p["pose_in"], p["K9"],
                               p["kps"], B, H, W, int(iters), float(max_dist), p["workspace"], p["pose_out"], p["stats"], p["status"],
                               current_stream()))
    return pose_out


STATUS_FLOW_PNP_FEW_POINTS = 128   # DIM_STATUS_FLOW_PNP_FEW_POINTS: a flow-PnP iteration had < 64 weighted points or a singular system


def flow_pnp_workspace(B, H, W, device):
    return _workspace_f64(lib().dim_flow_pnp_workspace_bytes(B, H, W), device)


def flow_pnp(depth_rendered, flow, pose_src, K, iters, warm=2, huber_px=2.0, max_px=8.0, standard_rep=False, valid=None, bbox=None,
             K_per_sample=None, pose_out=None, se3_q=None, stats=None, status=None, workspace=None):
    """pose from flow, dim_flow_pnp (restated by tests/flow_pnp_reference.py; the reference's flow2se3): depth_rendered (B,1,H,W)
    rendered at pose_src (B,3,4), flow (B,2,H,W) from the rendered image to the observed one in full-image pixels ((dy,dx) unless
    standard_rep), valid (B,1,H,W) read at the source pixel (None = every pixel), bbox (B,4) int32 of the render (None = whole frame);
    K / K_per_sample as icp_refine.  -> (pose_out (B,3,4), se3_q (B,7) = [quat, t] of the estimated transform); stats (B,iters,2) =
    (weighted points, rms pixel residual) per iteration, status (B,) int32: DIM_STATUS_FLOW_PNP_FEW_POINTS is OR-ed in."""
    B, _, H, W = depth_rendered.shape
    assert tuple(flow.shape) == (B, 2, H, W) and tuple(pose_src.shape) == (B, 3, 4)
    assert valid is None or valid.shape == depth_rendered.shape
    se3_q = se3_q if se3_q is not None else _new((B, 7), pose_src)
    pose_out, keep, p = _gn_tail(pose_src, K, K_per_sample, bbox, pose_out, stats, status, workspace, lib().dim_flow_pnp_workspace_bytes(B, H, W))
    check(lib().dim_flow_pnp(dptr(depth_rendered, f32), dptr(flow, f32), _opt(valid), p["bbox"], p["pose_in"], p["K9"], p["kps"], B, H, W,
                             int(bool(standard_rep)), int(iters), int(warm), float(huber_px), float(max_px), p["workspace"], p["pose_out"],
                             dptr(se3_q, f32), p["stats"], p["status"], current_stream()))
    return pose_out, se3_q


STATUS_PHOTO_FEW_POINTS = 1024   # DIM_STATUS_PHOTO_FEW_POINTS: a photometric iteration had < 64 weighted points, a singular system or no template
PHOTO_PLANES = ("obs", "ren", "depth", "valid")   # the plane kinds of dim_photo_workspace_offset, in its order


def photo_workspace(B, H, W, levels, device):
    nbytes = lib().dim_photo_workspace_bytes(B, H, W, int(levels))
    if nbytes <= 0:
        raise ValueError("photo_workspace: B = {}, a {}x{} frame and {} levels are refused (levels 1..5, coarsest level >= 3x3)".format(
            B, H, W, levels))
    return _workspace_f64(nbytes, device)


def photo_workspace_views(workspace, B, H, W, levels):
    """what dim_photo_refine left in its workspace, for tests and diagnostics (views, no copy) -> ({kind: [(B,H_l,W_l) f32 per level]}
    for the kinds of PHOTO_PLANES, (B,8) f64 = {n, sum Ir, sum Ir^2, sum Io, sum Io^2, a, b, may step})"""
    off = lambda plane, level: lib().dim_photo_workspace_offset(B, H, W, int(levels), plane, level)  # noqa: E731
    as_f32 = workspace.view(f32)
    planes, h, w = {k: [] for k in PHOTO_PLANES}, H, W
    for lv in range(levels):
        for p, kind in enumerate(PHOTO_PLANES):
            at = off(p, lv) // 4
            planes[kind].append(as_f32[at:at + B * h * w].view(B, h, w))
        h, w = h // 2, w // 2
    at = off(len(PHOTO_PLANES), 0) // 8
    return planes, workspace[at:at + 8 * B].view(B, 8)


def photo_refine(image_observed, image_rendered, depth_rendered, pose_in, K, levels, iters, huber, gate, gain=True, bbox=None,
                 K_per_sample=None, pose_out=None, stats=None, status=None, workspace=None):
    """photometric pose polish of dim_photo_refine (restated by tests/photo_reference.py): image_observed / image_rendered (B,3,H,W)
    mean-subtracted blobs, depth_rendered (B,1,H,W) rendered at pose_in (B,3,4); `levels` pyramid levels, `iters` Gauss-Newton
    iterations per level, huber and gate in units of the channel sum, one gain and bias per pair unless gain is False; K / K_per_sample
    / bbox as icp_refine.  -> pose_out (B,3,4); stats (B,levels*iters,2) = (weighted points, rms residual) per iteration, coarsest
    level first; status (B,) int32: DIM_STATUS_PHOTO_FEW_POINTS is OR-ed in."""
    B, _, H, W = depth_rendered.shape
    assert tuple(image_observed.shape) == (B, 3, H, W) and tuple(image_rendered.shape) == (B, 3, H, W)
    assert tuple(depth_rendered.shape) == (B, 1, H, W) and tuple(pose_in.shape) == (B, 3, 4)
    assert stats is None or stats.numel() >= 2 * B * int(levels) * int(iters)
    assert (status is None or status.numel() == B) and (bbox is None or bbox.numel() == 4 * B)
    if workspace is None:   # (refuses a shape the pyramid cannot hold)
        workspace = photo_workspace(B, H, W, levels, pose_in.device)
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace, lib().dim_photo_workspace_bytes(B, H, W, int(levels)))
    check(lib().dim_photo_refine(dptr(image_observed, f32), dptr(image_rendered, f32), dptr(depth_rendered, f32), p["bbox"], p["pose_in"],
                                 p["K9"], p["kps"], B, H, W, int(levels), int(iters), float(huber), float(gate), int(bool(gain)),
                                 p["workspace"], p["pose_out"], p["stats"], p["status"], current_stream()))
    return pose_out


STATUS_SIL_FEW_POINTS = 2048   # DIM_STATUS_SIL_FEW_POINTS: a silhouette iteration had < 64 weighted contour points or a singular system


def sil_edge_field(mask, radius, field=None):
    """nearest-edge field of dim_sil_edge_field (restated by tests/sil_reference.py): mask (B,1,H,W) f32, foreground where >= 0.5
    -> field (B,H,W) int32 = (ey << 16) | ex of the nearest edge pixel within `radius` (1..64) pixels, -1 where there is none"""
    B, C, H, W = mask.shape
    assert C == 1
    field = field if field is not None else _new((B, H, W), mask, i32)
    assert tuple(field.shape) == (B, H, W)
    check(lib().dim_sil_edge_field(dptr(mask, f32), B, H, W, int(radius), dptr(field, i32), current_stream()))
    return field


def sil_workspace(B, H, W, device):
    return _workspace_f64(lib().dim_sil_workspace_bytes(B, H, W), device)


def sil_refine(depth_rendered, field, pose_in, K, iters, huber_px, max_px, bbox=None, K_per_sample=None, pose_out=None, stats=None,
               status=None, workspace=None):
    """silhouette pose polish of dim_sil_refine (restated by tests/sil_reference.py): the contour pixels of depth_rendered (B,1,H,W),
    rendered at pose_in (B,3,4), are pulled onto the edge pixels of field (B,H,W) int32 (sil_edge_field) by `iters` Gauss-Newton
    iterations, Huber knee and hard gate in pixels; K / K_per_sample / bbox as flow_pnp.  -> pose_out (B,3,4); stats (B,iters,2) =
    (weighted points, rms pixel distance) per iteration; status (B,) int32: DIM_STATUS_SIL_FEW_POINTS is OR-ed in."""
    B, _, H, W = depth_rendered.shape
    assert tuple(depth_rendered.shape) == (B, 1, H, W) and tuple(field.shape) == (B, H, W) and tuple(pose_in.shape) == (B, 3, 4)
    assert stats is None or stats.numel() >= 2 * B * int(iters)
    assert (status is None or status.numel() == B) and (bbox is None or bbox.numel() == 4 * B)
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace, lib().dim_sil_workspace_bytes(B, H, W))
    check(lib().dim_sil_refine(dptr(depth_rendered, f32), dptr(field, i32), p["bbox"], p["pose_in"], p["K9"], p["kps"], B, H, W, int(iters),
                               float(huber_px), float(max_px), p["workspace"], p["pose_out"], p["stats"], p["status"], current_stream()))
    return pose_out


STATUS_VIEWS_NO_CONSENSUS = 32768   # DIM_STATUS_VIEWS_NO_CONSENSUS: dim_views_consensus found no eligible view in the sample's group
VIEWS_MAX = 16                      # views per group (kGnMaxViews)


def _views_shapes(cam_T_rig, B, V, who):
    V = int(V)
    if not 1 <= V <= VIEWS_MAX or B % V:
        raise ValueError("{}: V = {} must be in 1..{} and divide B = {}".format(who, V, VIEWS_MAX, B))
    assert tuple(cam_T_rig.shape) == (B, 3, 4), "{}: cam_T_rig must be ({},3,4), got {}".format(who, B, tuple(cam_T_rig.shape))
    return B // V, V


def views_from_rig(pose_rig, cam_T_rig, V, pose_views=None):
    """dim_views_from_rig (restated by tests/views_reference.py): pose_rig (G,3,4), cam_T_rig (G*V,3,4) = X_b with p_cam = X_b p_rig,
    sample b = g*V + v -> pose_views (G*V,3,4) = X_b pose_rig[g]"""
    B = cam_T_rig.shape[0]
    G, V = _views_shapes(cam_T_rig, B, V, "views_from_rig")
    assert tuple(pose_rig.shape) == (G, 3, 4)
    pose_views = pose_views if pose_views is not None else _new((B, 3, 4), pose_rig)
    assert tuple(pose_views.shape) == (B, 3, 4)
    check(lib().dim_views_from_rig(dptr(pose_rig, f32), dptr(cam_T_rig, f32), G, V, dptr(pose_views, f32), current_stream()))
    return pose_views


def views_consensus(score, pose, cam_T_rig, V, status=None, fatal_mask=0, choice=None, pose_rig=None, pose_views=None, status_out=None):
    """dim_views_consensus: score (B,) f32 and pose (B,3,4) of every view, status (B,) int32 whose fatal_mask bits rule a view out
    -> (choice (G,) int32 = the best eligible view of each group or -1, pose_rig (G,3,4) from that view, pose_views (B,3,4) = every
    view's pose from pose_rig, the chosen view's own bit for bit); DIM_STATUS_VIEWS_NO_CONSENSUS is OR-ed into status_out (B,) int32"""
    B = pose.shape[0]
    G, V = _views_shapes(cam_T_rig, B, V, "views_consensus")
    assert tuple(pose.shape) == (B, 3, 4) and score.numel() == B
    assert (status is None or status.numel() == B) and (status_out is None or status_out.numel() == B)
    choice = choice if choice is not None else _new((G,), pose, i32)
    pose_rig = pose_rig if pose_rig is not None else _new((G, 3, 4), pose)
    pose_views = pose_views if pose_views is not None else _new((B, 3, 4), pose)
    assert choice.numel() == G and tuple(pose_rig.shape) == (G, 3, 4) and tuple(pose_views.shape) == (B, 3, 4)
    check(lib().dim_views_consensus(dptr(score, f32), _opt(status, i32), int(fatal_mask), dptr(pose, f32), dptr(cam_T_rig, f32), G, V,
                                    dptr(choice, i32), dptr(pose_rig, f32), dptr(pose_views, f32), _opt(status_out, i32), current_stream()))
    return choice, pose_rig, pose_views


def _views_tail(cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group, B, n_iters, who):
    """what the three joint stage wrappers share -> (pose_rig_out, the five trailing C arguments)"""
    G, V = _views_shapes(cam_T_rig, B, V, who)
    assert tuple(pose_rig_in.shape) == (G, 3, 4)
    pose_rig_out = pose_rig_out if pose_rig_out is not None else _new((G, 3, 4), pose_rig_in)
    assert tuple(pose_rig_out.shape) == (G, 3, 4) and (stats_group is None or stats_group.numel() >= 2 * G * n_iters)
    return pose_rig_out, (dptr(cam_T_rig, f32), V, dptr(pose_rig_in, f32), dptr(pose_rig_out, f32), _opt(stats_group))


def icp_views_workspace(B, H, W, V, device):
    return _workspace_f64(lib().dim_icp_views_workspace_bytes(B, H, W, int(V)), device)


def icp_refine_views(depth_rendered, depth_observed, pose_in, K, iters, max_dist, cam_T_rig, V, pose_rig_in, mask_observed=None, bbox=None,
                     K_per_sample=None, pose_out=None, pose_rig_out=None, stats=None, stats_group=None, status=None, workspace=None):
    """icp_refine with one correction per group of V calibrated views (dim_icp_refine_views, restated by tests/views_reference.py):
    cam_T_rig (B,3,4), pose_rig_in (G,3,4), B = G*V, sample b = g*V + v.  -> (pose_out (B,3,4), pose_rig_out (G,3,4));
    stats (B,iters,2) per sample as icp_refine, stats_group (G,iters,2) = (inliers, rms residual) of the group; the FEW_POINTS bit
    goes to all V samples of a group whose step was skipped."""
    B, _, H, W = depth_rendered.shape
    assert depth_observed.shape == depth_rendered.shape and tuple(pose_in.shape) == (B, 3, 4)
    assert mask_observed is None or mask_observed.shape == depth_rendered.shape
    pose_rig_out, tail = _views_tail(cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group, B, int(iters), "icp_refine_views")
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace,
                                 lib().dim_icp_views_workspace_bytes(B, H, W, int(V)))
    check(lib().dim_icp_refine_views(dptr(depth_rendered, f32), dptr(depth_observed, f32), _opt(mask_observed), p["bbox"], p["pose_in"],
                                     p["K9"], p["kps"], B, H, W, int(iters), float(max_dist), p["workspace"], p["pose_out"], p["stats"],
                                     p["status"], *tail, current_stream()))
    return pose_out, pose_rig_out


STATUS_VIEWS_CALIB_HELD = 65536   # DIM_STATUS_VIEWS_CALIB_HELD: dim_icp_refine_rig held the sample's camera in an iteration


def icp_rig_workspace(B, H, W, V, device):
    return _workspace_f64(lib().dim_icp_rig_workspace_bytes(B, H, W, int(V)), device)


def icp_refine_rig(depth_rendered, depth_observed, pose_in, K, iters, max_dist, cam_T_rig, V, pose_rig_in, mask_observed=None, bbox=None,
                   K_per_sample=None, pose_out=None, pose_rig_out=None, cam_T_rig_out=None, stats=None, stats_group=None, stats_view=None,
                   status=None, workspace=None):
    """icp_refine_views with the rig's extrinsics refined along (dim_icp_refine_rig, restated by tests/rig_reference.py): cam_T_rig
    (B,3,4) whose groups repeat the V rows of one rig (the caller's check; group 0 is read).  -> (pose_out (B,3,4), pose_rig_out
    (G,3,4), cam_T_rig_out (B,3,4) = the refined rig repeated G times, camera 0's row unchanged); stats, stats_group as
    icp_refine_views, stats_view (V,iters,2) per camera; DIM_STATUS_VIEWS_CALIB_HELD goes to the samples of a camera held in an
    iteration."""
    B, _, H, W = depth_rendered.shape
    assert depth_observed.shape == depth_rendered.shape and tuple(pose_in.shape) == (B, 3, 4)
    assert mask_observed is None or mask_observed.shape == depth_rendered.shape
    pose_rig_out, tail = _views_tail(cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group, B, int(iters), "icp_refine_rig")
    cam_T_rig_out = cam_T_rig_out if cam_T_rig_out is not None else _new((B, 3, 4), cam_T_rig)
    assert tuple(cam_T_rig_out.shape) == (B, 3, 4) and cam_T_rig_out.data_ptr() != cam_T_rig.data_ptr()
    assert stats_view is None or stats_view.numel() >= 2 * int(V) * int(iters)
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace,
                                 lib().dim_icp_rig_workspace_bytes(B, H, W, int(V)))
    check(lib().dim_icp_refine_rig(dptr(depth_rendered, f32), dptr(depth_observed, f32), _opt(mask_observed), p["bbox"], p["pose_in"],
                                   p["K9"], p["kps"], B, H, W, int(iters), float(max_dist), p["workspace"], p["pose_out"], p["stats"],
                                   p["status"], *tail, dptr(cam_T_rig_out, f32), _opt(stats_view), current_stream()))
    return pose_out, pose_rig_out, cam_T_rig_out


def photo_views_workspace(B, H, W, levels, V, device):
    nbytes = lib().dim_photo_views_workspace_bytes(B, H, W, int(levels), int(V))
    if nbytes <= 0:
        raise ValueError("photo_views_workspace: B = {}, a {}x{} frame, {} levels and V = {} are refused (levels 1..5, coarsest level "
                         ">= 3x3)".format(B, H, W, levels, V))
    return _workspace_f64(nbytes, device)


def photo_refine_views(image_observed, image_rendered, depth_rendered, pose_in, K, levels, iters, huber, gate, cam_T_rig, V, pose_rig_in,
                       gain=True, bbox=None, K_per_sample=None, pose_out=None, pose_rig_out=None, stats=None, stats_group=None, status=None,
                       workspace=None):
    """photo_refine with one correction per group of V calibrated views (dim_photo_refine_views); the views' arguments and results as
    icp_refine_views, stats_group (G,levels*iters,2)"""
    B, _, H, W = depth_rendered.shape
    assert tuple(image_observed.shape) == (B, 3, H, W) and tuple(image_rendered.shape) == (B, 3, H, W)
    assert tuple(depth_rendered.shape) == (B, 1, H, W) and tuple(pose_in.shape) == (B, 3, 4)
    assert stats is None or stats.numel() >= 2 * B * int(levels) * int(iters)
    assert (status is None or status.numel() == B) and (bbox is None or bbox.numel() == 4 * B)
    pose_rig_out, tail = _views_tail(cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group, B, int(levels) * int(iters), "photo_refine_views")
    if workspace is None:
        workspace = photo_views_workspace(B, H, W, levels, V, pose_in.device)
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace,
                                 lib().dim_photo_views_workspace_bytes(B, H, W, int(levels), int(V)))
    check(lib().dim_photo_refine_views(dptr(image_observed, f32), dptr(image_rendered, f32), dptr(depth_rendered, f32), p["bbox"],
                                       p["pose_in"], p["K9"], p["kps"], B, H, W, int(levels), int(iters), float(huber), float(gate),
                                       int(bool(gain)), p["workspace"], p["pose_out"], p["stats"], p["status"], *tail, current_stream()))
    return pose_out, pose_rig_out


def sil_views_workspace(B, H, W, V, device):
    return _workspace_f64(lib().dim_sil_views_workspace_bytes(B, H, W, int(V)), device)


def sil_refine_views(depth_rendered, field, pose_in, K, iters, huber_px, max_px, cam_T_rig, V, pose_rig_in, bbox=None, K_per_sample=None,
                     pose_out=None, pose_rig_out=None, stats=None, stats_group=None, status=None, workspace=None):
    """sil_refine with one correction per group of V calibrated views (dim_sil_refine_views); the views' arguments and results as
    icp_refine_views"""
    B, _, H, W = depth_rendered.shape
    assert tuple(depth_rendered.shape) == (B, 1, H, W) and tuple(field.shape) == (B, H, W) and tuple(pose_in.shape) == (B, 3, 4)
    assert stats is None or stats.numel() >= 2 * B * int(iters)
    assert (status is None or status.numel() == B) and (bbox is None or bbox.numel() == 4 * B)
    pose_rig_out, tail = _views_tail(cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group, B, int(iters), "sil_refine_views")
    pose_out, keep, p = _gn_tail(pose_in, K, K_per_sample, bbox, pose_out, stats, status, workspace,
                                 lib().dim_sil_views_workspace_bytes(B, H, W, int(V)))
    check(lib().dim_sil_refine_views(dptr(depth_rendered, f32), dptr(field, i32), p["bbox"], p["pose_in"], p["K9"], p["kps"], B, H, W,
                                     int(iters), float(huber_px), float(max_px), p["workspace"], p["pose_out"], p["stats"], p["status"],
                                     *tail, current_stream()))
    return pose_out, pose_rig_out


STATUS_HYP_NO_SCORE = 64  # DIM_STATUS_HYP_NO_SCORE: dim_pose_score had < 64 counted pixels, a constant plane or a non-finite sum
HYP_SCORE_ID = {"rgb": 0, "depth": 1}   # DIM_HYP_SCORE_RGB / DIM_HYP_SCORE_DEPTH


def hyp_expand(rot_table, pose_in, N, out=None):
    """dim_hyp_expand: rot_table (N,3,3) or (N,9) f32 CUDA, pose_in (P,3,4) -> (P*N,3,4), sample p*N+h = [R_h R_p | t_p], h = 0 the
    pair's pose bit for bit"""
    P = pose_in.shape[0]
    assert rot_table.numel() == 9 * N and tuple(pose_in.shape) == (P, 3, 4)
    out = out if out is not None else _new((P * N, 3, 4), pose_in)
    assert tuple(out.shape) == (P * N, 3, 4)
    check(lib().dim_hyp_expand(dptr(rot_table, f32), dptr(pose_in, f32), P, int(N), dptr(out, f32), current_stream()))
    return out


def hyp_broadcast(dst, src, N):
    """dim_hyp_broadcast: the rows of src (P, ...) into dst (P*N, ...), row p into rows p*N .. p*N+N-1 (contiguous 4-byte tensors)"""
    P = src.shape[0]
    assert dst.shape[0] == P * N and tuple(dst.shape[1:]) == tuple(src.shape[1:]) and dst.dtype == src.dtype and src.element_size() == 4
    assert dst.is_contiguous() and src.is_contiguous() and dst.is_cuda and src.is_cuda
    check(lib().dim_hyp_broadcast(dptr(dst), dptr(src), P, int(N), src.numel() // P, current_stream()))
    return dst


def pose_score_workspace(B, H, W, device):
    return _workspace_f64(lib().dim_pose_score_workspace_bytes(B, H, W), device)


def pose_score(image_observed, image_rendered, depth_rendered, mode="rgb", tau=0.02, depth_observed=None, bbox=None, score=None,
               status=None, workspace=None, obs_row=None):
    """dim_pose_score (restated by tests/hyp_reference.py): one score per sample over the drawn pixels of the render inside bbox (B,4)
    int32 (None = whole frame).  mode "rgb": ZNCC of the channel sums of image_observed and image_rendered (B,3,H,W); "depth": the
    fraction of pixels with depth_observed > 0 where |depth_rendered - depth_observed| < tau.  -> score (B,) f32, -inf when it is
    undefined (and DIM_STATUS_HYP_NO_SCORE is OR-ed into status (B,) int32 when given).
    obs_row (B,) int32: dim_pose_score_indexed -- image_observed (n_obs,3,H,W) / depth_observed (n_obs,1,H,W) hold n_obs frames and
    sample b reads frame obs_row[b] (an index outside them: -inf and the status bit)"""
    B, _, H, W = depth_rendered.shape
    if mode not in HYP_SCORE_ID:
        raise ValueError("pose score mode must be 'rgb' or 'depth', got {!r}".format(mode))
    if mode == "depth" and depth_observed is None:
        raise ValueError("the depth pose score needs depth_observed")
    n_obs = image_observed.shape[0] if obs_row is not None else B
    assert tuple(image_observed.shape) == (n_obs, 3, H, W) and tuple(image_rendered.shape) == (B, 3, H, W)
    assert depth_observed is None or tuple(depth_observed.shape) == (n_obs, 1, H, W)
    assert obs_row is None or obs_row.numel() == B
    score = score if score is not None else _new((B,), depth_rendered)
    assert score.numel() == B and (status is None or status.numel() == B) and (bbox is None or bbox.numel() == 4 * B)
    if workspace is None:
        workspace = pose_score_workspace(B, H, W, depth_rendered.device)
    assert workspace.numel() * workspace.element_size() >= lib().dim_pose_score_workspace_bytes(B, H, W)
    if obs_row is not None:
        check(lib().dim_pose_score_indexed(dptr(image_observed, f32), dptr(image_rendered, f32), _opt(depth_observed),
                                           dptr(depth_rendered, f32), _opt(bbox, i32), dptr(obs_row, i32), n_obs, B, H, W,
                                           HYP_SCORE_ID[mode], float(tau), dptr(workspace, torch.float64), dptr(score, f32),
                                           _opt(status, i32), current_stream()))
        return score
    check(lib().dim_pose_score(dptr(image_observed, f32), dptr(image_rendered, f32), _opt(depth_observed), dptr(depth_rendered, f32),
                               _opt(bbox, i32), B, H, W, HYP_SCORE_ID[mode], float(tau), dptr(workspace, torch.float64), dptr(score, f32),
                               _opt(status, i32), current_stream()))
    return score


def hyp_select(score, N, poses_iter, status_iter=None, pose_icp=None, choice=None, poses_sel=None, status_sel=None, pose_icp_sel=None,
               status_load=None):
    """dim_hyp_select: score (P*N,), poses_iter (T,P*N,3,4) -> choice (P,) int32 (largest finite score, ties: smaller h, none: 0),
    poses_sel (T,P,3,4); status_iter (T,P*N) -> status_sel (T,P) and pose_icp (P*N,3,4) -> pose_icp_sel (P,3,4) when given.
    status_load (P*N,) int32: bits OR-ed into the selected last status row (the load-time hypothesis renders)"""
    T, B = poses_iter.shape[0], poses_iter.shape[1]
    assert B % N == 0 and score.numel() == B
    P = B // N
    choice = choice if choice is not None else _new((P,), score, i32)
    poses_sel = poses_sel if poses_sel is not None else _new((T, P, 3, 4), poses_iter)
    if status_iter is not None and status_sel is None:
        status_sel = _new((T, P), status_iter, i32)
    if pose_icp is not None and pose_icp_sel is None:
        pose_icp_sel = _new((P, 3, 4), pose_icp)
    check(lib().dim_hyp_select(dptr(score, f32), P, int(N), T, dptr(poses_iter, f32), _opt(status_iter, i32), _opt(status_load, i32), _opt(pose_icp),
                               dptr(choice, i32),
                               dptr(poses_sel, f32), _opt(status_sel, i32), _opt(pose_icp_sel), current_stream()))
    return choice, poses_sel, status_sel, pose_icp_sel


STATUS_TRACK_LOST = 4096     # DIM_STATUS_TRACK_LOST: dim_track_update did not accept the frame's pose
STATUS_TRACK_REINIT = 8192   # DIM_STATUS_TRACK_REINIT: ... and re-initialised the track from the offered pose
TRACK_MOTION_ID = {"hold": 0, "velocity": 1}   # DIM_TRACK_MOTION_HOLD / DIM_TRACK_MOTION_VELOCITY
TRACK_MAX_WINDOW = 64        # DIM_TRACK_MAX_WINDOW


def track_ingest(frame_bgr, depth_factor, pixel_means_bgr, image_observed, depth_raw=None, depth_observed=None):
    """dim_track_ingest: one camera frame, uint8 BGR (H,W,3) [+ uint16 depth (H,W)], into the observed blobs of P tracks:
    image_observed (P,3,H,W) [, depth_observed (P,1,H,W)], every row the same, every pixel as pair_blobs_from_raw writes it"""
    H, W, _ = frame_bgr.shape
    P = image_observed.shape[0]
    assert tuple(frame_bgr.shape) == (H, W, 3) and tuple(image_observed.shape) == (P, 3, H, W)
    assert depth_raw is None or tuple(depth_raw.shape) == (H, W)
    assert depth_observed is None or tuple(depth_observed.shape) == (P, 1, H, W)
    keep, mp = host_f32(pixel_means_bgr, 3)
    check(lib().dim_track_ingest(dptr(frame_bgr, torch.uint8), _opt(depth_raw, torch.uint16), P, H, W, float(depth_factor), mp,
                                 dptr(image_observed, f32), _opt(depth_observed), current_stream()))
    return image_observed


def track_predict(hist, age, mode="velocity", alpha=1.0, out=None):
    """dim_track_predict (restated by tests/track_reference.py): hist (P,2,3,4) f32, [1] the last accepted pose and [0] the one
    before, age (P,) int32 -> (P,3,4) the pose the next frame starts from: hist[1] bit for bit ("hold", age < 2, a bad history) or the
    damped constant-velocity extrapolation ("velocity", alpha in [0,1])"""
    P = hist.shape[0]
    if mode not in TRACK_MOTION_ID:
        raise ValueError("track motion must be 'hold' or 'velocity', got {!r}".format(mode))
    assert tuple(hist.shape) == (P, 2, 3, 4) and age.numel() == P
    out = out if out is not None else _new((P, 3, 4), hist)
    assert tuple(out.shape) == (P, 3, 4)
    check(lib().dim_track_predict(dptr(hist, f32), dptr(age, i32), P, TRACK_MOTION_ID[mode], float(alpha), dptr(out, f32), current_stream()))
    return out


def _track_update_args(pose_before, pose_new, hist, age, ring, ring_n, ring_pos, lost_rot_deg, lost_trans_m, znear, zfar, status_rows,
                       fatal_mask, score, min_score, reinit_pose, reinit_valid, flags, step, mean):
    """what track_update and track_update_occ share: the checks, flags / step / mean allocated when not given, and the arguments the two
    entries have in common -> (head: pose_before .. P, state: hist .. ring_pos, (flags, step, mean))"""
    P, Wn = ring.shape[0], ring.shape[1]
    assert tuple(pose_before.shape) == (P, 3, 4) and tuple(pose_new.shape) == (P, 3, 4) and tuple(hist.shape) == (P, 2, 3, 4)
    assert tuple(ring.shape) == (P, Wn, 2) and age.numel() == P and ring_n.numel() == P and ring_pos.numel() == P
    n_rows = 0
    if status_rows is not None:
        assert status_rows.numel() % P == 0
        n_rows = status_rows.numel() // P
    assert score is None or score.numel() == P
    assert (reinit_pose is None) == (reinit_valid is None)
    assert reinit_pose is None or (tuple(reinit_pose.shape) == (P, 3, 4) and reinit_valid.numel() == P)
    flags = flags if flags is not None else _new((P,), hist, i32)
    step = step if step is not None else _new((P, 2), hist)
    mean = mean if mean is not None else _new((P, 2), hist)
    assert flags.numel() == P and step.numel() == 2 * P and mean.numel() == 2 * P
    head = (dptr(pose_before, f32), dptr(pose_new, f32), _opt(status_rows, i32), n_rows, int(fatal_mask), _opt(score), float(min_score),
            _opt(reinit_pose), _opt(reinit_valid, i32), float(lost_rot_deg), float(lost_trans_m), int(Wn), float(znear), float(zfar), P)
    state = (dptr(hist, f32), dptr(age, i32), dptr(ring, f32), dptr(ring_n, i32), dptr(ring_pos, i32))
    return head, state, (flags, step, mean)


def track_update(pose_before, pose_new, hist, age, ring, ring_n, ring_pos, lost_rot_deg, lost_trans_m, znear, zfar, status_rows=None,
                 fatal_mask=0, score=None, min_score=0.0, reinit_pose=None, reinit_valid=None, flags=None, step=None, mean=None):
    """dim_track_update (restated by tests/track_reference.py): the per-track state machine after a frame's refinement.  Reads and
    writes hist (P,2,3,4), age (P,), ring (P,Wn,2), ring_n, ring_pos (P,) in place -> flags (P,) int32, step (P,2), mean (P,2).
    status_rows (n_rows,P) int32 are OR-ed; score (P,) f32 and reinit_pose (P,3,4) / reinit_valid (P,) int32 are optional"""
    head, state, (flags, step, mean) = _track_update_args(pose_before, pose_new, hist, age, ring, ring_n, ring_pos, lost_rot_deg, lost_trans_m,
                                                          znear, zfar, status_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid,
                                                          flags, step, mean)
    check(lib().dim_track_update(*head, *state, dptr(flags, i32), dptr(step, f32), dptr(mean, f32), current_stream()))
    return flags, step, mean


STATUS_TRACK_OCCLUDED = 16384   # DIM_STATUS_TRACK_OCCLUDED: dim_track_update_occ saw too little of the track's render
TRACK_OCC_MODE = {"tracks": 1, "depth": 2, "both": 3}   # DIM_TRACK_OCC_TRACKS | DIM_TRACK_OCC_DEPTH


def track_visibility_workspace(P, H, W, device):
    return torch.empty((max(lib().dim_track_visibility_workspace_bytes(P, H, W), 4) // 4,), dtype=i32, device=device)


def track_visibility(depth_rendered, mode, delta, depth_frame=None, occluder_ok=None, depth_visible=None, counts=None, workspace=None):
    """dim_track_visibility (restated by tests/track_occ_reference.py): depth_rendered (P,1,H,W), the renders of P tracks at one camera
    -> depth_visible (P,1,H,W), the render with the pixels zeroed that another track ("tracks": one whose occluder_ok (P,) int32 entry is
    not 0) or the frame's depth ("depth": depth_frame (H,W) metres, 0 = no reading) hides by more than delta metres ("both": either),
    and counts (P,4) int32 = {drawn, visible, hidden by a track, hidden by the frame's depth only}"""
    P, _, H, W = depth_rendered.shape
    if mode not in TRACK_OCC_MODE:
        raise ValueError("track occlusion mode must be 'tracks', 'depth' or 'both', got {!r}".format(mode))
    if TRACK_OCC_MODE[mode] & 2 and depth_frame is None:
        raise ValueError("track occlusion mode {!r} needs depth_frame".format(mode))
    assert tuple(depth_rendered.shape) == (P, 1, H, W) and (depth_frame is None or tuple(depth_frame.shape) == (H, W))
    assert occluder_ok is None or occluder_ok.numel() == P
    depth_visible = depth_visible if depth_visible is not None else _new((P, 1, H, W), depth_rendered)
    counts = counts if counts is not None else _new((P, 4), depth_rendered, i32)
    assert tuple(depth_visible.shape) == (P, 1, H, W) and counts.numel() == 4 * P
    if workspace is None:
        workspace = track_visibility_workspace(P, H, W, depth_rendered.device)
    assert workspace.numel() * workspace.element_size() >= lib().dim_track_visibility_workspace_bytes(P, H, W)
    check(lib().dim_track_visibility(dptr(depth_rendered, f32), _opt(depth_frame), _opt(occluder_ok, i32), P, H, W, TRACK_OCC_MODE[mode],
                                     float(delta), dptr(workspace), dptr(depth_visible, f32), dptr(counts, i32), current_stream()))
    return depth_visible, counts


def track_update_occ(pose_before, pose_new, hist, age, ring, ring_n, ring_pos, occ_age, counts, min_visible, max_occluded, pose_pred,
                     lost_rot_deg, lost_trans_m, znear, zfar, status_rows=None, fatal_mask=0, score=None, min_score=0.0, reinit_pose=None,
                     reinit_valid=None, flags=None, step=None, mean=None, visible=None, pose_track=None, occluder_ok=None):
    """dim_track_update_occ (restated by tests/track_occ_reference.py): track_update with an occluded state.  counts (P,4) int32 of
    track_visibility for the render of pose_new; a track of which less than min_visible is visible takes pose_pred (P,3,4), the pose
    the frame started from, for at most max_occluded frames in a row (state occ_age (P,) int32) instead of being lost.
    -> flags (STATUS_TRACK_OCCLUDED among them), step, mean, visible (P,) f32, pose_track (P,3,4) = hist[:, 1] after the update,
    occluder_ok (P,) int32: 0 for a track that is lost and not re-initialised"""
    head, state, (flags, step, mean) = _track_update_args(pose_before, pose_new, hist, age, ring, ring_n, ring_pos, lost_rot_deg, lost_trans_m,
                                                          znear, zfar, status_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid,
                                                          flags, step, mean)
    P = ring.shape[0]
    assert occ_age.numel() == P and counts.numel() == 4 * P and tuple(pose_pred.shape) == (P, 3, 4)
    visible = visible if visible is not None else _new((P,), hist)
    pose_track = pose_track if pose_track is not None else _new((P, 3, 4), hist)
    occluder_ok = occluder_ok if occluder_ok is not None else _new((P,), hist, i32)
    assert visible.numel() == P and tuple(pose_track.shape) == (P, 3, 4) and occluder_ok.numel() == P
    check(lib().dim_track_update_occ(*head, dptr(counts, i32), float(min_visible), int(max_occluded), dptr(pose_pred, f32), *state,
                                     dptr(occ_age, i32), dptr(flags, i32), dptr(step, f32), dptr(mean, f32), dptr(visible, f32),
                                     dptr(pose_track, f32), dptr(occluder_ok, i32), current_stream()))
    return flags, step, mean, visible, pose_track, occluder_ok


STATUS_TRACK_SEG_NO_MODEL = 131072   # DIM_STATUS_TRACK_SEG_NO_MODEL: dim_track_seg_mask had no colour model or no region for the track


def track_seg_workspace(P, H, W, bits, device):
    """the workspace of track_seg_mask and track_seg_learn (they use disjoint parts of it); needs no initialisation"""
    n = lib().dim_track_seg_workspace_bytes(P, H, W, int(bits))
    if n <= 0:
        raise ValueError("track_seg_workspace: P = {}, H = {}, W = {}, bits = {}".format(P, H, W, bits))
    return torch.empty((n // 4,), dtype=i32, device=device)


def _track_seg_shapes(frame_bgr, bbox, seg_hist, seg_age, bits, workspace):
    H, W, _ = frame_bgr.shape
    P, NB = bbox.shape[0], 1 << (3 * int(bits))
    assert tuple(frame_bgr.shape) == (H, W, 3) and tuple(bbox.shape) == (P, 4)
    assert tuple(seg_hist.shape) == (P, 2, NB) and seg_age.numel() == P
    if workspace is None:
        workspace = track_seg_workspace(P, H, W, bits, frame_bgr.device)
    assert workspace.numel() * workspace.element_size() >= lib().dim_track_seg_workspace_bytes(P, H, W, int(bits))
    return P, H, W, workspace


def track_seg_mask(frame_bgr, bbox, seg_hist, seg_age, bits, margin, radius, mask=None, counts=None, status=None, workspace=None):
    """dim_track_seg_mask (restated by tests/track_seg_reference.py): frame_bgr (H,W,3) uint8, bbox (P,4) int32 of the tracks' renders,
    the colour model seg_hist (P,2,NB) f32 / seg_age (P,) int32 -> mask (P,1,H,W) f32 of 0 / 1 (every word written): inside the box
    grown by `margin`, the pixels whose colour bin is more frequent in the foreground than in the background histogram, after an
    integer majority filter of `radius`; counts (P,2) int32 = {region pixels, mask pixels}; STATUS_TRACK_SEG_NO_MODEL is OR-ed into
    status (P,) int32 for a track without a model or a region"""
    P, H, W, workspace = _track_seg_shapes(frame_bgr, bbox, seg_hist, seg_age, bits, workspace)
    mask = mask if mask is not None else _new((P, 1, H, W), seg_hist)
    counts = counts if counts is not None else _new((P, 2), seg_hist, i32)
    assert tuple(mask.shape) == (P, 1, H, W) and counts.numel() == 2 * P and (status is None or status.numel() == P)
    check(lib().dim_track_seg_mask(dptr(frame_bgr, torch.uint8), dptr(bbox, i32), dptr(seg_hist, f32), dptr(seg_age, i32), P, H, W, int(bits),
                                   int(margin), int(radius), dptr(workspace), dptr(mask, f32), dptr(counts, i32), _opt(status, i32),
                                   current_stream()))
    return mask, counts


def track_seg_learn(frame_bgr, depth_drawn, bbox, seg_hist, seg_age, bits, margin, rate, min_pixels, depth_fg=None, flags=None, skip_mask=0,
                    counts=None, workspace=None):
    """dim_track_seg_learn (restated by tests/track_seg_reference.py): one update of the colour model, in place.  depth_drawn (P,1,H,W)
    each track's own render, depth_fg (P,1,H,W) what of it is visible (None = depth_drawn), bbox (P,4) of that render: inside the box
    grown by `margin` the visible pixels feed the foreground and the pixels the render does not draw the background histogram, blended
    at `rate` (the first update sets them).  A track with flags (P,) int32 & skip_mask, or fewer than min_pixels of either class, keeps
    seg_hist (P,2,NB) and seg_age (P,) bit for bit -> counts (P,2) int32 = {foreground, background pixels}"""
    P, H, W, workspace = _track_seg_shapes(frame_bgr, bbox, seg_hist, seg_age, bits, workspace)
    assert tuple(depth_drawn.shape) == (P, 1, H, W) and (depth_fg is None or tuple(depth_fg.shape) == (P, 1, H, W))
    assert flags is None or flags.numel() == P
    counts = counts if counts is not None else _new((P, 2), seg_hist, i32)
    assert counts.numel() == 2 * P
    check(lib().dim_track_seg_learn(dptr(frame_bgr, torch.uint8), dptr(depth_drawn, f32), _opt(depth_fg), dptr(bbox, i32), _opt(flags, i32),
                                    int(skip_mask), P, H, W, int(bits), int(margin), float(rate), int(min_pixels), dptr(workspace), dptr(seg_hist, f32),
                                    dptr(seg_age, i32), dptr(counts, i32), current_stream()))
    return counts


STATUS_COARSE_BAD_BOX = 512  # DIM_STATUS_COARSE_BAD_BOX: dim_pose_from_box gave the candidate its fallback row
HYP_TOPK_MAX = 64             # dim_hyp_topk: the largest k


def pose_from_box(points, table_off, class_index, rot_table, boxes, K, iters=8, z_init=1.0, K_per_sample=None, pose_out=None,
                  pose_out_f64=None, status=None):
    """dim_pose_from_box (restated by tests/coarse_reference.py): M candidate poses per pair, sample p*M+m = [R_m | t] with t fitted so
    that the projected model points of the pair's class fill its box.  points (Ntot,3) f64 and table_off (n_classes+1,) int32 as
    PoseEvaluator.device_tables returns them, class_index (P,) int32, rot_table (M,3,3) or (M,9) f32, boxes (P,4) f32 {x0,x1,y0,y1}
    continuous pixel extents, K the host 3x3 unless K_per_sample ((P,3,3) / (P,9)) is given.  -> (pose_out (P*M,3,4) f32, status
    (P*M,) int32: DIM_STATUS_COARSE_BAD_BOX / DIM_STATUS_BAD_CLASS are OR-ed in, zeroed when allocated here); pose_out_f64 (P*M,3,4)
    f64 is filled when given"""
    f64 = torch.float64
    P, M = class_index.numel(), rot_table.numel() // 9
    assert rot_table.numel() == 9 * M and tuple(boxes.shape) == (P, 4) and points.dim() == 2 and points.shape[1] == 3
    dev = boxes.device
    pose_out = pose_out if pose_out is not None else torch.empty((P * M, 3, 4), dtype=f32, device=dev)
    status = status if status is not None else torch.zeros((P * M,), dtype=i32, device=dev)
    assert pose_out.numel() == P * M * 12 and status.numel() == P * M and (pose_out_f64 is None or pose_out_f64.numel() == P * M * 12)
    kps = _kps_f64(K_per_sample, P, dev, "pose_from_box:")
    keep = _host_k9_f64(K)
    check(lib().dim_pose_from_box(dptr(points, f64), dptr(table_off, i32), table_off.numel() - 1, dptr(class_index, i32), dptr(rot_table, f32),
                                  dptr(boxes, f32), keep.ctypes.data, _opt(kps, f64), P, M, int(iters), float(z_init), dptr(pose_out, f32),
                                  _opt(pose_out_f64, f64), dptr(status, i32), current_stream()))
    return pose_out, status


def hyp_topk(score, M, k, poses_in, status_in=None, reject_mask=0, idx_out=None, score_out=None, poses_out=None, status_out=None):
    """dim_hyp_topk: score (P*M,), poses_in (P*M,3,4) -> per pair the k largest finite scores in descending order (ties: the smaller
    m; a candidate with status_in & reject_mask is skipped): idx_out (P,k) int32, score_out (P,k), poses_out (P,k,3,4), status_out
    (P,k) int32 = the candidate's status_in bits, DIM_STATUS_HYP_NO_SCORE on the slots that repeat slot 0 for want of candidates"""
    B = score.numel()
    assert B % M == 0 and poses_in.numel() == 12 * B and (status_in is None or status_in.numel() == B)
    P = B // M
    idx_out = idx_out if idx_out is not None else _new((P, k), score, i32)
    score_out = score_out if score_out is not None else _new((P, k), score)
    poses_out = poses_out if poses_out is not None else _new((P, k, 3, 4), score)
    status_out = status_out if status_out is not None else _new((P, k), score, i32)
    assert idx_out.numel() == P * k and score_out.numel() == P * k and poses_out.numel() == P * k * 12 and status_out.numel() == P * k
    check(lib().dim_hyp_topk(dptr(score, f32), _opt(status_in, i32), int(reject_mask), P, int(M), int(k), dptr(poses_in, f32),
                             dptr(idx_out, i32), dptr(score_out, f32), dptr(poses_out, f32), dptr(status_out, i32), current_stream()))
    return idx_out, score_out, poses_out, status_out


STATUS_BAD_CLASS = 4     # DIM_STATUS_BAD_CLASS: dim_pose_errors gave the pair a NaN row (class index outside the table)
POSE_ERR_ADI = 1         # DIM_POSE_ERR_ADI: the class's adi column is filled
POSE_ERR_FLIP_Z180 = 2   # DIM_POSE_ERR_FLIP_Z180: the eggbox rule of lib/dataset/evaluation.py
POSE_ERR_COLUMNS = ("re", "te", "add", "adi", "arp_2d")


def pose_errors_workspace(T, B, max_points, device):
    return _workspace_f64(lib().dim_pose_errors_workspace_bytes(T, B, max_points), device)


def pose_errors(points, table_off, class_flags, class_index, poses_est, pose_gt, K, errors=None, status=None, workspace=None):
    """dim_pose_errors: the five errors of lib/utils/pose_error.py in float64 on the device.  points (Ntot,3) f64, table_off
    (n_classes+1,) and class_flags (n_classes,) int32 as PoseEvaluator.device_tables returns them, class_index (B,) int32, poses_est
    (T,B,3,4) or (B,3,4) (= T 1) float32 or float64, pose_gt (B,3,4) f64, K the host 3x3.  -> errors (T,B,5) f64 (POSE_ERR_COLUMNS;
    (B,5) for a (B,3,4) input); DIM_STATUS_BAD_CLASS is OR-ed into status (B,) int32 when given"""
    f64 = torch.float64
    if poses_est.dtype not in (f32, f64):
        raise capi.DeepIMHipError("pose_errors: poses_est must be float32 or float64, got {}".format(poses_est.dtype))
    single = poses_est.dim() == 3
    T = 1 if single else poses_est.shape[0]
    B = poses_est.shape[-3]
    n_classes = class_flags.numel()
    assert tuple(poses_est.shape[-3:]) == (B, 3, 4) and poses_est.dim() in (3, 4) and tuple(pose_gt.shape) == (B, 3, 4)
    assert points.dim() == 2 and points.shape[1] == 3 and table_off.numel() == n_classes + 1 and class_index.numel() == B
    if errors is None:
        errors = torch.empty((B, 5) if single else (T, B, 5), dtype=f64, device=poses_est.device)
    assert errors.numel() == T * B * 5 and (status is None or status.numel() == B)
    if workspace is None:
        workspace = pose_errors_workspace(T, B, points.shape[0], poses_est.device)
    assert workspace.numel() * workspace.element_size() >= lib().dim_pose_errors_workspace_bytes(T, B, points.shape[0])
    keep = _host_k9_f64(K)
    is32 = poses_est.dtype == f32
    check(lib().dim_pose_errors(dptr(points, f64), dptr(table_off, i32), dptr(class_flags, i32), n_classes, dptr(class_index, i32),
                                dptr(poses_est, f32) if is32 else None, None if is32 else dptr(poses_est, f64), dptr(pose_gt, f64),
                                keep.ctypes.data, T, B, dptr(workspace), dptr(errors, f64), _opt(status, i32),
                                current_stream()))
    return errors


VSD_COST_ID = {"step": 0, "tlinear": 1}   # DIM_VSD_COST_STEP / DIM_VSD_COST_TLINEAR
VSD_MAX_TAU = 8                            # DIM_VSD_MAX_TAU
VSD_COUNT_COLUMNS = ("visib_gt", "union", "inter", "drawn_gt")


def vsd_workspace(T, B, device):
    return _workspace_f64(lib().dim_vsd_workspace_bytes(T, B), device)


def vsd_errors(depth_obs, depth_gt, depth_est, K, delta, taus, cost_type="step", K_per_sample=None, bbox_gt=None, bbox_est=None,
               errors=None, counts=None, workspace=None):
    """dim_vsd_errors (restated by lib/utils/pose_error.py vsd): the visible surface discrepancy of T pose sets of B pairs.
    depth_obs, depth_gt (B,H,W) or (B,1,H,W) and depth_est (T,B,H,W), (T,B,1,H,W) or one set shaped like depth_gt (= T 1): float32
    metres.  K: the host 3x3 used for every pair unless K_per_sample ((B,3,3) / (B,9), host array or CUDA tensor, made float64) is
    given.  taus: one number or up to 8, all scored from one read of the planes.  bbox_gt (B,4) / bbox_est (T,B,4) int32: the boxes
    the two renders returned, both or neither.  -> errors (T,B,n_tau) f64, counts (T,B,4) int32 (VSD_COUNT_COLUMNS); without the T
    axis for a single set"""
    f64 = torch.float64
    if cost_type not in VSD_COST_ID:
        raise ValueError("vsd cost_type must be 'step' or 'tlinear', got {!r}".format(cost_type))
    tau = np.ascontiguousarray(np.asarray(taus, dtype=np.float64).reshape(-1))
    if not 1 <= tau.size <= VSD_MAX_TAU or not np.all(tau > 0):
        raise ValueError("vsd taus: 1 to {} distances > 0, got {!r}".format(VSD_MAX_TAU, taus))
    H, W = depth_gt.shape[-2:]
    B = depth_gt.shape[0]
    assert depth_gt.numel() == B * H * W and tuple(depth_obs.shape) == tuple(depth_gt.shape)
    single = depth_est.dim() == depth_gt.dim()
    T = 1 if single else depth_est.shape[0]
    assert depth_est.numel() == T * B * H * W and tuple(depth_est.shape[-2:]) == (H, W)
    dev = depth_gt.device
    if errors is None:
        errors = torch.empty((B, tau.size) if single else (T, B, tau.size), dtype=f64, device=dev)
    if counts is None:
        counts = torch.empty((B, 4) if single else (T, B, 4), dtype=i32, device=dev)
    assert errors.numel() == T * B * tau.size and counts.numel() == T * B * 4
    assert (bbox_gt is None) == (bbox_est is None), "vsd_errors: both boxes or neither"
    assert bbox_gt is None or (bbox_gt.numel() == 4 * B and bbox_est.numel() == 4 * T * B)
    if workspace is None:
        workspace = vsd_workspace(T, B, dev)
    assert workspace.numel() * workspace.element_size() >= lib().dim_vsd_workspace_bytes(T, B)
    keep = _host_k9_f64(K)
    kps = _kps_f64(K_per_sample, B, dev, "vsd")
    check(lib().dim_vsd_errors(dptr(depth_obs, f32), dptr(depth_gt, f32), dptr(depth_est, f32), keep.ctypes.data, _opt(kps, f64),
                               _opt(bbox_gt, i32), _opt(bbox_est, i32), T, B, H, W, float(delta), tau.ctypes.data, int(tau.size),
                               VSD_COST_ID[cost_type], dptr(workspace), dptr(errors, f64), dptr(counts, i32), current_stream()))
    return errors, counts


VSD_GRID_MAX_TAU = 16   # DIM_VSD_GRID_MAX_TAU


def vsd_grid_workspace(T, B, device):
    return _workspace_f64(lib().dim_vsd_grid_workspace_bytes(T, B), device)


def vsd_tau_table(tau_table, device):
    """the tau table of vsd_grid_errors on `device`: a ready CUDA float64 tensor (n_classes, n_tau) is used where it lies; a host
    array is checked (finite, > 0, shape (n_classes >= 1, 1..16)) and uploaded"""
    if isinstance(tau_table, torch.Tensor) and tau_table.is_cuda:
        if tau_table.dtype != torch.float64 or tau_table.dim() != 2 or not tau_table.is_contiguous():
            raise ValueError("vsd tau_table on the device must be a contiguous float64 (n_classes, n_tau) tensor, got {} {}".format(
                tau_table.dtype, tuple(tau_table.shape)))
        table = tau_table
    else:
        a = np.asarray(tau_table, dtype=np.float64)
        if a.ndim != 2 or not (np.all(np.isfinite(a)) and np.all(a > 0)):
            raise ValueError("vsd tau_table: (n_classes, n_tau) finite distances > 0, got {!r}".format(tau_table))
        table = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if table.shape[0] < 1 or not 1 <= table.shape[1] <= VSD_GRID_MAX_TAU:
        raise ValueError("vsd tau_table: at least one class and 1 to {} taus per class, got shape {}".format(
            VSD_GRID_MAX_TAU, tuple(table.shape)))
    return table


def vsd_grid_errors(depth_obs, depth_gt, depth_est, K, delta, class_index, tau_table, K_per_sample=None, bbox_gt=None, bbox_est=None,
                    errors=None, counts=None, n_ge=None, workspace=None):
    """dim_vsd_grid_errors: the step-cost VSD of T pose sets of B pairs at the taus of each pair's class, from one read of the planes
    (BOP's grid: ten fractions of the class diameter).  Planes, K, K_per_sample and the boxes as vsd_errors takes them.  class_index
    (B,) int32 CUDA; tau_table (n_classes, n_tau <= 16) metres: a host array (checked and uploaded, see vsd_tau_table) or a ready CUDA
    float64 tensor (PoseEvaluator.device_vsd_tau_table).  -> errors (T,B,n_tau) f64 with the bits of pose_error.vsd(..., "step"),
    counts (T,B,4) int32 (VSD_COUNT_COLUMNS), n_ge (T,B,n_tau) int32 = pixels of the intersection with |S_gt - S_est| >= tau; without
    the T axis for a single set.  A class index outside the table: a NaN row, zero counts and n_ge"""
    f64 = torch.float64
    H, W = depth_gt.shape[-2:]
    B = depth_gt.shape[0]
    assert depth_gt.numel() == B * H * W and tuple(depth_obs.shape) == tuple(depth_gt.shape)
    single = depth_est.dim() == depth_gt.dim()
    T = 1 if single else depth_est.shape[0]
    assert depth_est.numel() == T * B * H * W and tuple(depth_est.shape[-2:]) == (H, W)
    dev = depth_gt.device
    table = vsd_tau_table(tau_table, dev)
    n_classes, n_tau = table.shape
    assert class_index.numel() == B
    lead = (B,) if single else (T, B)
    if errors is None:
        errors = torch.empty(lead + (n_tau,), dtype=f64, device=dev)
    if counts is None:
        counts = torch.empty(lead + (4,), dtype=i32, device=dev)
    if n_ge is None:
        n_ge = torch.empty(lead + (n_tau,), dtype=i32, device=dev)
    assert errors.numel() == T * B * n_tau and counts.numel() == T * B * 4 and n_ge.numel() == T * B * n_tau
    assert (bbox_gt is None) == (bbox_est is None), "vsd_grid_errors: both boxes or neither"
    assert bbox_gt is None or (bbox_gt.numel() == 4 * B and bbox_est.numel() == 4 * T * B)
    if workspace is None:
        workspace = vsd_grid_workspace(T, B, dev)
    assert workspace.numel() * workspace.element_size() >= lib().dim_vsd_grid_workspace_bytes(T, B)
    keep = _host_k9_f64(K)
    kps = _kps_f64(K_per_sample, B, dev, "vsd_grid")
    check(lib().dim_vsd_grid_errors(dptr(depth_obs, f32), dptr(depth_gt, f32), dptr(depth_est, f32), keep.ctypes.data, _opt(kps, f64),
                                    _opt(bbox_gt, i32), _opt(bbox_est, i32), dptr(class_index, i32), dptr(table, f64), int(n_classes),
                                    int(n_tau), T, B, H, W, float(delta), dptr(workspace), dptr(errors, f64), dptr(counts, i32),
                                    dptr(n_ge, i32), current_stream()))
    return errors, counts, n_ge


BOP_ERR_COLUMNS = ("mssd", "mspd")


def bop_errors_workspace(T, B, max_sym, device):
    return _workspace_f64(lib().dim_bop_errors_workspace_bytes(T, B, max_sym), device)


def bop_errors(points, table_off, sym, sym_off, class_index, poses_est, pose_gt, K, max_sym, K_per_sample=None, errors=None,
               best_sym=None, status=None, workspace=None):
    """dim_bop_errors (restated by lib/utils/pose_error.py mssd / mspd): the BOP symmetry-aware errors in float64 on the device.
    points (Ntot,3) f64 and table_off (n_classes+1,) int32 as PoseEvaluator.device_tables returns them, sym (Stot,3,4) f64 and
    sym_off (n_classes+1,) int32 as PoseEvaluator.device_sym_tables does, class_index (B,) int32, poses_est (T,B,3,4) or (B,3,4)
    (= T 1) float32 or float64, pose_gt (B,3,4) f64.  K: the host 3x3 used for every pair unless K_per_sample ((B,3,3) / (B,9), host
    array or CUDA tensor, made float64) is given.  max_sym: at least the largest set of a class that occurs (a larger set gives a NaN
    row); it sizes the workspace.  -> errors (T,B,2) f64 (BOP_ERR_COLUMNS), best_sym (T,B,2) int32: the index within the class's set
    that attains each minimum; without the T axis for a (B,3,4) input.  DIM_STATUS_BAD_CLASS is OR-ed into status (B,) int32 when given"""
    f64 = torch.float64
    if poses_est.dtype not in (f32, f64):
        raise capi.DeepIMHipError("bop_errors: poses_est must be float32 or float64, got {}".format(poses_est.dtype))
    single = poses_est.dim() == 3
    T = 1 if single else poses_est.shape[0]
    B = poses_est.shape[-3]
    n_classes = table_off.numel() - 1
    max_sym = int(max_sym)
    assert tuple(poses_est.shape[-3:]) == (B, 3, 4) and poses_est.dim() in (3, 4) and tuple(pose_gt.shape) == (B, 3, 4)
    assert points.dim() == 2 and points.shape[1] == 3 and sym_off.numel() == n_classes + 1 and class_index.numel() == B
    assert sym.dim() == 3 and tuple(sym.shape[1:]) == (3, 4)
    dev = poses_est.device
    if errors is None:
        errors = torch.empty((B, 2) if single else (T, B, 2), dtype=f64, device=dev)
    if best_sym is None:
        best_sym = torch.empty((B, 2) if single else (T, B, 2), dtype=i32, device=dev)
    assert errors.numel() == T * B * 2 and best_sym.numel() == T * B * 2 and (status is None or status.numel() == B)
    if workspace is None:
        workspace = bop_errors_workspace(T, B, max_sym, dev)
    assert max_sym <= 0 or workspace.numel() * workspace.element_size() >= lib().dim_bop_errors_workspace_bytes(T, B, max_sym)
    keep = _host_k9_f64(K)
    kps = _kps_f64(K_per_sample, B, dev, "bop")
    is32 = poses_est.dtype == f32
    check(lib().dim_bop_errors(dptr(points, f64), dptr(table_off, i32), dptr(sym, f64), dptr(sym_off, i32), n_classes,
                               dptr(class_index, i32), dptr(poses_est, f32) if is32 else None, None if is32 else dptr(poses_est, f64),
                               dptr(pose_gt, f64), keep.ctypes.data, _opt(kps, f64), T, B, max_sym,
                               dptr(workspace), dptr(errors, f64), dptr(best_sym, i32), _opt(status, i32),
                               current_stream()))
    return errors, best_sym


STATUS_BAD_FACE = 8   # DIM_STATUS_BAD_FACE: a z-buffer key of dim_raster_render* named a face outside the mesh (pixel left black)
STATUS_BAD_K = 16   # DIM_STATUS_BAD_K: dim_raster_render_k drew the sample as background (fx <= 0, fy <= 0 or a non-finite entry)


def intrinsics_per_sample(K, B, device):
    """the K argument of a batched render -> None (one camera for the batch: None or nine values, the uniform path) or a contiguous
    (B,9) f32 CUDA tensor for dim_raster_render_k.  K: (B,3,3) or (B,9), a host array or a CUDA tensor; a CUDA f32 tensor that is
    already contiguous is used where it lies (a captured graph then renders with whatever it holds at replay).  Any other shape
    raises ValueError before anything is launched."""
    if K is None:
        return None
    if isinstance(K, torch.Tensor) and K.is_cuda:
        if tuple(K.shape) in ((B, 3, 3), (B, 9)):
            return K.to(device=device, dtype=f32).reshape(B, 9).contiguous()
        if K.numel() == 9:
            return None
        raise ValueError("per-sample K must be (B,3,3) or (B,9) with B = {}, got {}".format(B, tuple(K.shape)))
    a = np.asarray(K, dtype=np.float32)
    if a.size == 9:
        return None
    if a.shape not in ((B, 3, 3), (B, 9)):
        raise ValueError("K must be a 3x3 matrix or per-sample (B,3,3) / (B,9) with B = {}, got {}".format(B, a.shape))
    return torch.from_numpy(np.ascontiguousarray(a.reshape(B, 9))).to(device)


def raster_render(rm, class_index, poses, workspace, K=None, K_per_sample=None, light_position=None, light_intensity=None,
                  brightness_ratio=0.0, lm=False, plane_means=None, mask_thr=0.2, image=None, depth=None, mask=None, bgr=None, bbox=None,
                  status=None, clean_bbox=None):
    """Render machine `rm` (lib/render_hip: its mesh table, K, znear / zfar; lit when it has normals) into whichever outputs are given.
    K: another uniform camera than rm.K (nine values); K_per_sample: (B,9) f32 CUDA (intrinsics_per_sample), one camera per sample, or
    None.  lm: dim_raster_render_lit_lm, the LINEMOD light rule (the light colour scales the diffuse term only; rm must have normals and
    both light tensors (B,3) f32 CUDA are required); otherwise dim_raster_render_k, which with K_per_sample None is
    dim_raster_render_dirty argument for argument.  workspace: rm's for this B."""
    keep, k9 = host_f32(rm.K if K is None else K, 9)   # (keeps the host array alive through the call)
    pm = host_f32(plane_means, 3) if plane_means is not None else (None, None)
    render = lib().dim_raster_render_lit_lm if lm else lib().dim_raster_render_k
    check(render(
        dptr(rm.verts), _opt(getattr(rm, "normals", None)), dptr(rm.uvs), dptr(rm.faces), dptr(rm.mesh_table), int(rm.mesh_table.shape[0]),
        rm.vmax, rm.fmax, dptr(rm.textures), dptr(rm.tex_table), dptr(class_index, i32), dptr(poses, f32), k9, poses.shape[0], rm.height,
        rm.width, float(rm.zNear), float(rm.zFar), int(rm.tex_bilinear), _opt(light_position), _opt(light_intensity), float(brightness_ratio),
        pm[1], float(mask_thr), workspace.data_ptr(), dptr(image), dptr(depth), dptr(mask), dptr(bgr), _opt(bbox, i32), _opt(status, i32),
        _opt(clean_bbox, i32), _opt(K_per_sample), current_stream()))


STATUS_LAYER_HIDDEN = 256   # DIM_STATUS_LAYER_HIDDEN: dim_scene_compose, a used layer won no pixel


def scene_compose_workspace(N, S, H, W, device):
    """the partial-row workspace of scene_compose (needed for counts / vis_bbox / status); allocate before a graph capture"""
    n = lib().dim_scene_compose_workspace_bytes(N, S, H, W)
    return torch.empty(((n + 3) // 4,), dtype=i32, device=device)


def scene_compose(layer_bgr, layer_depth, layer_label, S, scene_bgr=None, scene_depth=None, scene_label=None, vis_mask=None, counts=None,
                  vis_bbox=None, status=None, workspace=None):
    """dim_scene_compose: N scenes of S layers.  layer_bgr (N*S,H,W,3) f32 or None, layer_depth (N*S,1,H,W) f32, layer_label (N*S,)
    int32 (<= 0: unused slot).  Every output is written only when its tensor is given: scene_bgr (N,H,W,3), scene_depth / scene_label
    (N,1,H,W), vis_mask (N*S,1,H,W), counts (N*S,2) int32 {full, visible}, vis_bbox (N*S,4) int32, status (N*S,) int32 (OR-ed into).
    workspace: scene_compose_workspace(...); allocated here when counts / vis_bbox / status are asked for and none is given."""
    NS, _, H, W = layer_depth.shape
    if S < 1 or NS % S:
        raise ValueError("{} layers cannot be split into scenes of S = {}".format(NS, S))
    N = NS // S
    if workspace is None and (counts is not None or vis_bbox is not None or status is not None):
        workspace = scene_compose_workspace(N, S, H, W, layer_depth.device)
    check(lib().dim_scene_compose(dptr(layer_bgr, f32), dptr(layer_depth, f32), dptr(layer_label, i32), N, S, H, W, dptr(workspace, i32),
                                  dptr(scene_bgr, f32), dptr(scene_depth, f32), dptr(scene_label, f32), dptr(vis_mask, f32),
                                  dptr(counts, i32), dptr(vis_bbox, i32), dptr(status, i32), current_stream()))


def box_mask(bbox, mask, bbox_of_mask=None):
    """mask <- filled rectangle of bbox (end-exclusive); bbox_of_mask (B,4) int32: optional bbox of that rectangle"""
    B, _, H, W = mask.shape
    check(lib().dim_box_mask(dptr(bbox, i32), dptr(mask, f32), B, H, W, dptr(bbox_of_mask, i32) if bbox_of_mask is not None else None,
                             current_stream()))
    return mask


def test_blobs_from_raw(obs_bgr, ren_bgr, depth_ren, depth_factor, pixel_means_bgr, image_observed, image_rendered, mask_rendered, bbox,
                        mask_thr=0.2):
    """uint8 BGR images (B,H,W,3) + uint16 rendered depth (B,H,W) -> the float blobs of a test batch, on the device (csrc/data.hip)"""
    B, H, W = depth_ren.shape
    keep, mp = host_f32(pixel_means_bgr, 3)
    check(lib().dim_test_blobs_from_raw(dptr(obs_bgr, torch.uint8), dptr(ren_bgr, torch.uint8), dptr(depth_ren, torch.uint16), B, H, W,
                                        float(depth_factor), mp, float(mask_thr), dptr(image_observed, f32), dptr(image_rendered, f32),
                                        dptr(mask_rendered, f32), dptr(bbox, i32), current_stream()))


def pair_blobs_from_raw(B, H, W, depth_factor, pixel_means_bgr, obs_bgr=None, bg_bgr=None, use_bg=None, ren_bgr=None, depth_ren=None,
                        depth_a=None, depth_b=None, label=None, mask_idx=None, image_observed=None, image_rendered=None, mask_rendered=None,
                        depth_rendered=None, depth_a_out=None, depth_b_out=None, mask_label=None, label_raw=None, bbox_ren=None,
                        bbox_label=None, mask_thr=0.2):
    """raw file pixels of B pairs -> float blobs of a training / test batch on the device (csrc/data.hip; include/deepim_hip.h lists the
    rules); every tensor optional"""
    keep, mp = host_f32(pixel_means_bgr, 3)
    u8, u16 = torch.uint8, torch.uint16
    check(lib().dim_pair_blobs_from_raw(dptr(obs_bgr, u8), dptr(bg_bgr, u8), dptr(use_bg, i32), dptr(ren_bgr, u8), dptr(depth_ren, u16),
                                        dptr(depth_a, u16), dptr(depth_b, u16), dptr(label, u8), dptr(mask_idx, i32), B, H, W,
                                        float(depth_factor), mp, float(mask_thr), dptr(image_observed, f32), dptr(image_rendered, f32),
                                        dptr(mask_rendered, f32), dptr(depth_rendered, f32), dptr(depth_a_out, f32), dptr(depth_b_out, f32),
                                        dptr(mask_label, f32), dptr(label_raw, f32), dptr(bbox_ren, i32), dptr(bbox_label, i32),
                                        current_stream()))


def mask_dilate(mask_in, thickness4, out=None):
    """mask_dilate.py:10-55 with the caller's draws: thickness4 (B,4) int32 = {down, up, right, left}, 0 = side skipped"""
    B, _, H, W = mask_in.shape
    out = out if out is not None else torch.empty_like(mask_in)
    check(lib().dim_mask_dilate(dptr(mask_in, f32), dptr(thickness4, i32), dptr(out, f32), B, H, W, current_stream()))
    return out


def augment_observed(image, on, radius, taps, chain, seed, pixel_means_bgr, quantize=True, out=None):
    """photometric augmentation of an image_observed blob (B,3,H,W) with the caller's draws (csrc/augment.hip; include/deepim_hip.h lists
    the rules; lib/utils/augment.py draws them).  Device tensors: on (B,) int32, taps (B,15) f32, chain (B,7) f32 = {saturation,
    contrast, brightness, gain of plane 0, 1, 2, noise sigma}, seed (B,) int32 holding the uint32 bits.  radius: HOST int array (B,),
    0..7 (checked before the launch).  out must not be image."""
    B, C, H, W = image.shape
    if C != 3:
        raise ValueError("augment_observed: expected a (B,3,H,W) blob, got {}".format(tuple(image.shape)))
    out = out if out is not None else torch.empty_like(image)
    rad = np.ascontiguousarray(np.asarray(radius, dtype=np.int32).reshape(-1))
    if rad.size != B or tuple(on.shape) != (B,) or tuple(taps.shape) != (B, 15) or tuple(chain.shape) != (B, 7) or tuple(seed.shape) != (B,) \
            or tuple(out.shape) != tuple(image.shape):
        raise ValueError("augment_observed: parameters of {} pairs expected: on (B,), radius (B,), taps (B,15), chain (B,7), seed (B,)".format(B))
    keep, mp = host_f32(pixel_means_bgr, 3)
    check(lib().dim_augment_observed(dptr(image, f32), dptr(out, f32), B, H, W, mp, dptr(on, i32), rad.ctypes.data, dptr(taps, f32),
                                     dptr(chain, f32), dptr(seed, i32), int(bool(quantize)), current_stream()))
    return out


VIS_MAX_LAYERS = 8   # dim_vis_overlay: the most layers of one call
VIS_MAX_RADIUS = 3   # ... and the widest outline (2 radius + 1 pixels)


def vis_overlay(image, layers, style, radius, pixel_means_bgr, out=None, counts=None):
    """dim_vis_overlay (csrc/vis.hip; include/deepim_hip.h lists the rules): the outlines of layers (L,B,H,W) f32 (inside where > 0)
    painted in order over the image_observed blob image (B,3,H,W) -> out (B,H,W,3) uint8 B,G,R.  style: HOST ints (L,5) = {B, G, R,
    edge_alpha, fill_alpha}, checked before the launch like radius (0..3).  counts: optional (B,L,2) int32 = {marked, inside} pixels."""
    B, C, H, W = image.shape
    sty = np.ascontiguousarray(np.asarray(style, dtype=np.int32))
    if C != 3 or layers.dim() != 4 or tuple(layers.shape[1:]) != (B, H, W) or sty.shape != (layers.shape[0], 5):
        raise ValueError("vis_overlay: image (B,3,H,W), layers (L,B,H,W) and style (L,5) expected, got {} {} {}".format(
            tuple(image.shape), tuple(layers.shape), sty.shape))
    L = int(layers.shape[0])
    out = out if out is not None else torch.empty((B, H, W, 3), dtype=torch.uint8, device=image.device)
    _same_shape(out, (B, H, W, 3), "out")
    _same_shape(counts, (B, L, 2), "counts")
    keep, mp = host_f32(pixel_means_bgr, 3)
    check(lib().dim_vis_overlay(dptr(image, f32), mp, dptr(layers, f32), L, sty.ctypes.data, int(radius), B, H, W, dptr(out, torch.uint8),
                                dptr(counts, i32), current_stream()))
    return out


FLOW_WEIGHT_ID = {"all": 0, "viz": 1, "valid": 2}


def calc_flow_labels(depth_src, depth_tgt, P12, Kinv_f64, flow, flow_weights=None, thresh=3e-3, standard_rep=False, weight_type="viz"):
    """first-iteration flow labels (calc_flow of lib/pair_matching/flow.py + the weights of get_pair_flow)"""
    B, _, H, W = depth_src.shape
    kinv = np.ascontiguousarray(np.asarray(Kinv_f64, dtype=np.float64).reshape(9))
    check(lib().dim_calc_flow_labels(dptr(depth_src, f32), dptr(depth_tgt, f32), dptr(P12, torch.float64), kinv.ctypes.data, B, H, W, float(thresh),
                                     int(bool(standard_rep)), FLOW_WEIGHT_ID[weight_type], dptr(flow, f32), dptr(flow_weights, f32),
                                     current_stream()))
    return flow, flow_weights


def point_clouds(table, table_off, idx, pose_observed, model, weights, observed):
    B, n = idx.shape
    check(lib().dim_point_clouds(dptr(table, f32), dptr(table_off, i32), dptr(idx, i32), dptr(pose_observed, f32), B, n, dptr(model, f32),
                                 dptr(weights, f32), dptr(observed, f32), current_stream()))


def conv2d_pack_weight(w_oihw, as_bf16=False):
    Cout, Cin, KH, KW = w_oihw.shape
    n = lib().dim_conv2d_packed_weight_floats(Cout, Cin, KH, KW)
    wp = torch.empty((n,), dtype=bf16 if as_bf16 else f32, device=w_oihw.device)
    if as_bf16:
        check(lib().dim_conv2d_pack_weight_bf16(dptr(w_oihw.contiguous(), f32), dptr(wp, bf16), Cout, Cout, Cin, KH, KW, current_stream()))
    else:
        check(lib().dim_conv2d_pack_weight(dptr(w_oihw.contiguous(), f32), dptr(wp, f32), Cout, Cin, KH, KW, current_stream()))
    return wp


def fc_pack_weight(w_out_in, C, H, W):
    Out = w_out_in.shape[0]
    wp = _new((Out * C * H * W,), w_out_in)
    check(lib().dim_fc_pack_weight(dptr(w_out_in.contiguous(), f32), dptr(wp, f32), Out, C, H, W, current_stream()))
    return wp


def conv_out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


TILE_NAMES = {1: "128x128 (4 waves)", 2: "128x64", 3: "64x64", 4: "128x128 (8 waves)"}


def conv_auto_plan(M, Cout, nchunks, cin=32):
    """default (tile, splits) of a direct f32 layer when the caller does not autotune: dim_conv_auto_plan -- the ONE copy of the
    rule, shared with the C resident loop (csrc/refiner.hip)"""
    import ctypes

    tile, splits = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().dim_conv_auto_plan(int(M), int(Cout), int(nchunks), int(cin), ctypes.byref(tile), ctypes.byref(splits)))
    return tile.value, splits.value


def copy(dst, src):
    """dst <- src (same shape, 4-byte dtype, contiguous CUDA tensors) as a kernel launch: graph-safe replacement for Tensor.copy_
    (hipMemcpyAsync nodes inside captured graphs are avoided, see include/deepim_hip.h dim_copy_words)."""
    assert dst.shape == src.shape and dst.dtype == src.dtype and dst.element_size() == 4, (dst.shape, src.shape, dst.dtype, src.dtype)
    check(lib().dim_copy_words(dptr(dst), dptr(src), dst.numel(), current_stream()))
    return dst


def copy_rows(dst, dst_pitch, src, src_pitch, rows, width):
    """dim_copy_rows on two contiguous 4-byte tensors: `rows` runs of `width` words, dst_pitch / src_pitch words apart"""
    assert dst.is_contiguous() and src.is_contiguous() and dst.element_size() == 4 and src.element_size() == 4
    assert (rows - 1) * dst_pitch + width <= dst.numel() and (rows - 1) * src_pitch + width <= src.numel()
    check(lib().dim_copy_rows(dptr(dst), int(dst_pitch), dptr(src), int(src_pitch), int(rows), int(width), current_stream()))
    return dst


def copy_nhwc_channels(dst, dst_c0, src, src_c0, nch, add=False):
    """dst[..., dst_c0:dst_c0+nch] (+)= src[..., src_c0:src_c0+nch] for two contiguous f32 tensors with the same leading dims and their own
    channel counts (NHWC maps, or (B, C) matrices): dim_copy_rows / dim_add_rows with rows = pixels -- the strided copy / add a
    Tensor.copy_ / add_ on a channel slice would hand to a vendor elementwise kernel"""
    assert dst.is_contiguous() and src.is_contiguous() and dst.shape[:-1] == src.shape[:-1], (dst.shape, src.shape)
    Cd, Cs = dst.shape[-1], src.shape[-1]
    assert 0 <= dst_c0 and dst_c0 + nch <= Cd and 0 <= src_c0 and src_c0 + nch <= Cs
    rows = dst.numel() // Cd
    fn = lib().dim_add_rows if add else lib().dim_copy_rows
    check(fn(dptr(dst, f32) + 4 * dst_c0, Cd, dptr(src, f32) + 4 * src_c0, Cs, rows, nch, current_stream()))
    return dst


def fill(dst, value=0.0):
    """dst[...] = value (contiguous f32 / int32 tensor) as a kernel launch (dim_fill_words)"""
    assert dst.is_contiguous() and dst.element_size() == 4
    bits = struct.unpack("<I", struct.pack("<f", float(value)))[0] if dst.dtype == f32 else int(value) & 0xFFFFFFFF
    check(lib().dim_fill_words(dptr(dst), dst.numel(), bits, current_stream()))
    return dst


def copy_channels(dst_oihw, dst_c0, src_oihw, src_c0, nch):
    """dst[:, dst_c0:dst_c0+nch] <- src[:, src_c0:src_c0+nch] for two contiguous (O, I, kh, kw) f32 weights with the same O, kh, kw
    (dim_copy_rows: one run of nch*kh*kw floats per output channel)"""
    O, Id, kh, kw = dst_oihw.shape
    Os, Is = src_oihw.shape[:2]
    assert O == Os and tuple(src_oihw.shape[2:]) == (kh, kw) and dst_oihw.is_contiguous() and src_oihw.is_contiguous()
    assert 0 <= dst_c0 and dst_c0 + nch <= Id and 0 <= src_c0 and src_c0 + nch <= Is
    t = kh * kw
    check(lib().dim_copy_rows(dptr(dst_oihw, f32) + 4 * dst_c0 * t, Id * t, dptr(src_oihw, f32) + 4 * src_c0 * t, Is * t, O, nch * t,
                              current_stream()))
    return dst_oihw


def set_winograd_split(on):
    """arithmetic of the Winograd layers' plane GEMMs: True = f32 operands as three bf16 terms, six MFMA products (default);
    False = the f32 matrix pipe.  Read when a layer is next planned (launch / graph capture)."""
    check(lib().dim_set_winograd_split(1 if on else 0))


def get_winograd_split():
    return bool(lib().dim_get_winograd_split())


def winograd_plane_gemm(V, U_pkn, T, K, Cout, P, tile, out=None):
    """the plane GEMM of the Winograd layers on its own (dim_winograd_plane_gemm): M[t][p] = V[t][p] . U_pkn[p] for V (T, P, K) and
    U_pkn (P, K, Cout), in the arithmetic set_winograd_split selects.  Returns (M (T, P, Cout), used_split); `out`: M to write into."""
    import ctypes

    assert tuple(V.shape) == (T, P, K) and tuple(U_pkn.shape) == (P, K, Cout) and K % 32 == 0, (V.shape, U_pkn.shape)
    n = P * K * Cout
    wp = _new((lib().dim_winograd_plane_gemm_weight_floats(K, Cout, P),), V)
    wp[:n] = U_pkn.reshape(P, K // 32, 32, Cout).permute(0, 1, 3, 2).reshape(-1)      # -> the chunk layout [P][K/32][Cout][32]
    check(lib().dim_winograd_plane_gemm_split_weights(dptr(wp, f32), K, Cout, P, current_stream()))
    out = out if out is not None else _new((T, P, Cout), V)
    used = ctypes.c_int(-1)
    check(lib().dim_winograd_plane_gemm(dptr(V, f32), dptr(wp, f32), dptr(out, f32), T, K, Cout, P, int(tile), ctypes.byref(used),
                                        current_stream()))
    return out, used.value


def winograd_pack_weight(w_oihw, m=2):
    """(Cout,Cin,3,3) -> the (m+2)^2 transformed 1x1 weight sets of the Winograd F(m x m, 3x3) path, m = 2 or 4"""
    Cout, Cin, KH, KW = w_oihw.shape
    assert KH == 3 and KW == 3
    out = _new((lib().dim_winograd_packed_weight_floats(Cout, Cin, m),), w_oihw)
    check(lib().dim_winograd_pack_weight(dptr(w_oihw, f32), dptr(out, f32), Cout, Cin, m, current_stream()))
    return out


def winograd_dgrad_pack_weight(w_oihw, m=2):
    """the transformed weights of the layer's INPUT gradient from its forward (Cout,Cin,3,3) array: the same array
    winograd_pack_weight(w.flip(2, 3).transpose(0, 1)) gives, without the flipped copy"""
    Cout, Cin, KH, KW = w_oihw.shape
    assert KH == 3 and KW == 3 and w_oihw.is_contiguous()
    out = _new((lib().dim_winograd_packed_weight_floats(Cin, Cout, m),), w_oihw)
    check(lib().dim_winograd_dgrad_pack_weight(dptr(w_oihw, f32), dptr(out, f32), Cout, Cin, m, current_stream()))
    return out


def _wino_events(events):
    import ctypes

    if events is None:
        return None, None
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in evs:
        e.record()  # materialises the hipEvent_t behind the torch object
    return (ctypes.c_void_p * 4)(*[e.cuda_event for e in evs]), evs


def _winograd_fwd(entry, workspace_floats, out_hw, x_nhwc, Cin, w_packed, bias, Cout, slope, tile, out, out_coff, workspace, events, *tail):
    """the three forward Winograd wrappers: `entry` into `out` ((N,) + out_hw + (Cout,) when not given) through `workspace` (a new one
    when none or a smaller one than workspace_floats(...) is given).  tail: what entry takes between tile and events4, and
    workspace_floats after Cout (the m of the stride-1 path)"""
    N, H, W, in_cs = x_nhwc.shape
    out = out if out is not None else _new((N,) + out_hw + (Cout,), x_nhwc)
    need = workspace_floats(N, H, W, Cin, Cout, *tail)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), x_nhwc)
    ev_arr, evs = _wino_events(events)
    check(entry(dptr(x_nhwc, f32), dptr(w_packed, f32), dptr(bias, f32), dptr(out, f32), dptr(workspace, f32), N, H, W, Cin, in_cs, Cout,
                out.shape[-1], out_coff, float(slope), tile, *tail, ev_arr, current_stream()))
    if events is not None:
        events.extend([("wino_in", evs[0], evs[1]), ("conv", evs[1], evs[2]), ("wino_out", evs[2], evs[3])])
    return out


def conv2d_fwd_winograd(x_nhwc, Cin, w_packed, bias, Cout, slope=0.1, tile=0, out=None, out_coff=0, workspace=None, events=None, m=2):
    """3x3 / stride 1 / pad 1 convolution through Winograd F(m x m, 3x3) (m = 2 or 4, the m the weights were packed with);
    x may carry padded channels (in_cstride = x.shape[-1]).
    events: optional list; ("wino_in" | "conv" | "wino_out", start, end) HIP-event triples of the three launches are appended."""
    H, W = x_nhwc.shape[1:3]
    return _winograd_fwd(lib().dim_conv2d_fwd_winograd, lib().dim_winograd_workspace_floats, (H, W), x_nhwc, Cin, w_packed, bias, Cout, slope,
                         tile, out, out_coff, workspace, events, m)


def winograd3x3s2_pack_weight(w_oihw):
    """(Cout,Cin,3,3) of a stride-2 / pad-1 layer -> the 81 transformed weight sets of dim_conv2d_fwd_winograd3x3s2"""
    Cout, Cin, KH, KW = w_oihw.shape
    assert KH == 3 and KW == 3
    out = _new((lib().dim_winograd3x3s2_packed_weight_floats(Cout, Cin),), w_oihw)
    check(lib().dim_winograd3x3s2_pack_weight(dptr(w_oihw.contiguous(), f32), dptr(out, f32), Cout, Cin, current_stream()))
    return out


def conv2d_fwd_winograd3x3s2(x_nhwc, Cin, w_packed, bias, Cout, slope=0.1, tile=0, out=None, out_coff=0, workspace=None, events=None):
    """y = LeakyReLU(conv 3x3 / stride 2 / pad 1 + bias) through the phase-image Winograd path (81 plane GEMMs); x (N,H,W,>=Cin) NHWC.
    events: as conv2d_fwd_winograd."""
    H, W = x_nhwc.shape[1:3]
    return _winograd_fwd(lib().dim_conv2d_fwd_winograd3x3s2, lib().dim_winograd3x3s2_workspace_floats, ((H - 1) // 2 + 1, (W - 1) // 2 + 1),
                         x_nhwc, Cin, w_packed, bias, Cout, slope, tile, out, out_coff, workspace, events)


def winograd5x5s2_pack_weight(w_oihw):
    """(Cout,Cin,5,5) of a stride-2 / pad-2 layer -> the 36 transformed weight sets (K = 4 Cin) of dim_conv2d_fwd_winograd5x5s2"""
    Cout, Cin, KH, KW = w_oihw.shape
    assert KH == 5 and KW == 5
    out = _new((lib().dim_winograd5x5s2_packed_weight_floats(Cout, Cin),), w_oihw)
    check(lib().dim_winograd5x5s2_pack_weight(dptr(w_oihw, f32), dptr(out, f32), Cout, Cin, current_stream()))
    return out


def winograd5x5s2_dgrad_pack_weight(w_oihw):
    """(Cout,Cin,5,5) -> the 36 transformed weight sets (K = Cout, N = 4 Cin) of dim_conv2d_dgrad_winograd5x5s2"""
    Cout, Cin, KH, KW = w_oihw.shape
    assert KH == 5 and KW == 5
    out = _new((lib().dim_winograd5x5s2_packed_weight_floats(Cout, Cin),), w_oihw)
    check(lib().dim_winograd5x5s2_dgrad_pack_weight(dptr(w_oihw, f32), dptr(out, f32), Cout, Cin, current_stream()))
    return out


def conv2d_dgrad_winograd5x5s2(dy_nhwc, Cout, w_packed, dx_nhwc, Cin, tile=0, workspace=None):
    """dx (N,H,W,>=Cin) = input gradient of the 5x5 / stride 2 / pad 2 convolution, from dy (N,ceil(H/2),ceil(W/2),>=Cout); overwrites dx"""
    N, H, W, dx_cs = dx_nhwc.shape
    assert dy_nhwc.shape[:3] == (N, (H + 1) // 2, (W + 1) // 2)
    need = lib().dim_winograd5x5s2_workspace_floats(N, H, W, Cin, Cout)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), dx_nhwc)
    check(lib().dim_conv2d_dgrad_winograd5x5s2(dptr(dy_nhwc, f32), dptr(w_packed, f32), dptr(dx_nhwc, f32), dptr(workspace, f32), N, H, W, Cin,
                                               dx_cs, Cout, dy_nhwc.shape[-1], tile, current_stream()))
    return dx_nhwc


def conv2d_wgrad_winograd(x_nhwc, Cin, dy_nhwc, Cout, dw_oihw, S=1, splits=4, workspace=None, scale=1.0, accumulate=False):
    """dw (Cout,Cin,k,k) (+)= scale * weight gradient through Winograd; S = 1: 3x3 / stride 1 / pad 1, S = 2: 5x5 / stride 2 / pad 2"""
    N, H, W, in_cs = x_nhwc.shape
    k = 3 if S == 1 else 5
    assert tuple(dw_oihw.shape) == (Cout, Cin, k, k) and dw_oihw.is_contiguous()
    need = lib().dim_conv2d_wgrad_winograd_workspace_floats(N, H, W, Cin, Cout, S, splits)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), x_nhwc)
    check(lib().dim_conv2d_wgrad_winograd(dptr(x_nhwc, f32), dptr(dy_nhwc, f32), dptr(dw_oihw, f32), dptr(workspace, f32), N, H, W, Cin, in_cs,
                                          Cout, dy_nhwc.shape[-1], S, splits, float(scale), int(accumulate), current_stream()))
    return dw_oihw


def fc_fwd(x_nhwc, w_packed, bias, Out, slope=0.1, out=None, workspace=None, events=None):
    """y (B,Out) = LeakyReLU(flatten(x) . W^T + b) as a weight stream (dim_fc_fwd); w_packed from fc_pack_weight.
    events: optional list; one ("fc", start, end, 2) HIP-event tuple around the stream + reduce launches is appended."""
    B, H, W, C = x_nhwc.shape
    assert x_nhwc.is_contiguous()
    out = out if out is not None else _new((B, Out), x_nhwc)
    need = lib().dim_fc_fwd_workspace_floats(C, H, W, Out)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), x_nhwc)
    evs = None
    if events is not None:
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        evs[0].record()
    check(lib().dim_fc_fwd(dptr(x_nhwc, f32), dptr(w_packed, f32), dptr(bias, f32), dptr(out, f32), dptr(workspace, f32), B, C, H, W, Out,
                           float(slope), current_stream()))
    if events is not None:
        evs[1].record()
        events.append(("fc", evs[0], evs[1], 2))
    return out


WINO_ITEM_MAP_HEADER = ("T", "K", "Cout", "tile", "G", "per", "rem", "live_max_before", "live_max_after", "moved", "items", "nch")


def _wino_item_map_read(query):
    """header dict and table (items,) int32 of an item map; query(header_ptr, table_ptr, capacity) is one of the two C queries"""
    hdr = np.zeros(len(WINO_ITEM_MAP_HEADER), dtype=np.int32)
    check(query(hdr.ctypes.data, None, 0))
    table = np.zeros(int(hdr[WINO_ITEM_MAP_HEADER.index("items")]), dtype=np.int32)
    check(query(hdr.ctypes.data, table.ctypes.data, table.size))
    return dict(zip(WINO_ITEM_MAP_HEADER, (int(v) for v in hdr))), table


def wino_item_map_plan(T, K, Cout, tile, G=0, skip5=True):
    """the item-slot table dim_wino_item_map_create would build for the plane GEMMs [T x K] . [K x Cout] x 36 on `tile` cut into G ranges
    (0: the G of a launch on this device), without a device: (header dict, table).  Host arithmetic only when G is given."""
    return _wino_item_map_read(lambda h, t, n: lib().dim_wino_item_map_plan(int(T), int(K), int(Cout), int(tile), int(G), int(skip5), h, t, n))


class WinoItemMap(object):
    """a 5x5 / stride-2 layer's item-slot table in device memory (dim_wino_item_map_create); lives as long as this object"""

    def __init__(self, N, H, W, Cin, Cout, tile=0):
        import ctypes

        self._destroy, handle = lib().dim_wino_item_map_destroy, ctypes.c_void_p()
        check(lib().dim_wino_item_map_create(ctypes.byref(handle), int(N), int(H), int(W), int(Cin), int(Cout), int(tile)))
        self.handle = handle.value

    def query(self):
        return _wino_item_map_read(lambda h, t, n: lib().dim_wino_item_map_query(self.handle, h, t, n))

    def __del__(self):
        if getattr(self, "handle", None):
            self._destroy(self.handle)
            self.handle = None


def wino_item_map_create(N, H, W, Cin, Cout, tile=0):
    """plan step of a 5x5 / stride-2 layer with input (N,H,W,Cin): its WinoItemMap.  Allocates and copies: never under graph capture."""
    return WinoItemMap(N, H, W, Cin, Cout, tile)


def conv2d_fwd_winograd5x5s2(x_nhwc, Cin, w_packed, bias, Cout, slope=0.1, tile=0, out=None, out_coff=0, workspace=None, events=None,
                             item_map=None):
    """5x5 / stride 2 / pad 2 convolution as four phase images through Winograd F(4x4,3x3) (see include/deepim_hip.h).
    item_map: the layer's WinoItemMap; when not given, the one its planner left on the packed weights (`w_packed.item_map`), else
    none.  A map built for another plan is ignored by the library: same bits either way."""
    H, W = x_nhwc.shape[1:3]
    item_map = item_map if item_map is not None else getattr(w_packed, "item_map", None)
    if item_map is None:
        return _winograd_fwd(lib().dim_conv2d_fwd_winograd5x5s2, lib().dim_winograd5x5s2_workspace_floats, ((H + 1) // 2, (W + 1) // 2),
                             x_nhwc, Cin, w_packed, bias, Cout, slope, tile, out, out_coff, workspace, events)
    return _winograd_fwd(lib().dim_conv2d_fwd_winograd5x5s2_map, lambda *a: lib().dim_winograd5x5s2_workspace_floats(*a[:5]),
                         ((H + 1) // 2, (W + 1) // 2), x_nhwc, Cin, w_packed, bias, Cout, slope, tile, out, out_coff, workspace, events,
                         item_map.handle)


def conv2d_fwd(x_nhwc, w_packed, bias, Cout, KH, KW, stride, pad, slope=0.1, splits=1, tile=0, out=None, workspace=None,
               events=None):
    """splits: 1 = one launch; > 1 = split-K through `workspace`; 0 = auto (whole tiles per CU in one launch, the remaining tiles
    as a split-K launch + reduce; needs `workspace`, see dim_conv2d_fwd / dim_conv2d_tail_plan).
    events: optional list; when given, (kernel_tag, start_event, end_event) tuples are appended with HIP events recorded on the
    launch stream around the conv kernel and (split-K) around the reduce kernel separately (auto mode: one tuple for everything,
    tag "conv", with a 4th element = number of conv-kernel launches inside)."""
    N, H, W, Cin = x_nhwc.shape
    Ho, Wo = conv_out_hw(H, W, KH, KW, stride, pad)
    out = out if out is not None else _new((N, Ho, Wo, Cout), x_nhwc)
    if splits != 1 and workspace is None:
        workspace = _new((lib().dim_conv2d_workspace_floats(N, H, W, Cin, Cout, KH, KW, stride, pad, splits),), x_nhwc)
    if events is not None:
        def ev():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e
        e0 = ev()
        if splits > 1 and w_packed.dtype != bf16:
            check(lib().dim_conv2d_fwd_partial(dptr(x_nhwc, f32), dptr(w_packed, f32), dptr(workspace, f32), N, H, W, Cin, Cout, KH, KW,
                                               stride, pad, splits, tile, current_stream()))
            e1 = ev()
            check(lib().dim_splitk_reduce(dptr(workspace, f32), dptr(bias, f32), dptr(out, f32), N * Ho * Wo, Cout, splits, float(slope),
                                          current_stream()))
            e2 = ev()
            events += [("conv", e0, e1), ("reduce", e1, e2)]
        else:
            wp, is16 = _wp(w_packed)
            check((lib().dim_conv2d_fwd_bf16 if is16 else lib().dim_conv2d_fwd)(dptr(x_nhwc, f32), wp, dptr(bias, f32), dptr(out, f32),
                                                                                 dptr(workspace, f32), N, H, W, Cin, Cout, KH, KW, stride, pad,
                                                                                 float(slope), splits, tile, current_stream()))
            n_launch = 1
            if splits == 0:
                import ctypes

                tb, ts = ctypes.c_int(0), ctypes.c_int(1)
                check(lib().dim_conv2d_tail_plan(N * Ho * Wo, Cout, Cin, KH, KW, tile, ctypes.byref(tb), ctypes.byref(ts)))
                n_launch = 2 if ts.value >= 2 else 1
            events.append(("conv", e0, ev(), n_launch))
        return out
    wp, is16 = _wp(w_packed)
    fn = lib().dim_conv2d_fwd_bf16 if is16 else lib().dim_conv2d_fwd
    check(fn(dptr(x_nhwc, f32), wp, dptr(bias, f32), dptr(out, f32), dptr(workspace, f32), N, H, W,
             Cin, Cout, KH, KW, stride, pad, float(slope), splits, tile, current_stream()))
    return out


def pose_head_fwd(fc6, p, zf, se3=None, fc7_out=None):
    """p: dict with fc7_weight/bias, rot_weight/bias, trans_weight/bias (reference (out,in) layout)."""
    B = fc6.shape[0]
    se3 = se3 if se3 is not None else _new((B, 7), fc6)
    check(lib().dim_pose_head_fwd(dptr(fc6, f32), dptr(p["fc7_weight"], f32), dptr(p["fc7_bias"], f32), dptr(p["rot_weight"], f32),
                                  dptr(p["rot_bias"], f32), dptr(p["trans_weight"], f32), dptr(p["trans_bias"], f32), dptr(zf, f32),
                                  dptr(se3, f32), dptr(fc7_out, f32), B, current_stream()))
    return se3


def _cls_arg(class_index, B, K):
    if class_index is None:
        if K > 1:
            raise ValueError("{} per-class pose heads need the batch's class_index".format(K))
        return None
    assert class_index.numel() == B, (class_index.numel(), B)
    return dptr(class_index, i32)


def pose_head_fwd_cls(fc6, p, class_index, n_regressors, zf, se3=None, fc7_out=None, status=None):
    """dim_pose_head_fwd_cls: pose_head_fwd with one rot / trans head per class (p: rot (4K,256) / (4K), trans (3K,256) / (3K)); sample
    b reads the rows of class_index[b] ((B,) int32; None allowed with n_regressors 1).  DIM_STATUS_BAD_CLASS is OR-ed into status (B,)
    int32 when given, for a class outside [0, K) (identity delta)."""
    B, K = fc6.shape[0], int(n_regressors)
    se3 = se3 if se3 is not None else _new((B, 7), fc6)
    assert status is None or status.numel() == B
    check(lib().dim_pose_head_fwd_cls(dptr(fc6, f32), dptr(p["fc7_weight"], f32), dptr(p["fc7_bias"], f32), dptr(p["rot_weight"], f32),
                                      dptr(p["rot_bias"], f32), dptr(p["trans_weight"], f32), dptr(p["trans_bias"], f32),
                                      _cls_arg(class_index, B, K), K, dptr(zf, f32), dptr(se3, f32), dptr(fc7_out, f32), _opt(status, i32),
                                      B, current_stream()))
    return se3


# ---------------------------------------------------------------- decoder pieces (deepIM_flownet.py:213-299, :315-340, :502-529)
def pad32(c):
    return (c + 31) // 32 * 32


def _new_packed(n, like, as_bf16):
    return torch.empty((n,), dtype=bf16 if as_bf16 else f32, device=like.device)


def deconv4x4s2_pack_weight(w_iohw, as_bf16=False):
    """as_bf16: the bf16 image of the packed array in one pass (== to_bf16 of the f32 result); same for the packers below"""
    Cin, Cout = w_iohw.shape[:2]
    wp = _new_packed(lib().dim_deconv4x4s2_packed_weight_floats(Cin, Cout), w_iohw, as_bf16)
    if as_bf16:
        check(lib().dim_deconv4x4s2_pack_weight_bf16(dptr(w_iohw.contiguous(), f32), dptr(wp, bf16), Cin, Cout, current_stream()))
    else:
        check(lib().dim_deconv4x4s2_pack_weight(dptr(w_iohw.contiguous(), f32), dptr(wp, f32), Cin, Cout, current_stream()))
    return wp


def deconv4x4s2_fwd(x_nhwc, Cin, w_packed, bias, y_nhwc, Cout, crop, slope, out_coff=0, tile=3):
    """y[..., out_coff:out_coff+Cout] = LeakyReLU(Crop(Deconvolution(x[..., :Cin]) + bias)); y's H,W define the crop window."""
    N, H, W, in_cs = x_nhwc.shape
    _, OH, OW, out_cs = y_nhwc.shape
    wp, is16 = _wp(w_packed)
    fn = lib().dim_deconv4x4s2_fwd_bf16 if is16 else lib().dim_deconv4x4s2_fwd
    check(fn(dptr(x_nhwc, f32), wp, dptr(bias, f32), dptr(y_nhwc, f32), N, H, W, Cin, in_cs, Cout,
             OH, OW, crop, float(slope), out_cs, out_coff, tile, current_stream()))
    return y_nhwc


def deconv4x4s2_tiny_fwd(x_nhwc, Cin, w_iohw, bias, y_nhwc, Cout, crop, out_coff=0):
    N, H, W, in_cs = x_nhwc.shape
    _, OH, OW, out_cs = y_nhwc.shape
    check(lib().dim_deconv4x4s2_tiny_fwd(dptr(x_nhwc, f32), dptr(w_iohw, f32), dptr(bias, f32), dptr(y_nhwc, f32), N, H, W, Cin, in_cs,
                                         Cout, OH, OW, crop, out_cs, out_coff, current_stream()))
    return y_nhwc


def conv_small_cout_pack_weight(w_oihw):
    Cout, Cin, KH, KW = w_oihw.shape
    wp = _new((Cout * KH * KW * pad32(Cin),), w_oihw)
    check(lib().dim_conv_small_cout_pack_weight(dptr(w_oihw.contiguous(), f32), dptr(wp, f32), Cout, Cin, KH, KW, current_stream()))
    return wp


def conv_small_cout_fwd(x_nhwc, Cin, w_packed, bias, Cout, KH=3, KW=3, pad=1, out=None, out_coff=0):
    N, H, W, in_cs = x_nhwc.shape
    out = out if out is not None else _new((N, H, W, Cout), x_nhwc)
    check(lib().dim_conv_small_cout_fwd(dptr(x_nhwc, f32), dptr(w_packed, f32), dptr(bias, f32), dptr(out, f32), N, H, W, Cin, in_cs, Cout,
                                        KH, KW, pad, out.shape[3], out_coff, current_stream()))
    return out


def upsample16_fwd(x_nhwc, w_c1_32_32, OH, OW, crop=8, scale=1.0, sigmoid=False, out=None):
    N, h, w, C = x_nhwc.shape
    out = out if out is not None else _new((N, C, OH, OW), x_nhwc)
    check(lib().dim_upsample16_fwd(dptr(x_nhwc, f32), dptr(w_c1_32_32, f32), dptr(out, f32), N, C, h, w, OH, OW, crop, float(scale),
                                   1 if sigmoid else 0, current_stream()))
    return out


# ---------------------------------------------------------------- backward of the convolution stack
def pad64(c):
    return (c + 63) // 64 * 64


def conv2d_dgrad_pack_weight(w_oihw, stride, pad, as_bf16=False):
    Cout, Cin, KH, KW = w_oihw.shape
    wp = _new_packed(lib().dim_conv2d_dgrad_packed_weight_floats(Cout, Cin, KH, KW, stride, pad), w_oihw, as_bf16)
    if as_bf16:
        check(lib().dim_conv2d_dgrad_pack_weight_bf16(dptr(w_oihw.contiguous(), f32), dptr(wp, bf16), Cout, Cin, KH, KW, stride, pad,
                                                      current_stream()))
    else:
        check(lib().dim_conv2d_dgrad_pack_weight(dptr(w_oihw.contiguous(), f32), dptr(wp, f32), Cout, Cin, KH, KW, stride, pad, current_stream()))
    return wp


def conv2d_dgrad_lrelu(dy_nhwc, Cout, w_dgrad_packed_bf16, dz_nhwc, y_act_nhwc, Cin, KH, KW, stride, pad, db, slope=0.1, workspace=None,
                       accumulate_db=False):
    """dz = dgrad(dy) * LeakyReLU'(y_act), db (+)= column sums of dz -- the lower layer's activation gradient pass folded into this
    layer's input gradient (dim_conv2d_dgrad_bf16_lrelu: bf16 patch kernel only).  dz, y_act: dense (N, H, W, Cin)."""
    N, Ho, Wo, dy_cs = dy_nhwc.shape
    _, H, W, dx_cs = dz_nhwc.shape
    assert w_dgrad_packed_bf16.dtype == bf16 and tuple(y_act_nhwc.shape) == tuple(dz_nhwc.shape) == (N, H, W, Cin)
    assert dz_nhwc.is_contiguous() and y_act_nhwc.is_contiguous() and db.numel() == Cin
    need = lib().dim_conv2d_dgrad_lrelu_workspace_floats(N, H, W, Cin, stride)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), dz_nhwc)
    check(lib().dim_conv2d_dgrad_bf16_lrelu(dptr(dy_nhwc, f32), dptr(w_dgrad_packed_bf16, bf16), dptr(dz_nhwc, f32), dptr(y_act_nhwc, f32),
                                            float(slope), dptr(db, f32), dptr(workspace, f32), N, H, W, Cin, dx_cs, Ho, Wo, Cout, dy_cs, KH, KW,
                                            stride, pad, int(accumulate_db), current_stream()))
    return dz_nhwc


def conv2d_dgrad(dy_nhwc, Cout, w_dgrad_packed, dx_nhwc, Cin, KH, KW, stride, pad, accumulate=False, tile=3, splits=1, workspace=None):
    """dx[..., :Cin] (+)= dgrad(dy[..., :Cout]); dx / dy may be wider concat buffers.
    splits > 1 (bf16 weights, tile 3 / 4): split-K through output-shaped slabs in `workspace` (small maps: too few tiles for the chip)"""
    N, Ho, Wo, dy_cs = dy_nhwc.shape
    _, H, W, dx_cs = dx_nhwc.shape
    wp, is16 = _wp(w_dgrad_packed)
    if splits > 1:
        assert is16, "split-K input gradient is built for the bf16 kernels"
        need = lib().dim_conv2d_dgrad_splitk_workspace_floats(N, H, W, dx_cs, splits)
        if workspace is None or workspace.numel() < need:
            workspace = _new((need,), dx_nhwc)
        check(lib().dim_conv2d_dgrad_bf16_splitk(dptr(dy_nhwc, f32), wp, dptr(dx_nhwc, f32), dptr(workspace, f32), N, H, W, Cin, dx_cs, Ho, Wo,
                                                 Cout, dy_cs, KH, KW, stride, pad, int(accumulate), tile, splits, current_stream()))
        return dx_nhwc
    fn = lib().dim_conv2d_dgrad_bf16 if is16 else lib().dim_conv2d_dgrad
    check(fn(dptr(dy_nhwc, f32), wp, dptr(dx_nhwc, f32), N, H, W, Cin, dx_cs, Ho, Wo, Cout, dy_cs,
             KH, KW, stride, pad, int(accumulate), tile, current_stream()))
    return dx_nhwc


def conv2d_wgrad(x_nhwc, Cin, dz_nhwc, Cout, KH, KW, stride, pad, dw_packed, splits=1, dz_coff=0, workspace=None, accumulate=False,
                 bf16_mfma=False):
    """bf16_mfma: products on the bf16 matrix pipe (operands rounded on the way into LDS; f32 accumulate, f32 result)"""
    N, H, W, in_cs = x_nhwc.shape
    _, Ho, Wo, dz_cs = dz_nhwc.shape
    if splits > 1 and workspace is None:
        workspace = _new((lib().dim_conv2d_wgrad_workspace_floats(Cout, Cin, KH, KW, splits),), x_nhwc)
    check((lib().dim_conv2d_wgrad_bf16 if bf16_mfma else lib().dim_conv2d_wgrad)(dptr(x_nhwc, f32), dptr(dz_nhwc, f32), dptr(dw_packed, f32), dptr(workspace, f32), N, H, W, Cin, in_cs, Ho,
                                 Wo, Cout, dz_cs, dz_coff, KH, KW, stride, pad, splits, int(accumulate), current_stream()))
    return dw_packed


def conv2d_wgrad_oihw(x_nhwc, Cin, dz_nhwc, Cout, KH, KW, stride, pad, dw_oihw, splits=1, dz_coff=0, workspace=None, bf16_mfma=False,
                      scale=1.0, accumulate=False):
    """dw_oihw (rows <= Cout, Cin, KH, KW) (+)= scale * weight gradient, slabs summed inside the layout converter (dim_conv2d_wgrad_oihw)"""
    N, H, W, in_cs = x_nhwc.shape
    _, Ho, Wo, dz_cs = dz_nhwc.shape
    assert dw_oihw.is_contiguous() and tuple(dw_oihw.shape[1:]) == (Cin, KH, KW) and dw_oihw.shape[0] <= Cout
    need = lib().dim_conv2d_wgrad_workspace_floats(Cout, Cin, KH, KW, max(int(splits), 1) + 1)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), x_nhwc)
    check(lib().dim_conv2d_wgrad_oihw(dptr(x_nhwc, f32), dptr(dz_nhwc, f32), dptr(dw_oihw, f32), dptr(workspace, f32), N, H, W, Cin, in_cs, Ho, Wo,
                                      Cout, dz_cs, dz_coff, KH, KW, stride, pad, int(splits), int(bool(bf16_mfma)), dw_oihw.shape[0],
                                      float(scale), int(accumulate), current_stream()))
    return dw_oihw


def bias_grad(dz_nhwc, C, db, dz_coff=0, workspace=None, accumulate=False):
    M = dz_nhwc.numel() // dz_nhwc.shape[-1]
    if workspace is None:
        workspace = _new((lib().dim_bias_grad_workspace_floats(M, C),), dz_nhwc)
    check(lib().dim_bias_grad(dptr(dz_nhwc, f32), dptr(db, f32), dptr(workspace, f32), M, C, dz_nhwc.shape[-1], dz_coff, int(accumulate),
                              current_stream()))
    return db


def lrelu_bwd(y_nhwc, dy_nhwc, C, slope=0.1, y_coff=0, dy_coff=0):
    M = dy_nhwc.numel() // dy_nhwc.shape[-1]
    check(lib().dim_lrelu_bwd(dptr(y_nhwc, f32), y_nhwc.shape[-1], y_coff, dptr(dy_nhwc, f32), dy_nhwc.shape[-1], dy_coff, M, C, float(slope),
                              current_stream()))
    return dy_nhwc


def lrelu_bwd_bias_grad(y_nhwc, dy_nhwc, C, db, slope=0.1, y_coff=0, dy_coff=0, workspace=None, accumulate=False):
    """dy[..., dy_coff:dy_coff+C] *= LeakyReLU'(y[..., y_coff:y_coff+C]) in place and db (+)= its column sums, one pass (dim_lrelu_bwd_bias_grad)"""
    M = dy_nhwc.numel() // dy_nhwc.shape[-1]
    need = lib().dim_lrelu_bwd_bias_grad_workspace_floats(M, C)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), dy_nhwc)
    check(lib().dim_lrelu_bwd_bias_grad(dptr(y_nhwc, f32), y_nhwc.shape[-1], y_coff, dptr(dy_nhwc, f32), dy_nhwc.shape[-1], dy_coff, dptr(db, f32),
                                        dptr(workspace, f32), M, C, float(slope), int(accumulate), current_stream()))
    return dy_nhwc


# ---------------------------------------------------------------- training-only pieces (csrc/train.hip)
def _p(t, off=0):
    """device pointer of a contiguous CUDA f32 tensor, advanced by `off` floats (channel offset inside an NHWC row)"""
    return dptr(t, f32) + 4 * off


def conv2d_pack_weight_padded(w_oihw, CoutPad, as_bf16=False):
    Cout, Cin, KH, KW = w_oihw.shape
    wp = _new_packed(KH * KW * Cin * CoutPad, w_oihw, as_bf16)
    if as_bf16:
        check(lib().dim_conv2d_pack_weight_bf16(dptr(w_oihw.contiguous(), f32), dptr(wp, bf16), Cout, CoutPad, Cin, KH, KW, current_stream()))
    else:
        check(lib().dim_conv2d_pack_weight_padded(dptr(w_oihw.contiguous(), f32), dptr(wp, f32), Cout, CoutPad, Cin, KH, KW, current_stream()))
    return wp


def conv2d_unpack_weight(w_packed, out_oihw, CoutPad=None, scale=1.0, accumulate=False):
    Cout, Cin, KH, KW = out_oihw.shape
    check(lib().dim_conv2d_unpack_weight(dptr(w_packed, f32), dptr(out_oihw, f32), Cout, CoutPad or Cout, Cin, KH, KW, float(scale),
                                         int(accumulate), current_stream()))
    return out_oihw


def fc_unpack_weight(w_packed, out_w, C, H, W):
    check(lib().dim_fc_unpack_weight(dptr(w_packed, f32), dptr(out_w, f32), out_w.shape[0], C, H, W, current_stream()))
    return out_w


def fc_wgrad_nhwc(dz, x_nhwc, dW):
    """dW (Out, C*H*W in MXNet's (c, h, w) order) = dz (B, Out)^T . x (B, H, W, C); B <= 32 (dim_fc_wgrad_nhwc)"""
    B, H, W, C = x_nhwc.shape
    Out = dW.shape[0]
    assert x_nhwc.is_contiguous() and dW.is_contiguous() and dW.numel() == Out * C * H * W and dz.numel() == B * Out
    check(lib().dim_fc_wgrad_nhwc(dptr(dz, f32), dptr(x_nhwc, f32), dptr(dW, f32), B, Out, C, H, W, current_stream()))
    return dW


def fc_dgrad_pack_weight(w_out_in, C, H, W, out=None, as_bf16=False):
    Out = w_out_in.shape[0]
    out = out if out is not None else _new_packed(Out * C * H * W, w_out_in, as_bf16)
    if as_bf16:
        check(lib().dim_fc_dgrad_pack_weight_bf16(dptr(w_out_in, f32), dptr(out, bf16), Out, C, H, W, current_stream()))
    else:
        check(lib().dim_fc_dgrad_pack_weight(dptr(w_out_in, f32), dptr(out, f32), Out, C, H, W, current_stream()))
    return out


def conv2d_fwd_ex(x, x_coff, Cin, w_packed, bias, y, y_coff, Cout, KH, KW, stride, pad, slope=1.0, tile=3, Ho=0, Wo=0, accumulate=False):
    """dense generalised conv: channel windows [x_coff, x_coff+Cin) of x and [y_coff, y_coff+Cout) of y (NHWC concat buffers)."""
    N, H, W, in_cs = x.shape
    out_cs = y.shape[-1]
    wp, is16 = _wp(w_packed)
    fn = lib().dim_conv2d_fwd_ex_bf16 if is16 else lib().dim_conv2d_fwd_ex
    check(fn(_p(x, x_coff), wp, dptr(bias, f32), dptr(y, f32), N, H, W, Cin, in_cs, Cout, KH, KW, stride,
             pad, float(slope), tile, out_cs, y_coff, 0, 0, 0, 0, 0, 0, Ho, Wo, -1, int(accumulate), current_stream()))
    return y


def conv2d_wgrad_ex(x, x_coff, Cin, dz, dz_coff, Cout, KH, KW, stride, pad, dw_packed, splits=1, workspace=None, bf16_mfma=False):
    N, H, W, in_cs = x.shape
    _, Ho, Wo, dz_cs = dz.shape
    if splits > 1 and workspace is None:
        workspace = _new((lib().dim_conv2d_wgrad_workspace_floats(Cout, Cin, KH, KW, splits),), x)
    check((lib().dim_conv2d_wgrad_bf16 if bf16_mfma else lib().dim_conv2d_wgrad)(_p(x, x_coff), dptr(dz, f32), dptr(dw_packed, f32), dptr(workspace, f32), N, H, W, Cin, in_cs, Ho, Wo, Cout,
                                 dz_cs, dz_coff, KH, KW, stride, pad, splits, 0, current_stream()))
    return dw_packed


def flow_loss_grad(flow_est, flow_label, flow_weights, grad, normalize_flow, grad_scale, loss_sum=None):
    check(lib().dim_flow_loss_grad(dptr(flow_est, f32), dptr(flow_label, f32), dptr(flow_weights, f32), dptr(grad, f32), flow_est.numel(),
                                   float(normalize_flow), float(grad_scale), dptr(loss_sum, f32), current_stream()))
    return grad


def logistic_grad(logits, label, grad, grad_scale_over_num_output, prob=None):
    check(lib().dim_logistic_grad(dptr(logits, f32), dptr(label, f32), dptr(grad, f32), dptr(prob, f32), logits.numel(),
                                  float(grad_scale_over_num_output), current_stream()))
    return grad


def pm_l1_grad(p_est, p_obs, weights, grad, norm_term, grad_scale, loss_sum=None):
    check(lib().dim_pm_l1_grad(dptr(p_est, f32), dptr(p_obs, f32), dptr(weights, f32), dptr(grad, f32), p_est.numel(), float(norm_term),
                               float(grad_scale), dptr(loss_sum, f32), current_stream()))
    return grad


LOSS_TYPE_ID = {"L1": 0, "L2": 1, "smooth_L1": 2}


def pm_loss_grad(p_est, p_obs, weights, grad, norm_term, grad_scale, loss_type="L1", smooth_l1_scalar=1.0, loss_sum=None):
    """point-matching loss gradient for SE3_PM_LOSS_TYPE 'L1' | 'L2' | 'smooth_L1' (deepIM_flownet.py:458-499)"""
    check(lib().dim_pm_loss_grad(dptr(p_est, f32), dptr(p_obs, f32), dptr(weights, f32), dptr(grad, f32), p_est.numel(), float(norm_term),
                                 float(grad_scale), LOSS_TYPE_ID[loss_type], float(smooth_l1_scalar), dptr(loss_sum, f32), current_stream()))
    return grad


PM_SYM_MAX = 4096   # dim_pm_sym_loss_grad's largest symmetry set


def pm_sym_workspace(B, n_points, max_sym, device):
    return torch.empty((max(lib().dim_pm_sym_workspace_bytes(B, n_points, max_sym), 4) // 4,), dtype=f32, device=device)


def pm_sym_loss_grad(p_est, points_model, weights, tgt_pose, sym, sym_off, class_index, grad, norm_term, grad_scale, max_sym, loss_type="L1",
                     smooth_l1_scalar=1.0, loss_sum=None, target_out=None, best_sym=None, status=None, workspace=None):
    """dim_pm_sym_loss_grad: the point-matching loss gradient against the closest of the symmetric ground truths.  p_est,
    points_model, weights, grad (and target_out when given) (B,3,N) f32, tgt_pose (B,3,4) f32, sym (Stot,3,4) f32 and sym_off
    (n_classes+1,) int32 as lib.utils.symmetry.symmetry_tables builds them, class_index (B,) int32.  max_sym: at least the largest set
    of a class that occurs (a larger set gives the pair a zero gradient, best_sym -1 and DIM_STATUS_BAD_CLASS in status (B,) int32);
    it sizes the workspace.  loss_sum (1,) f32 accumulates the loss of the chosen symmetry, best_sym (B,) int32 receives its index
    within the class's set.  -> grad"""
    if loss_type not in LOSS_TYPE_ID:
        raise ValueError("pm_sym_loss_grad: loss_type must be one of {}, got {!r}".format(sorted(LOSS_TYPE_ID), loss_type))
    B, three, N = p_est.shape
    n_classes = sym_off.numel() - 1
    max_sym = int(max_sym)
    assert three == 3 and tuple(points_model.shape) == (B, 3, N) and tuple(weights.shape) == (B, 3, N) and tuple(grad.shape) == (B, 3, N)
    assert tuple(tgt_pose.shape) == (B, 3, 4) and class_index.numel() == B and n_classes >= 1
    assert sym.dim() == 3 and tuple(sym.shape[1:]) == (3, 4)
    assert target_out is None or tuple(target_out.shape) == (B, 3, N)
    assert (best_sym is None or best_sym.numel() == B) and (status is None or status.numel() == B)
    assert loss_sum is None or loss_sum.numel() == 1
    if workspace is None:
        workspace = pm_sym_workspace(B, N, max_sym, p_est.device)
    assert not 1 <= max_sym <= PM_SYM_MAX or workspace.numel() * workspace.element_size() >= lib().dim_pm_sym_workspace_bytes(B, N, max_sym)
    check(lib().dim_pm_sym_loss_grad(dptr(p_est, f32), dptr(points_model, f32), dptr(weights, f32), dptr(tgt_pose, f32), dptr(sym, f32),
                                     dptr(sym_off, i32), n_classes, dptr(class_index, i32), B, N, max_sym, float(norm_term),
                                     float(grad_scale), LOSS_TYPE_ID[loss_type], float(smooth_l1_scalar), dptr(workspace), dptr(grad, f32),
                                     _opt(target_out), _opt(best_sym, i32), _opt(loss_sum), _opt(status, i32), current_stream()))
    return grad


def se3_dist_loss_grad(rot_est_norm, rot_gt, fc7, p, zoom_trans_gt, d_rot_norm, d_zoom_trans, lw_rot, lw_trans, trans_loss_type="L2",
                       smooth_l1_scalar=3.0, loss_sums2=None):
    """SE3_DIST_LOSS (deepIM_flownet.py:396-437): adds the rot / trans loss gradients to d_rot_norm (B,4) / d_zoom_trans (B,3)"""
    check(lib().dim_se3_dist_loss_grad(dptr(rot_est_norm, f32), dptr(rot_gt, f32), dptr(fc7, f32), dptr(p["trans_weight"], f32),
                                       dptr(p["trans_bias"], f32), dptr(zoom_trans_gt, f32), dptr(d_rot_norm, f32), dptr(d_zoom_trans, f32),
                                       rot_est_norm.shape[0], float(lw_rot), float(lw_trans), LOSS_TYPE_ID[trans_loss_type],
                                       float(smooth_l1_scalar), dptr(loss_sums2, f32), current_stream()))


def se3_dist_loss_grad_cls(rot_est_norm, rot_gt, fc7, p, class_index, n_regressors, zoom_trans_gt, d_rot_norm, d_zoom_trans, lw_rot, lw_trans,
                           trans_loss_type="L2", smooth_l1_scalar=3.0, loss_sums2=None):
    """se3_dist_loss_grad with per-class trans heads (3K,256) / (3K): zoom_trans_est of sample b from the rows of class_index[b]"""
    B, K = rot_est_norm.shape[0], int(n_regressors)
    check(lib().dim_se3_dist_loss_grad_cls(dptr(rot_est_norm, f32), dptr(rot_gt, f32), dptr(fc7, f32), dptr(p["trans_weight"], f32),
                                           dptr(p["trans_bias"], f32), _cls_arg(class_index, B, K), K, dptr(zoom_trans_gt, f32),
                                           dptr(d_rot_norm, f32), dptr(d_zoom_trans, f32), B, float(lw_rot), float(lw_trans),
                                           LOSS_TYPE_ID[trans_loss_type], float(smooth_l1_scalar), dptr(loss_sums2, f32), current_stream()))


def quat_normalize(rot, out=None):
    out = out if out is not None else torch.empty_like(rot)
    check(lib().dim_quat_normalize(dptr(rot, f32), dptr(out, f32), rot.shape[0], current_stream()))
    return out


def pose_head_bwd(fc6a, fc7, rot_raw, d_rot_norm, d_trans, p, d_rot, dz7, dz6):
    check(lib().dim_pose_head_bwd(dptr(fc6a, f32), dptr(fc7, f32), dptr(rot_raw, f32), dptr(d_rot_norm, f32), dptr(d_trans, f32),
                                  dptr(p["fc7_weight"], f32), dptr(p["rot_weight"], f32), dptr(p["trans_weight"], f32), dptr(d_rot, f32),
                                  dptr(dz7, f32), dptr(dz6, f32), fc6a.shape[0], current_stream()))


def fc_wgrad(dz, x, dW, db=None):
    check(lib().dim_fc_wgrad(dptr(dz, f32), dptr(x, f32), dptr(dW, f32), dptr(db, f32), dz.shape[0], dz.shape[1], x.shape[1], current_stream()))


def pose_head_bwd_cls(fc6a, fc7, rot_raw, d_rot_norm, d_trans, p, class_index, n_regressors, d_rot, dz7, dz6):
    """pose_head_bwd through the rot (4K,256) / trans (3K,256) rows of each sample's class"""
    B, K = fc6a.shape[0], int(n_regressors)
    check(lib().dim_pose_head_bwd_cls(dptr(fc6a, f32), dptr(fc7, f32), dptr(rot_raw, f32), dptr(d_rot_norm, f32), dptr(d_trans, f32),
                                      dptr(p["fc7_weight"], f32), dptr(p["rot_weight"], f32), dptr(p["trans_weight"], f32),
                                      _cls_arg(class_index, B, K), K, dptr(d_rot, f32), dptr(dz7, f32), dptr(dz6, f32), B, current_stream()))


def fc_wgrad_cls(dz, x, class_index, n_regressors, dW, db=None):
    """dW (K Out, In) / db (K Out): class c's rows = fc_wgrad over the samples of class c; zeros for a class the batch does not hold"""
    B, K = dz.shape[0], int(n_regressors)
    assert tuple(dW.shape) == (K * dz.shape[1], x.shape[1]) and (db is None or db.numel() == K * dz.shape[1])
    check(lib().dim_fc_wgrad_cls(dptr(dz, f32), dptr(x, f32), _cls_arg(class_index, B, K), K, dptr(dW, f32), dptr(db, f32), B, dz.shape[1],
                                 x.shape[1], current_stream()))


def upsample16_bwd(dout_nchw, w_c1_32_32, df_nhwc, crop=8, scale=1.0):
    N, C, OH, OW = dout_nchw.shape
    _, h, w, _ = df_nhwc.shape
    check(lib().dim_upsample16_bwd(dptr(dout_nchw, f32), dptr(w_c1_32_32, f32), dptr(df_nhwc, f32), N, C, h, w, OH, OW, crop, float(scale),
                                   current_stream()))
    return df_nhwc


def conv_small_cout_bwd(x, Cin, dy, w_oihw, dx, dw, db, accumulate_dx=False, pad=1, workspace=None):
    N, H, W, in_cs = x.shape
    Cout, _, KH, KW = w_oihw.shape
    need = lib().dim_conv_small_cout_bwd_workspace_floats(N, H, W, Cin, Cout, KH, KW)
    if workspace is None or workspace.numel() < need:
        workspace = _new((need,), x)
    check(lib().dim_conv_small_cout_bwd(dptr(x, f32), dptr(dy, f32), dptr(w_oihw, f32), dptr(dx, f32), dptr(dw, f32), dptr(db, f32),
                                        dptr(workspace, f32), N, H, W, Cin, in_cs, dx.shape[-1] if dx is not None else 0, Cout, KH, KW, pad,
                                        int(accumulate_dx), current_stream()))


def deconv4x4s2_tiny_bwd(x, dy, dy_coff, w_iohw, dx, dw, db, crop=1):
    N, H, W, x_cs = x.shape
    _, OH, OW, dy_cs = dy.shape
    Cin, Cout = w_iohw.shape[:2]
    check(lib().dim_deconv4x4s2_tiny_bwd(dptr(x, f32), x_cs, dptr(dy, f32), dy_cs, dy_coff, dptr(w_iohw, f32), dptr(dx, f32), dptr(dw, f32),
                                         dptr(db, f32), N, H, W, Cin, Cout, OH, OW, crop, current_stream()))


def sgd_momentum(w, grad, mom, lr, momentum, wd, rescale_grad=1.0):
    check(lib().dim_sgd_momentum(dptr(w, f32), dptr(grad, f32), dptr(mom, f32), w.numel(), float(lr), float(momentum), float(wd),
                                 float(rescale_grad), current_stream()))


def adam(w, grad, mean, var, lr_t, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale_grad=1.0):
    check(lib().dim_adam(dptr(w, f32), dptr(grad, f32), dptr(mean, f32), dptr(var, f32), w.numel(), float(lr_t), float(beta1), float(beta2),
                         float(epsilon), float(wd), float(rescale_grad), current_stream()))


def pose_to_KT(pose_src, pose_tgt, K, out=None):
    B = pose_src.shape[0]
    out = out if out is not None else _new((B, 3, 4), pose_src)
    keep, kp = host_f32(K, 9)
    check(lib().dim_pose_to_KT(dptr(pose_src, f32), dptr(pose_tgt, f32), kp, dptr(out, f32), B, current_stream()))
    return out
