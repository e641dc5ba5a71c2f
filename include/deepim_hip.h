/* libdeepim_hip.so -- C ABI of the MI355X-native DeepIM refinement hot path.
 *
 * Drop-in boundary: these are the entry points a maintainer of wangg12/mx-DeepIM would bind
 * (ctypes) in place of
 *   - the numpy/MXNet bodies of the Python custom ops in deepim/operator_py/ (every .py there),
 *   - the one native function the reference has today,
 *       void _flow(float* flow, float* valid, float* depth_src, float* depth_tgt, float* KT,
 *                  float* Kinv, int batch_size, int height, int width, int device_id)
 *       (lib/flow_c/gpu_flow.hpp:1-3, Cython binding lib/flow_c/gpu_flow.pyx:24-41),
 *   - the glumpy renderer object lib/render_glumpy/render_py_multi.py:49-147,
 *   - MXNet's Convolution / FullyConnected operators used by deepim/symbols/deepIM_flownet.py.
 *
 * Conventions
 *   - every function returns DIM_OK (0) or a negative DIM_ERR_* code; dim_last_error() returns a
 *     thread-local description of the last failure on the calling thread.
 *   - pointers are DEVICE pointers (caller-owned, fp32, C-contiguous) unless the parameter name
 *     ends in a digit count (`K9`, `means3`, `T_means3`, ...): those are small HOST arrays.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work;
 *     nothing here allocates, frees or synchronises, so every call is hipGraph-capturable.
 *   - image-like tensors are NCHW as in the reference's blobs; the conv stack's activations are
 *     NHWC (this library's internal layout, produced by dim_zoom_net_input).
 */
#ifndef DEEPIM_HIP_H_
#define DEEPIM_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define DIM_OK 0
#define DIM_ERR_ARG (-1)
#define DIM_ERR_LAUNCH (-2)
/* per-sample status words (device int32).  Contract: dim_zoom_factor OVERWRITES status[b] (0 or its two bits) -- it is the first
 * kernel of an iteration, so a replayed loop (dim_refiner_run, Refiner._loop) starts every iteration's row clean without a fill;
 * dim_raster_render* OR their bits into the word.  A caller of a standalone render zeroes the words first (dim_fill_words), and a
 * caller that wants both kinds of bits in one word calls dim_zoom_factor BEFORE the render, as the loop does. */
#define DIM_STATUS_OBS_BOX_EMPTY 1 /* dim_zoom_factor: observed box empty (the reference raises) */
#define DIM_STATUS_REN_BOX_EMPTY 2 /* dim_zoom_factor: rendered box empty */
#define DIM_STATUS_BAD_CLASS 4     /* dim_raster_render*: class_index outside [0, n_classes): sample rendered as background; dim_pose_errors, dim_bop_errors: NaN row; dim_pose_head_fwd_cls: identity delta; dim_pose_from_box: fallback row */
#define DIM_STATUS_BAD_FACE 8      /* dim_raster_render*: a z-buffer key named a face outside the mesh (pixel left black) */
#define DIM_STATUS_BAD_K 16        /* dim_raster_render_k: the sample's K has fx <= 0, fy <= 0 or a non-finite entry (rendered as background) */
#define DIM_STATUS_ICP_FEW_POINTS 32 /* dim_icp_refine: an iteration found fewer than 64 inliers or a singular system (no update) */
#define DIM_STATUS_HYP_NO_SCORE 64  /* dim_pose_score[_indexed]: fewer than 64 counted pixels, a constant plane or a non-finite sum (score -inf); dim_hyp_topk: a slot filled for want of candidates */
#define DIM_STATUS_FLOW_PNP_FEW_POINTS 128 /* dim_flow_pnp: an iteration had fewer than 64 weighted points or a singular system (no update) */
#define DIM_STATUS_LAYER_HIDDEN 256 /* dim_scene_compose: a used layer won no pixel (empty or wholly hidden); per layer, (N*S) words */
#define DIM_STATUS_COARSE_BAD_BOX 512 /* dim_pose_from_box: a bad box, a class without points, a point behind the camera or a non-finite scale (fallback row) */
#define DIM_STATUS_PHOTO_FEW_POINTS 1024 /* dim_photo_refine: an iteration had fewer than 64 weighted points or a singular system, or the pair has no usable template (no update) */
#define DIM_STATUS_SIL_FEW_POINTS 2048 /* dim_sil_refine: an iteration had fewer than 64 weighted contour points or a singular system (no update) */
#define DIM_STATUS_TRACK_LOST 4096 /* dim_track_update: the track failed the lost test on this frame (the frame's pose was not accepted) */
#define DIM_STATUS_TRACK_REINIT 8192 /* dim_track_update: ... and was re-initialised from the offered pose */
#define DIM_STATUS_TRACK_OCCLUDED 16384 /* dim_track_update_occ: too little of the track's render is visible on this frame (it coasts, or is lost when the budget is spent) */
#define DIM_STATUS_VIEWS_NO_CONSENSUS 32768 /* dim_views_consensus: no view of the sample's group was eligible (view 0 was used) */
#define DIM_STATUS_VIEWS_CALIB_HELD 65536 /* dim_icp_refine_rig: the sample's camera shared too few points with the gauge camera in an iteration (its extrinsic was held) */
#define DIM_STATUS_TRACK_SEG_NO_MODEL 131072 /* dim_track_seg_mask: the track has no colour model yet, or its box gives no region (the mask is empty); not fatal */

const char* dim_last_error(void);
/* library / device probe: fills name (<= n bytes), returns number of compute units or <0 */
int dim_device_info(char* name, int n);

/* Device-to-device copy of `nwords` 4-byte words as a plain kernel launch.  The refinement loop uses it instead of
 * hipMemcpyAsync / hipMemsetAsync inside captured hipGraphs: a captured memset node was observed to overlap the kernel
 * after it on replay (ROCm 7.2), so no copy / fill node is left in the graph (deepim/core/tester.py Refiner._loop). */
int dim_copy_words(void* dst, const void* src, long nwords, void* stream);
/* The same for `rows` runs of `width_words` words with different pitches on the two sides: a channel window [:, a:b] of an
 * (O, I, kh, kw) weight is one run of (b - a) kh kw words per output channel (the training executor's first layer when the network
 * input has 6 or 10 channels: reference get_convs, deepim/symbols/deepIM_flownet.py:33-66). */
int dim_copy_rows(void* dst, long dst_pitch_words, const void* src, long src_pitch_words, long rows, long width_words, void* stream);
/* dst += src over the same geometry, as floats (the skip connections of the decoder add a channel range of a concat-gradient buffer to
 * an encoder gradient: get_convs Concat2 / Concat3, deepim/symbols/deepIM_flownet.py:236-299), and a constant fill (loss sums) -- so
 * that no vendor elementwise kernel sits on the training or test path. */
int dim_add_rows(float* dst, long dst_pitch, const float* src, long src_pitch, long rows, long width, void* stream);
int dim_fill_words(void* dst, long nwords, unsigned value, void* stream);

/* ---------------------------------------------------------------- zoom ops
 * bbox of {x > thr} (mode 0, C==1) or {sum_c (x_c + means3[c]) > thr} (mode 1, C==3):
 *   bbox[b] = {min_x, max_x, min_y, max_y}, empty = {W,-1,H,-1}.
 * replaces zoom_mask.py:36-70 / zoom_image.py:34-70 (np.max / np.nonzero on host copies). */
int dim_mask_bbox(const float* x, int B, int C, int H, int W, int mode, float thr, const float* means3, int* bbox, void* stream);

/* zoom window rule -> zoom_factor (B,4) = [wx, wy, tx, ty]   (zoom_mask.py:71-117).
 * status (B) may be NULL; bit0 = observed box empty (reference raises), bit1 = rendered box empty
 * (reference prints "NO POINT VALID IN MASK rendered" and uses the observed box). */
int dim_zoom_factor(const int* bbox_observed, const int* bbox_rendered, const float* src_pose, const float* K9, int B, int H, int W,
                    float* zoom_factor, int* status, void* stream);

/* affine bilinear gather of C planes with a zoom factor (GridGenerator + BilinearSampler fused).
 *   inverse   1 = inverse zoom (zoom_flow.py:35-44)
 *   pre       0 none | 1 binarise input at 0.2          (zoom_mask.py:39-46)
 *   post      0 none | 1 mx.nd.round | 2 round(x-0.45)   (zoom_mask.py:121-129, zoom_flow.py:74-76)
 *   add3      HOST per-plane constant added before / removed after sampling (pixel means), or NULL
 *   scale_mode 0 none | 1 divide by wx | 2 multiply by wx (zoom_flow.py:59-66) */
int dim_zoom_planes(const float* x, const float* zoom_factor, float* y, int B, int C, int H, int W, int inverse, int pre, int post,
                    const float* add3, int scale_mode, void* stream);

/* ZoomMask + ZoomImageWithFactor + Concat(/255) fused: X (B,H,W,8) NHWC network input
 * (deepIM_flownet.py:53-60).  The four z_* NCHW outputs are optional (all or none). */
int dim_zoom_net_input(const float* image_observed, const float* image_rendered, const float* mask_observed,
                       const float* mask_rendered, const float* zoom_factor, float* X_nhwc8, int B, int H, int W,
                       const float* means3, float* z_image_observed, float* z_image_rendered, float* z_mask_observed,
                       float* z_mask_rendered, void* stream);
/* the other input arities of get_convs (deepIM_flownet.py:33-66): mode 0 = masks (as dim_zoom_net_input), 1 = images only (INPUT_MASK
 * off, ZoomImage path: channels 6, 7 of X are zero), 2 = depth_observed / depth_rendered in place of the masks (INPUT_DEPTH without
 * masks: ZoomDepth's plain bilinear sample, / 255), 3 = the two zoomed masks alone in lanes 0, 1 (lanes 2-7 zero; images not read): the
 * second 8-lane group of the 10-channel first layer (INPUT_DEPTH with masks; the first group is mode 2).  X stays (B,H,W,8) NHWC. */
int dim_zoom_net_input_ex(const float* image_observed, const float* image_rendered, const float* extra_observed, const float* extra_rendered,
                          const float* zoom_factor, float* X_nhwc8, int B, int H, int W, const float* means3, int mode, void* stream);

/* The same samplers from planes of a SOURCE size Hs x Ws into the NETWORK size Hn x Wn (MXNet's GridGenerator(target_shape = (Hn, Wn))
 * + BilinearSampler on Hs x Ws data): target coordinates x_t = -1 + j 2/(Wn-1), j < Wn; the affine step unchanged; x_real =
 * (x_s + 1)(Ws-1)/2; corner validity, clamps and plane stride of the Hs x Ws planes.  The zoom factor is the window in the source's
 * normalised coordinates (dim_zoom_factor with H = Hs, W = Ws).  With Hs, Ws == Hn, Wn every bit equals the entry points above.  All
 * four sizes must be >= 2.
 * dim_zoom_planes_src: the forward direction of dim_zoom_planes (no inverse, no scale_mode): x (B,C,Hs,Ws) -> y (B,C,Hn,Wn).
 * dim_zoom_net_input_src: dim_zoom_net_input_ex (modes 0-3) with X (B,Hn,Wn,8), plus the four optional (Hn,Wn) NCHW outputs of
 * dim_zoom_net_input (all or none; mode 0 only). */
int dim_zoom_planes_src(const float* x, const float* zoom_factor, float* y, int B, int C, int Hs, int Ws, int Hn, int Wn, int pre, int post,
                        const float* add3, void* stream);
int dim_zoom_net_input_src(const float* image_observed, const float* image_rendered, const float* extra_observed, const float* extra_rendered,
                           const float* zoom_factor, float* X_nhwc8, int B, int Hs, int Ws, int Hn, int Wn, const float* means3, int mode,
                           float* z_image_observed, float* z_image_rendered, float* z_mask_observed, float* z_mask_rendered, void* stream);

/* The `_src` samplers with an area filter for windows that shrink the source.  Per pair and per axis, with the
 * window's size w = |wx| or |wy| of zoom_factor[b]:
 *   step = w * f32((S-1)/(N-1))                       source pixels per network pixel (S, N: source and network extent of the axis)
 *   n    = min(max(floor(step + 0.5), 1), max_taps)   sub-samples (a NaN step gives 1, an infinite one max_taps)
 *   o_k  = f32((k + 0.5)/n - 0.5), k < n              their offsets in network pixels (0 for n = 1)
 * Every output is the mean of the n_y x n_x bilinear samples at the target coordinates -1 + (j + o_k) 2/(N-1): summed with ky outer and
 * kx inner, one float32 addition each, then one division by n_x n_y; `- add`, the rounding and / 255 follow the mean.  Sub-samples
 * outside the source plane are zeros (no clamp).  Where n_x = n_y = 1 every bit equals the `_src` entry point.  The argument lists and
 * checks are the `_src` ones plus max_taps in 1..8.
 * dim_zoom_area_taps writes the (n_x, n_y) the two samplers use into taps_xy, device (B,2) int32. */
int dim_zoom_planes_area(const float* x, const float* zoom_factor, float* y, int B, int C, int Hs, int Ws, int Hn, int Wn, int pre, int post,
                         const float* add3, int max_taps, void* stream);
int dim_zoom_net_input_area(const float* image_observed, const float* image_rendered, const float* extra_observed, const float* extra_rendered,
                            const float* zoom_factor, float* X_nhwc8, int B, int Hs, int Ws, int Hn, int Wn, const float* means3, int mode,
                            float* z_image_observed, float* z_image_rendered, float* z_mask_observed, float* z_mask_rendered, int max_taps,
                            void* stream);
int dim_zoom_area_taps(const float* zoom_factor, int B, int Hs, int Ws, int Hn, int Wn, int max_taps, int* taps_xy, void* stream);

/* ZoomTrans (zoom_trans.py:22-76): mode 0 copy, 1 (dx,dy)/wx, 2 (dx,dy)*wx */
int dim_zoom_trans(const float* zoom_factor, const float* in, float* out, int B, int mode, void* stream);

/* ---------------------------------------------------------------- SE(3)
 * rot_coord: 0 MODEL, 1 CAMERA, 2 CAMERA_NEW, 3 NAIVE.
 * pose_out = RT_transform(pose_src, se3[:, :4], se3[:, 4:])  (RT_transform.py:135-161); float64 inside. */
int dim_se3_compose(const float* pose_src, const float* se3, float* pose_out, double* pose_out_f64, int B, int rot_coord,
                    const float* T_means3, const float* T_stds3, void* stream);
/* (rot_quat, trans) = calc_RT_delta(pose_src, pose_tgt, rot_type="QUAT")  (RT_transform.py:16-48) */
int dim_se3_delta(const float* pose_src, const float* pose_tgt, float* rot_quat, float* trans, int B, int rot_coord,
                  const float* T_means3, const float* T_stds3, void* stream);
/* the same residual with the rotation as a 3x3 matrix (calc_RT_delta(..., rot_type="MATRIX"), RT_transform.py:16-48): rot_mat (B,3,3) */
int dim_se3_delta_matrix(const float* pose_src, const float* pose_tgt, float* rot_mat, float* trans, int B, int rot_coord,
                         const float* T_means3, const float* T_stds3, void* stream);
/* EULER deltas (RT_transform.py:139-140, :39-40: euler2mat / mat2euler with their default static-xyz axes): euler_trans6 (B,6) =
 * [ai, aj, ak, tx, ty, tz]; rot_euler (B,3). */
int dim_se3_compose_euler(const float* pose_src, const float* euler_trans6, float* pose_out, double* pose_out_f64, int B, int rot_coord,
                          const float* T_means3, const float* T_stds3, void* stream);
int dim_se3_delta_euler(const float* pose_src, const float* pose_tgt, float* rot_euler, float* trans, int B, int rot_coord,
                        const float* T_means3, const float* T_stds3, void* stream);
/* KT (B,3,4) = K * calc_se3(pose_src, pose_tgt): the per-sample matrix dim_depth_to_flow needs (batch_updater_py_multi.py:306-312) */
int dim_pose_to_KT(const float* pose_src, const float* pose_tgt, const float* K9, float* KT, int B, void* stream);
/* Transform3D custom op (transform3d.py:42-327); points/out/out_grad are (B,3,Npts). */
int dim_transform3d_fwd(const float* points, const float* rot, const float* trans, const float* pose_src, float* out, int B,
                        int Npts, int rot_coord, const float* T_means3, const float* T_stds3, void* stream);
int dim_transform3d_bwd(const float* out_grad, const float* points, const float* rot, const float* trans, const float* pose_src,
                        float* d_rot, float* d_trans, int B, int Npts, int rot_coord, const float* T_means3, const float* T_stds3,
                        void* stream);

/* ---------------------------------------------------------------- depth -> flow labels
 * device-pointer version of _flow (lib/flow_c/gpu_flow.hpp:1-3): flow (B,2,H,W) in (dy,dx), valid (B,1,H,W). */
int dim_depth_to_flow(const float* depth_src, const float* depth_tgt, const float* KT, const float* Kinv9, int B, int H, int W,
                      float* flow, float* valid, void* stream);
/* Test-time flow error of the first forward (deepim/core/tester.py:500-512; calc_EPE_one_pair :719-736 over the [flow, visible, bg]
 * list of par_generate_gt :706-716).  flow_pred = the network's flow_est_crop_output (B,2,H,W), rounded to float16 first as
 * tester.py:485-487 stores it; flow_gt (B,2,H,W) / visible (B,1,H,W) = calc_flow's outputs (dim_calc_flow_labels, weight_type 1);
 * bg = visible == 0 and depth_rendered == 0.  sums (B,5) float64 (device) = {epe_all, epe_viz, epe_vizbg, num_viz, num_vizbg} per
 * sample (num_all = H W), overwritten or -- accumulate != 0 -- added to.  Float64 arithmetic like numpy's (calc_flow returns
 * float64); deterministic two-stage sum.  workspace: dim_flow_epe_workspace_bytes(B) bytes (doubles), 8-byte aligned, no
 * initialisation needed: every partial sum is written before it is read. */
long dim_flow_epe_workspace_bytes(int B);
int dim_flow_epe_sums(const float* flow_pred, const float* flow_gt, const float* visible, const float* depth_rendered, int B, int H,
                      int W, void* workspace, double* sums, int accumulate, void* stream);

/* ---------------------------------------------------------------- depth ICP after the refinement loop (RGB-D test time)
 * Projective point-to-plane ICP, model to frame, `iters` fixed iterations (no early exit: graph-capturable), restated in float64 by
 * tests/icp_reference.py.  Per pair b:
 *   source = the pixels of depth_rendered (B,1,H,W) metres > 0 inside bbox[b] (B,4 int32 {min_x,max_x,min_y,max_y} inclusive, as
 *   dim_raster_render* returns it; NULL = whole frame), back-projected with the pair's camera: p0 = d ((x-cx)/fx, (y-cy)/fy, 1).
 *   pose_in (B,3,4) = T0, the pose depth_rendered was rendered at.  Each iteration moves p0 by the correction T_delta (identity at the
 *   start), projects it to the integer pixel floor(fx px/pz + cx + 0.5), floor(fy py/pz + cy + 0.5) inside [1,W-2] x [1,H-2] of
 *   depth_observed (B,1,H,W) metres, 0 = no reading, gated by mask_observed (B,1,H,W) >= 0.5 when given (NULL = none); the
 *   observed point q and its four neighbours (depth > 0, |depth - depth(q)| < max_dist) give the normal n (n . q < 0); pairs with
 *   |p - q| > max_dist are rejected.  r = n . (p - q), J = (p x n, n); (A + 1e-9 tr(A)/6 I) xi = -sum J r by float64 Cholesky,
 *   T_delta <- [Rodrigues(omega) | v] T_delta.  Fewer than 64 inliers or a non-positive-definite A: no update, and
 *   DIM_STATUS_ICP_FEW_POINTS is OR-ed into status[b] (B int32, may be NULL).
 * pose_out (B,3,4) = T_delta T0 in float32; a pair that never updated gets pose_in bit for bit.  stats (B,iters,2) f32 or NULL =
 * (inliers, rms residual in metres) of every iteration before its update.  Camera: K_per_sample (B,9) device f32 (fx = [0],
 * fy = [4], cx = [2], cy = [5]) or NULL = K9 (host, 9 floats) for every pair; a non-positive or non-finite focal length gives the
 * pair no source points.  workspace: dim_icp_workspace_bytes(B, H, W) bytes, 8-byte aligned, no initialisation needed.
 * Sums: float32 per lane, float64 across lanes, waves and workgroups in a fixed order (no atomics): a replay is bit-identical.
 * 2 launches per iteration; iters == 0 copies pose_in to pose_out.  B <= 0, iters < 0, max_dist <= 0, H or W < 3 or a NULL
 * required pointer return DIM_ERR_ARG before anything is enqueued. */
long dim_icp_workspace_bytes(int B, int H, int W);
int dim_icp_refine(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox, const float* pose_in,
                   const float* K9, const float* K_per_sample, int B, int H, int W, int iters, float max_dist, void* workspace,
                   float* pose_out, float* stats, int* status, void* stream);

/* ---------------------------------------------------------------- pose from predicted flow (a deterministic robust PnP)
 * The device form of flow2se3 (lib/pair_matching/flow2se3.py:13-56): back-project the rendered depth, add the flow to every pixel,
 * solve for the pose that maps the 3-D points onto the flowed pixels.  The reference's cv2.solvePnPRansac draws random samples and
 * exits early; here `iters` fixed Gauss-Newton iterations with a Huber weight under a hard gate (graph-capturable), restated in
 * float64 by tests/flow_pnp_reference.py.  Per pair b:
 *   a source pixel (x, y) is taken when it lies inside bbox[b] (B,4 int32 {min_x,max_x,min_y,max_y} inclusive, clipped to the frame,
 *   as dim_raster_render* returns it; NULL = whole frame), depth_rendered (B,1,H,W) metres > 0, both components of flow (B,2,H,W)
 *   are finite and valid (B,1,H,W; NULL = none) is >= 0.5 AT THE SOURCE PIXEL (flow2se3 indexes mask_image by source pixel too).
 *   It gives the point p = d ((x-cx)/fx, (y-cy)/fy, 1) and the target (u, v) = (x + flow_x, y + flow_y); flow[:,0] is dy and
 *   flow[:,1] dx unless standard_rep != 0 (lib/pair_matching/flow.py, dim_depth_to_flow).  A target outside
 *   [-0.5, W-0.5] x [-0.5, H-0.5] is dropped.
 *   T = [R|t] starts at the identity.  Each iteration: m = R p + t (m_z <= 0: dropped), r = (fx m_x/m_z + cx - u,
 *   fy m_y/m_z + cy - v), e = |r|; weight w = 1 in the first `warm` iterations (at the identity the residual is the flow itself, so
 *   nothing may be gated yet), afterwards w = 0 when e > max_px, 1 when e <= huber_px and huber_px / e between; Jacobian rows in
 *   the left twist xi = (omega, v), dm = omega x m + v; (A + 1e-9 tr(A)/6 I) xi = -sum w J^T r by float64 Cholesky,
 *   T <- [Rodrigues(omega) | v] T.  Fewer than 64 points with w > 0 or a non-positive-definite A: no update, and
 *   DIM_STATUS_FLOW_PNP_FEW_POINTS is OR-ed into status[b] (B int32, may be NULL).
 * pose_out (B,3,4) f32 = T pose_src (pose_src (B,3,4): the pose depth_rendered was rendered at); a pair that never updated gets
 * pose_src bit for bit.  se3_q (B,7) f32 or NULL = [mat2quat(R), t] as flow2se3 returns it ([1,0,0,0,0,0,0] for a pair that never
 * updated, flow2se3's "not convex" answer).  stats (B,iters,2) f32 or NULL = (points with w > 0, rms of e over them in pixels) of every
 * iteration before its update.  Camera as dim_icp_refine: K_per_sample (B,9) device f32 or NULL = K9 (host, 9 floats) for every
 * pair; a non-positive or non-finite focal length gives the pair no points.
 * workspace: dim_flow_pnp_workspace_bytes(B, H, W) bytes, 8-byte aligned, no initialisation needed.
 * Arithmetic: float64 per point, per lane, across lanes, waves and workgroups in a fixed order (no atomics): a replay is
 * bit-identical.  Four pixels per lane, as 16-byte loads when W % 4 == 0 and the planes are 16-byte aligned.  2 launches per
 * iteration; iters == 0 copies pose_src to pose_out (and writes the identity se3_q).  B <= 0, iters < 0, warm < 0, huber_px <= 0,
 * max_px < huber_px, H or W < 1 or a NULL required pointer return DIM_ERR_ARG before anything is enqueued. */
long dim_flow_pnp_workspace_bytes(int B, int H, int W);
int dim_flow_pnp(const float* depth_rendered, const float* flow, const float* valid, const int* bbox, const float* pose_src, const float* K9,
                 const float* K_per_sample, int B, int H, int W, int standard_rep, int iters, int warm, float huber_px, float max_px,
                 void* workspace, float* pose_out, float* se3_q, float* stats, int* status, void* stream);

/* ---------------------------------------------------------------- photometric pose polish after the refinement loop (RGB test time)
 * Dense direct image alignment between the render at a pose and the observed image: coarse to fine over `levels` pyramid levels,
 * `iters` fixed Gauss-Newton iterations per level (no early exit: graph-capturable), restated by tests/photo_reference.py.  A polish
 * for a pose that is already within a few degrees and millimetres, not a tracker.  Per pair b:
 *   image_observed, image_rendered (B,3,H,W) f32 mean-subtracted blobs give the gray planes g = (c0 + c1) + c2 (float32, no division:
 *   huber and gate are in units of the channel sum); depth_rendered (B,1,H,W) metres, 0 = background; pose_in (B,3,4) = T0, the pose
 *   the render was drawn at; bbox[b] (B,4 int32 {min_x,max_x,min_y,max_y} inclusive, clipped to the frame, as dim_raster_render*
 *   returns it; NULL = whole frame).
 *   Pyramids: level 0 is the frame, level l the 2x2 mean ((a + b) + (c + d)) * 0.25f of level l-1 (a, b the upper row), size
 *   floor(H/2) x floor(W/2) of it (a leftover row or column is dropped) -- of the observed gray, the rendered gray, the rendered depth
 *   and a template-valid flag: level 0 = depth > 0 inside the box, level l = all four children valid.
 *   Gain and bias: over the level-0 valid pixels float64 n, sum Ir, sum Ir^2, sum Io, sum Io^2 (Io at the same pixel);
 *   a = sqrt(var_o / var_r), b = mean_o - a mean_r (gain == 0: a = 1, b = 0); the template value is t = a Ir_l + b.  n < 64 or a
 *   variance that is not a finite number > 0: the pair takes no step in any iteration.
 *   Levels levels-1 .. 0; T_delta starts at the identity and carries over.  At level l, s = 2^l, a valid pixel (X, Y) has the level-0
 *   centre (xc, yc) = (X s + (s-1)/2, Y s + (s-1)/2) and the point p0 = d_l ((xc-cx)/fx, (yc-cy)/fy, 1).  Each iteration:
 *   p = R p0 + t (p_z <= 0: dropped), (u, v) its projection, (U, V) = ((u - (s-1)/2)/s, (v - (s-1)/2)/s), cell x0 = floor(U),
 *   y0 = floor(V) (dropped unless 0 <= x0 < W_l - 1 and 0 <= y0 < H_l - 1), I the bilinear value of the observed level there and
 *   (gx, gy) the gradient of that interpolant divided by s; r = I - t, e = |r|, w = 1 for e <= huber, huber / e above, 0 for
 *   e > gate; gp = gx du/dp + gy dv/dp, J = (p x gp, gp) in the left twist xi = (omega, v);
 *   (A + 1e-9 tr(A)/6 I) xi = -sum w J r by float64 Cholesky, T_delta <- [Rodrigues(omega) | v] T_delta.  Fewer than 64 points with
 *   w > 0 or a non-positive-definite A: no update, DIM_STATUS_PHOTO_FEW_POINTS is OR-ed into status[b] (B int32, may be NULL), and
 *   the later iterations and levels still run.
 * pose_out (B,3,4) f32 = T_delta T0; a pair that never updated gets pose_in bit for bit.  stats (B, levels*iters, 2) f32 or NULL =
 * (points with w > 0, sqrt(sum of w r^2 over them / their count)) of every iteration before its update, coarsest level first.
 * Camera as dim_icp_refine: K_per_sample (B,9) device f32 or NULL = K9 (host, 9 floats) for every pair; a non-positive or non-finite
 * focal length gives the pair no points.
 * workspace: dim_photo_workspace_bytes(B, H, W, levels) bytes (0 for a refused shape), no initialisation needed; 16-byte aligned for
 * the 16-byte loads (8 suffices otherwise).  It holds the Gauss-Newton state and partials, per pair 8 doubles {n, sum Ir, sum Ir^2,
 * sum Io, sum Io^2, a, b, may step} and the planes; dim_photo_workspace_offset(B, H, W, levels, plane, level) is the byte offset of
 * plane 0 .. 3 = {observed gray, rendered gray, depth, valid flag as 0.f / 1.f} at `level` ((B, H_l, W_l) f32), and with plane = 4 of
 * the (B, 8) doubles (-1 for a bad index) -- for tests and diagnostics.
 * Arithmetic: planes in float32; per point, per lane, across lanes, waves and workgroups float64 in a fixed order (no atomics, no
 * memcpy / memset): a replay is bit-identical.  16-byte loads in the pyramid pass when W % 4 == 0 and the arrays are 16-byte aligned.
 * levels + 2 + 2 levels iters launches; iters == 0 copies pose_in to pose_out.  B <= 0, levels outside 1 .. 5, iters < 0, huber <= 0,
 * gate < huber, a coarsest level smaller than 3 x 3 or a NULL required pointer (the three images, pose_in, K9, workspace, pose_out)
 * return DIM_ERR_ARG before anything is enqueued. */
long dim_photo_workspace_bytes(int B, int H, int W, int levels);
long dim_photo_workspace_offset(int B, int H, int W, int levels, int plane, int level);
int dim_photo_refine(const float* image_observed, const float* image_rendered, const float* depth_rendered, const int* bbox,
                     const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int levels, int iters,
                     float huber, float gate, int gain, void* workspace, float* pose_out, float* stats, int* status, void* stream);

/* ---------------------------------------------------------------- silhouette pose polish after the refinement loop (RGB test time)
 * Contour alignment for textureless objects: the outline of the render at a pose is pulled onto the edge of a segmentation mask
 * (a detector's, or the network's own mask head).  Restated by tests/sil_reference.py.  A polish for a pose that is already within a
 * few degrees and pixels; a silhouette constrains depth, and rotation about the axes of near-symmetric outlines, only weakly.
 *
 * dim_sil_edge_field: mask (B,1,H,W) f32 -> field (B,H,W) int32, the exact nearest edge pixel of every pixel within `radius`.
 *   A pixel is foreground when m >= 0.5 (a NaN is background).  An edge pixel is a foreground pixel with at least one 4-neighbour
 *   inside the frame that is background; neighbours outside the frame count as foreground, so an object cut by the image border grows
 *   no edge along the border.  field[b,y,x] = (ey << 16) | ex of the edge pixel of pair b that minimises the key (dx^2 + dy^2, ex, ey)
 *   lexicographically among the edge pixels with dx^2 + dy^2 <= radius^2, or -1 when there is none.  Integer arithmetic throughout:
 *   the result is exact and has no ties.  Two launches (columns, then rows; the column pass leaves its nearest edge row per pixel in
 *   `field` itself and the row pass rewrites each row in place, so no scratch is needed), no atomics: a replay is bit-identical.
 *   1 <= radius <= 64, H and W in 3 .. 32767, B in 1 .. 65535; otherwise, or with a NULL pointer, DIM_ERR_ARG before anything is
 *   enqueued.
 *
 * dim_sil_refine: `iters` fixed Gauss-Newton iterations (no early exit: graph-capturable) per pair b.
 *   depth_rendered (B,1,H,W) metres, 0 = background, rendered at pose_in (B,3,4) = T0; field (B,H,W) from dim_sil_edge_field; bbox,
 *   K9 / K_per_sample, stats, status and the workspace as dim_flow_pnp: bbox[b] (B,4 int32 {min_x,max_x,min_y,max_y} inclusive,
 *   clipped to the frame; NULL = whole frame), K_per_sample (B,9) device f32 or NULL = K9 (host, 9 floats) for every pair, a
 *   non-positive or non-finite focal length gives the pair no points.
 *   Contour points: a pixel (x, y) inside the clipped box with depth > 0 and at least one 4-neighbour inside the frame (not
 *   necessarily inside the box) whose depth is not > 0; the frame-border rule is that of the field.  p0 = d ((x-cx)/fx, (y-cy)/fy, 1).
 *   T = [R | t] starts at the identity.  Each iteration: m = R p0 + t (m_z <= 0: dropped), (u, v) = (fx m_x/m_z + cx, fy m_y/m_z + cy),
 *   xi = floor(u + 0.5), yi = floor(v + 0.5) (outside the frame: dropped), f = field[b, yi, xi] (f < 0: dropped), (ex, ey) its edge
 *   pixel, r = (u - ex, v - ey), e = |r|, w = 0 for e > max_px, 1 for e <= huber_px, huber_px / e between.  Jacobian rows in the left
 *   twist (omega, v) with dm = omega x m + v, (A + 1e-9 tr(A)/6 I) xi = -sum w J r by float64 Cholesky, T <- [Rodrigues(omega) | v] T
 *   -- the arithmetic of dim_flow_pnp.  Fewer than 64 points with w > 0 or a non-positive-definite A: no update,
 *   DIM_STATUS_SIL_FEW_POINTS is OR-ed into status[b] (B int32, may be NULL), and the later iterations still run.
 *   Matching is one-directional, render to mask: an occluded mask only loses points to the gate.
 * pose_out (B,3,4) f32 = T T0; a pair that never updated gets pose_in bit for bit.  stats (B, iters, 2) f32 or NULL = (points with
 * w > 0, rms of e over them in pixels) of every iteration before its update.
 * workspace: dim_sil_workspace_bytes(B, H, W) bytes = B (16 + 16 x 32) doubles (0 for B <= 0), 8-byte aligned, no initialisation needed.
 * Arithmetic: float64 per point, per lane, across lanes, waves and workgroups in a fixed order; the box is scanned in every
 * iteration and its contour pixels are compacted by position (no atomics): a replay is bit-identical.  Two launches per iteration;
 * iters == 0 copies pose_in to pose_out.  B outside 1 .. 65535, iters < 0, huber_px <= 0, max_px < huber_px, H or W outside
 * 3 .. 32767 (a field word holds 16 bits per coordinate) or a NULL required pointer (depth_rendered, field, pose_in, K9, workspace,
 * pose_out) return DIM_ERR_ARG before anything is enqueued. */
int dim_sil_edge_field(const float* mask, int B, int H, int W, int radius, int* field, void* stream);
long dim_sil_workspace_bytes(int B, int H, int W);
int dim_sil_refine(const float* depth_rendered, const int* field, const int* bbox, const float* pose_in, const float* K9,
                   const float* K_per_sample, int B, int H, int W, int iters, float huber_px, float max_px, void* workspace,
                   float* pose_out, float* stats, int* status, void* stream);

/* ---------------------------------------------------------------- one object from several calibrated cameras (joint pose stages)
 * A batch of B = G V samples holds G groups (one object instance each) with V views, 1 <= V <= 16; sample b = g V + v.
 * cam_T_rig (B,3,4) f32 holds the rigid X_b = [R_b | t_b] with p_cam = X_b p_rig (a rig of V fixed cameras repeats its V rows G
 * times).  A group has one pose T_g (3,4) in the rig frame; its pose in the camera of sample b is X_b T_g.
 * X_b^-1 = [R_b^T | -R_b^T t_b]: nothing on the device checks that X_b is rigid.  Restated in float64 by tests/views_reference.py.
 *
 * dim_views_from_rig: pose_views[b] (B,3,4) = float32(X_b pose_rig[g]) (pose_rig (G,3,4)), products and sums in float64, rounded once.
 *
 * dim_views_consensus: one rig pose per group from the per-view poses `pose` (B,3,4) and their scores.  A view is eligible when
 *   score[b] (B f32, as dim_pose_score gives it) is finite and (status[b] & fatal_mask) == 0 (status (B) int32, NULL = no bits).
 *   choice[g] (G int32) = the eligible view v with the largest score, the lowest v on a tie; c = g V + choice[g].
 *   pose_rig[g] (G,3,4) = float32(X_c^-1 pose[c]) in float64; for b != c pose_views[b] = float32(X_b (X_c^-1 pose[c])), from the
 *   float64 product and not from the rounded pose_rig; pose_views[c] = pose[c] bit for bit.  No eligible view: choice[g] = -1, view 0
 *   is used as c, and DIM_STATUS_VIEWS_NO_CONSENSUS is OR-ed into status_out[b] (B int32, may be NULL, may be status itself) of all V
 *   samples; status_out is not written otherwise.  pose_views may be pose itself.
 * Both: one launch, no workspace, no atomics; G <= 0, V outside 1 .. 16 or a NULL required pointer return DIM_ERR_ARG before
 * anything is enqueued.
 *
 * dim_icp_refine_views, dim_photo_refine_views, dim_sil_refine_views: the stage of the same name with ONE correction per group.
 *   Arguments, checks, accumulate launches (the photometric pyramid and gain passes included), stats (B, iters, 2) rows and the
 *   workspace layout are those of the single-view entry; the solve launch of every iteration is the joint one, per group g:
 *   for v = 0 .. V-1 in order, s_v = the sample's 16 workgroup partials added in block order; A_v from terms 0..20, g_v from terms
 *   21..26, N_v = term 27, rr_v = term 28.  With twists ordered (omega, v), Ad_v = [[R_v, 0], [[t_v]x R_v, R_v]] maps a rig-frame twist
 *   to the camera of sample g V + v, and A = sum_v Ad_v^T A_v Ad_v, g = sum_v Ad_v^T g_v, N = sum_v N_v, rr = sum_v rr_v, all in
 *   ascending v, in float64.  stats_group (G, iters, 2) f32 or NULL = (N, sqrt(rr / N)) (0 for N = 0).  The step is taken when
 *   N >= 64 -- the group's points, not each view's -- and (A + 1e-9 tr(A)/6 I) xi = -g passes the float64 Cholesky.  The correction
 *   lives in the rig frame, D_g <- [Rodrigues(omega) | v] D_g from the identity, and after every iteration the correction of sample
 *   b, the one its accumulate kernel linearises at next, is rewritten as X_b D_g X_b^-1 in float64: the samples' corrections are
 *   conjugates of one rig correction by construction, not separately integrated twists ([Rodrigues(omega) | v] is a retraction,
 *   not the exponential, so integrating Ad_v xi per view would let the views drift apart at second order).  A skipped step ORs the
 *   stage's FEW_POINTS bit into status[b] of all V samples and leaves D_g; the later iterations still run.
 *   pose_out[b] = float32((X_b D_g X_b^-1) pose_in[b]) and pose_rig_out[g] (G,3,4) = float32(D_g pose_rig_in[g]); a group that never
 *   stepped gets pose_in and pose_rig_in bit for bit.  With V = 1 and X_b = [I | 0] every entry returns the bits of its single-view
 *   entry.  workspace: dim_<stage>_views_workspace_bytes bytes = the single-view layout unchanged, then G x 16 doubles of group
 *   state {R, t, stepped, pad}; alignment as the single-view entry, no initialisation needed.  One workgroup of 64 lanes per group:
 *   the 29-term sums spread over lanes, the fusion on one lane; no atomics, fixed order: a replay is bit-identical.
 *   Launches as the single-view entry.  iters == 0 copies pose_in to pose_out and pose_rig_in to pose_rig_out.  V outside 1 .. 16,
 *   B % V != 0, a NULL cam_T_rig, pose_rig_in or pose_rig_out and every condition of the single-view entry return DIM_ERR_ARG before
 *   anything is enqueued.
 *
 * dim_icp_refine_rig: dim_icp_refine_views with the rig's extrinsics refined along (a small bundle adjustment over the G objects of
 *   the batch; restated in float64 by tests/rig_reference.py).  Arguments, checks and the accumulate launch are those of
 *   dim_icp_refine_views.  cam_T_rig stays (B,3,4): the V rows of group 0 are read as the nominal X_v, the rows of the other groups
 *   must repeat them (the caller's check).  pose_in[b] is (about) X_v pose_rig_in[g], as dim_views_consensus leaves it.
 *   Unknowns: a correction C_v per camera, X'_v = C_v X_v, with C_0 = I for good (camera 0 is the gauge: its row never changes), and
 *   a rig-frame correction D_g per object; all from the identity.  The correction of sample b, what its accumulate kernel linearises
 *   at, is S_b = X'_v D_g X_v^-1 (the inverse of the NOMINAL X_v: depth_rendered was drawn at pose_in), so S_b pose_in[b] = X'_v D_g P_g.
 *   A left perturbation exp(alpha_v) of C_v and exp(eta_g) of D_g moves sample b by the camera-frame twist alpha_v + Ad(X'_v) eta_g,
 *   Ad([R|t]) = [[R,0],[[t]x R,R]] at the CURRENT extrinsic (never-moved cameras use the nominal row exactly).
 *   One iteration: s_gv, A_gv, g_gv, N_gv, rr_gv as the joint solve takes them (block order); W_gv = A_gv Ad_v,
 *   H_ee[g] = sum_v Ad_v^T W_gv, r_e[g] = -sum_v Ad_v^T g_gv, H_aa[v] = sum_g A_gv, r_a[v] = -sum_g g_gv, coupling block
 *   (alpha_v, eta_g) = W_gv; every sum ascending, float64.  Who takes part, from the counts alone: group g is active when
 *   N_g = sum_v N_gv >= 64 (an inactive group enters no sum, keeps D_g, and its V samples get DIM_STATUS_ICP_FEW_POINTS); view v >= 1
 *   is free when the sum of N_gv over the active groups with N_g0 >= 64 is >= 64, else held for the iteration: alpha_v = 0, its block
 *   leaves the reduced system, its samples still count in H_ee and r_e at X'_v, and its samples in all groups get
 *   DIM_STATUS_VIEWS_CALIB_HELD.  H_ee[g] and H_aa[v] of the free views get + 1e-9 tr/6 I.  S = H_aa - sum_g W_g H_ee[g]^-1 W_g^T and
 *   rs = r_a - sum_g W_g H_ee[g]^-1 r_e[g] over the free views (H_ee^-1 through the 6x6 Cholesky), S (at most 90 x 90) by Cholesky,
 *   eta_g = H_ee[g]^-1 r_e[g] - (H_ee[g]^-1 W_g^T) alpha.  A pivot that is not > 0 anywhere skips the whole step:
 *   DIM_STATUS_ICP_FEW_POINTS on all B samples, nothing moves.  Otherwise C_v <- [Rodrigues(alpha_v) | alpha_v,trans] C_v,
 *   D_g <- [Rodrigues(eta_g) | eta_g,trans] D_g and every state row is rewritten.  With no free view (V = 1 always) the step is
 *   dim_icp_refine_views' per active group, bit for bit, a failed Cholesky flagging its own group only.
 *   After the last iteration pose_out[b] = float32(S_b pose_in[b]), pose_rig_out[g] = float32(D_g pose_rig_in[g]) and
 *   cam_T_rig_out[g V + v] (B,3,4, required, not cam_T_rig itself) = float32(C_v X_v) for every g; a group that never stepped gets
 *   pose_in and pose_rig_in bit for bit, a view that never moved its nominal row bit for bit.  iters == 0 copies the three inputs.
 *   stats, stats_group as dim_icp_refine_views; stats_view (V, iters, 2) f32 or NULL = (sum_g N_gv, sqrt(sum_g rr_gv / that)) over
 *   all groups in ascending g, 0 for an empty view.
 *   workspace: dim_icp_rig_workspace_bytes bytes = the joint layout unchanged, then V x 16 doubles of rig state {R, t of C_v, moved,
 *   pad}, then per group V x (32 + 36 + 36) + 8 doubles: {s_gv (32 each), W_gv, H_ee^-1 W_gv^T, then H_ee^-1 r_e (6), active, H_ee
 *   passed}.  8-byte aligned, no initialisation needed.  Three launches per iteration: the accumulate launch, one workgroup per group
 *   (the 6x6 work spread over 128 lanes), one workgroup of 256 lanes for the reduced system (S a packed triangle in LDS, one lane per
 *   row).  Float64, no atomics, fixed ascending order: a replay is bit-identical.  Argument errors as dim_icp_refine_views, and a
 *   NULL cam_T_rig_out, return DIM_ERR_ARG before anything is enqueued. */
int dim_views_from_rig(const float* pose_rig, const float* cam_T_rig, int G, int V, float* pose_views, void* stream);
int dim_views_consensus(const float* score, const int* status, int fatal_mask, const float* pose, const float* cam_T_rig, int G, int V,
                        int* choice, float* pose_rig, float* pose_views, int* status_out, void* stream);
long dim_icp_views_workspace_bytes(int B, int H, int W, int V);
int dim_icp_refine_views(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                         const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters, float max_dist,
                         void* workspace, float* pose_out, float* stats, int* status, const float* cam_T_rig, int V,
                         const float* pose_rig_in, float* pose_rig_out, float* stats_group, void* stream);
long dim_icp_rig_workspace_bytes(int B, int H, int W, int V);
int dim_icp_refine_rig(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                       const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters, float max_dist,
                       void* workspace, float* pose_out, float* stats, int* status, const float* cam_T_rig, int V,
                       const float* pose_rig_in, float* pose_rig_out, float* stats_group, float* cam_T_rig_out, float* stats_view,
                       void* stream);
long dim_photo_views_workspace_bytes(int B, int H, int W, int levels, int V);
int dim_photo_refine_views(const float* image_observed, const float* image_rendered, const float* depth_rendered, const int* bbox,
                           const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int levels, int iters,
                           float huber, float gate, int gain, void* workspace, float* pose_out, float* stats, int* status,
                           const float* cam_T_rig, int V, const float* pose_rig_in, float* pose_rig_out, float* stats_group, void* stream);
long dim_sil_views_workspace_bytes(int B, int H, int W, int V);
int dim_sil_refine_views(const float* depth_rendered, const int* field, const int* bbox, const float* pose_in, const float* K9,
                         const float* K_per_sample, int B, int H, int W, int iters, float huber_px, float max_px, void* workspace,
                         float* pose_out, float* stats, int* status, const float* cam_T_rig, int V, const float* pose_rig_in,
                         float* pose_rig_out, float* stats_group, void* stream);

/* ---------------------------------------------------------------- multi-hypothesis refinement (several starting poses per pair)
 * Samples are pair-major: sample b = p * N + h of P pairs with N hypotheses each.  Restated in float64 by tests/hyp_reference.py.
 * dim_hyp_expand: pose_out (P*N,3,4) from pose_in (P,3,4) and rot_table (N,3,3) device f32: pose_out[p*N+h] = [R_h R_p | t_p]
 *   (a rotation about the object origin in the camera frame, products in float64); h = 0 is a bit-exact copy (rot_table[0] is
 *   not read).
 * dim_hyp_broadcast: dst[(p*N+h) * row_words + k] = src[p * row_words + k] for 4-byte words (a plane, a K row, a class index):
 *   every pair's row into its N sample rows in one launch; float4 when row_words % 4 == 0 and both pointers are 16-byte aligned.
 * dim_pose_score: one score per sample over S = {pixels inside bbox[b] (B,4 int32 {min_x,max_x,min_y,max_y} inclusive, clipped to
 *   the frame; NULL = whole frame) with depth_rendered (B,1,H,W) > 0}:
 *     DIM_HYP_SCORE_RGB:   zero-mean normalised cross-correlation of a = sum_c image_observed and r = sum_c image_rendered
 *                          (both (B,3,H,W)), in [-1, 1];
 *     DIM_HYP_SCORE_DEPTH: among the pixels of S with depth_observed (B,1,H,W) > 0, the fraction with |D_r - D_o| < tau (metres).
 *   Fewer than 64 counted pixels, for RGB a plane that is constant over S, or a non-finite result give score[b] = -inf and OR
 *   DIM_STATUS_HYP_NO_SCORE into status[b] (B int32, may be NULL).  Sums: float64 per lane (shifted by the bbox's first pixel),
 *   across lanes, waves and workgroups in a fixed order, no atomics: a replay is bit-identical.  workspace:
 *   dim_pose_score_workspace_bytes(B, H, W) bytes, 8-byte aligned, no initialisation.  2 launches.
 * dim_hyp_select: per pair, choice[p] = the h of the largest finite score[p*N+h] (ties: the smaller h; none finite: 0, and
 *   DIM_STATUS_HYP_NO_SCORE is OR-ed into the selected last status row); then gathers poses_iter (T,P*N,3,4) -> poses_sel (T,P,3,4),
 *   status_iter (T,P*N) -> status_sel (T,P) int32 and pose_icp (P*N,3,4) -> pose_icp_sel (P,3,4) (each pair optional: NULL, NULL).
 *   status_load (P*N int32 or NULL): bits of the load-time hypothesis renders, OR-ed into the selected last status row (the loop
 *   rewrites status_iter, so they would be lost there).  One launch.
 * Bad sizes, an unknown mode, tau <= 0 for the depth score or a NULL required pointer return DIM_ERR_ARG before anything is enqueued. */
#define DIM_HYP_SCORE_RGB 0
#define DIM_HYP_SCORE_DEPTH 1
int dim_hyp_expand(const float* rot_table, const float* pose_in, int P, int N, float* pose_out, void* stream);
int dim_hyp_broadcast(void* dst, const void* src, int P, int N, long row_words, void* stream);
long dim_pose_score_workspace_bytes(int B, int H, int W);
int dim_pose_score(const float* image_observed, const float* image_rendered, const float* depth_observed, const float* depth_rendered,
                   const int* bbox, int B, int H, int W, int mode, float tau, void* workspace, float* score, int* status, void* stream);
int dim_hyp_select(const float* score, int P, int N, int T, const float* poses_iter, const int* status_iter, const int* status_load,
                   const float* pose_icp, int* choice, float* poses_sel, int* status_sel, float* pose_icp_sel, void* stream);

/* ---------------------------------------------------------------- coarse pose from a 2-D detection box (csrc/coarse.hip)
 * The front stage of a pipeline that starts from a detector: M candidate rotations per pair, each with the translation at which the
 * projected model fills the pair's box, all P*M rendered and scored against the pair's one observed frame, the k best of each pair
 * kept.  Samples are pair-major: sample b = p * M + m.  Restated in float64 by tests/coarse_reference.py.
 * dim_pose_from_box: pose_out (P*M,3,4) float32 = [R_m | t], rot_table (M,9) float32 device copied into the rotation entries, t fitted
 *   in float64 (pose_out_f64 (P*M,3,4) float64: the same before the rounding of t; may be NULL).
 *     points (Ntot,3) float64, table_off (n_classes+1) int32, class_index (P) int32: the tables of dim_pose_errors, one class per pair.
 *     boxes (P,4) float32 device = {x0, x1, y0, y1}: continuous pixel extents with pixel centres at integers, so the inclusive int box
 *     {min_x,max_x,min_y,max_y} is {min_x - 0.5, max_x + 0.5, min_y - 0.5, max_y + 0.5}.  K9_f64: HOST pointer, 9 doubles row-major, read
 *     before the call returns; K_per_sample (P,9) float64 device, one camera per pair, or NULL.
 *   With fx = K[0], fy = K[4], cx = K[2], cy = K[5], bw = x1 - x0, bh = y1 - y0, cu = (x0 + x1) / 2, cv = (y0 + y1) / 2 the fit starts
 *   at t = ((cu - cx) z_init / fx, (cv - cy) z_init / fy, z_init) and repeats `iters` times: project every model point of the class
 *   under [R_m | t] (the transform, then K row by row and two divisions: dim_pose_errors' order) to (u, v); umin, umax, vmin, vmax;
 *     s = ((umax - umin) / bw + (vmax - vmin) / bh) / 2;  tz' = tz s;  tx' = tx s + (cu - (umin + umax) / 2) tz' / fx;  ty' likewise.
 *   min / max do not depend on the order of the points: the result equals the numpy restatement bit for bit.
 *   DIM_STATUS_COARSE_BAD_BOX is OR-ed into status[b] (P*M int32, required) and the row becomes [R_m | (0, 0, z_init)] for: a
 *   non-finite box, x1 <= x0 or y1 <= y0; a class without points; at any iteration a point whose third projective row is not > 0, or a
 *   non-finite s.  A class index outside [0, n_classes) gives the same row and DIM_STATUS_BAD_CLASS.  A bad row leaves every other
 *   row as it would be without it.  One launch (one workgroup per candidate), nothing allocated, no synchronisation.
 *   P or M outside [1, 65535], iters < 1, z_init <= 0 or non-finite, n_classes <= 0 or a NULL required pointer return DIM_ERR_ARG
 *   before anything is enqueued.
 * dim_pose_score_indexed: dim_pose_score with the observed planes indexed: sample b reads row obs_row[b] (B int32 device) of
 *   image_observed / depth_observed (n_obs rows); image_rendered, depth_rendered and bbox stay per sample.  Terms, summation order,
 *   status bit and workspace are dim_pose_score's (with obs_row[b] = b it gives the same bits).  An index outside [0, n_obs) gives
 *   score -inf and DIM_STATUS_HYP_NO_SCORE.  dim_pose_score's argument errors, a NULL obs_row or n_obs < 1 return DIM_ERR_ARG.
 * dim_hyp_topk: per pair the k largest finite score[p*M+m] in descending order, ties to the smaller m; a candidate with
 *   status_in[p*M+m] & reject_mask (status_in: P*M int32 or NULL) counts as not finite.  idx_out (P,k) int32 = m, score_out (P,k),
 *   poses_out (P*k,3,4) gathered from poses_in (P*M,3,4), status_out (P*k) int32 = the candidate's status_in bits.  With fewer than k
 *   finite scores the remaining slots repeat slot 0 and get DIM_STATUS_HYP_NO_SCORE; with none every slot is candidate 0 with that
 *   bit.  One workgroup per pair, no atomics: a replay is bit-identical.  One launch.
 *   P or M outside [1, 65535], k outside [1, min(M, 64)] or a NULL required pointer return DIM_ERR_ARG before anything is enqueued. */
int dim_pose_from_box(const double* points, const int* table_off, int n_classes, const int* class_index, const float* rot_table,
                      const float* boxes, const double* K9_f64, const double* K_per_sample, int P, int M, int iters, double z_init,
                      float* pose_out, double* pose_out_f64, int* status, void* stream);
int dim_pose_score_indexed(const float* image_observed, const float* image_rendered, const float* depth_observed,
                           const float* depth_rendered, const int* bbox, const int* obs_row, int n_obs, int B, int H, int W, int mode,
                           float tau, void* workspace, float* score, int* status, void* stream);
int dim_hyp_topk(const float* score, const int* status_in, int reject_mask, int P, int M, int k, const float* poses_in, int* idx_out,
                 float* score_out, float* poses_out, int* status_out, void* stream);

/* ---------------------------------------------------------------- pose tracking through a video (csrc/track.hip)
 * The temporal layer around the refinement loop: P tracks share one camera, and their state lives on the device, so a frame costs no
 * host round trip.  Restated in float64 by tests/track_reference.py.  Each entry is one launch.
 * dim_track_ingest: one camera frame -> the observed blobs of the P tracks.  frame_bgr (H,W,3) uint8, depth_raw (H,W) uint16 or NULL;
 *   image_observed (P,3,H,W), depth_observed (P,1,H,W) or NULL (it needs depth_raw).  Every pixel has the bits dim_pair_blobs_from_raw
 *   writes: plane c = bgr[2 - c] - pixel_means_bgr3[2 - c] (HOST array), depth = raw / depth_factor as a true division.  The frame is
 *   read once and written P times in 16-byte stores.  W % 4 != 0, H <= 0, P <= 0, depth_factor <= 0, a NULL required pointer or a
 *   misaligned one (frame 4 bytes, raw depth 8, float planes 16) return DIM_ERR_ARG.
 * dim_track_predict: the pose each track's frame starts from.  hist (P,2,3,4): [1] the last accepted pose, [0] the one before; age (P)
 *   int32: the valid entries of hist (0, 1 or 2).  DIM_TRACK_MOTION_HOLD, age < 2, a non-finite entry of hist or tz <= 0 in either pose:
 *   pose_out = hist[1] bit for bit.  DIM_TRACK_MOTION_VELOCITY otherwise, in float64 with one rounding at the end:
 *     R_pred = exp(alpha log(R_last R_prev^T)) R_last;   u = tx / tz, v = ty / tz:  u_pred = u_last + alpha (u_last - u_prev), v likewise;
 *     z_pred = z_last (z_last / z_prev)^alpha;   t_pred = (u_pred z_pred, v_pred z_pred, z_pred)
 *   (the untangled translation of the network, T_transform).  The logarithm of D = R_last R_prev^T: s v = half the antisymmetric part
 *   of D as a vector (|v| = 1), c = (tr D - 1) / 2, angle = atan2(s, c); the axis is v for c >= -0.5 (log = s v itself when s < 1e-8),
 *   and for c < -0.5 it is taken from the symmetric part, (D + D^T) / 2 = c I + (1 - c) a a^T (row of the largest diagonal entry,
 *   normalised, signed like v): stable at angle 0 and up to pi.  mode outside the two, alpha outside [0, 1], P <= 0 or a NULL pointer
 *   return DIM_ERR_ARG.
 * dim_track_update: the state machine after a frame's refinement, per track, in float64, in this order:
 *   1. step = (angle of R_new R_before^T in degrees, atan2 form as above; |t_new - t_before|), +inf where not finite; pose_before is the
 *      pose before the loop's last iteration, pose_new the tracked pose (both (P,3,4)).
 *   2. the step overwrites the oldest entry of ring (P,Wn,2) at ring_pos, ring_n = min(ring_n + 1, Wn); mean (P,2) = the mean of the
 *      ring_n stored entries, summed oldest first.
 *   3. lost = (status & fatal_mask) != 0, status the OR of status_rows (n_rows,P) int32 (NULL with n_rows 0); or a non-finite entry of
 *      pose_new; or t_z outside [znear, zfar]; or score (P, may be NULL) with !(score >= min_score); or ring_n == Wn and (mean_rot >
 *      lost_rot_deg or mean_trans > lost_trans_m).
 *   4. not lost: hist[0] = hist[1], hist[1] = pose_new, age = min(age + 1, 2).
 *   5. lost and reinit_valid[p] != 0: hist[1] = reinit_pose[p], age = 1, ring zeroed with ring_n = ring_pos = 0, flags gain
 *      DIM_STATUS_TRACK_LOST | DIM_STATUS_TRACK_REINIT.  reinit_pose (P,3,4) / reinit_valid (P) int32 may both be NULL (nothing offered).
 *   6. lost otherwise: hist and ring unchanged, age = min(age, 1), flags gain DIM_STATUS_TRACK_LOST.
 *   flags (P) int32 = status plus the new bits; step (P,2) and mean (P,2) float32.  Poses enter hist as bit-for-bit copies.
 *   Wn outside [1, DIM_TRACK_MAX_WINDOW], P <= 0, n_rows < 0 or a NULL required pointer return DIM_ERR_ARG. */
#define DIM_TRACK_MOTION_HOLD 0
#define DIM_TRACK_MOTION_VELOCITY 1
#define DIM_TRACK_MAX_WINDOW 64
int dim_track_ingest(const unsigned char* frame_bgr, const unsigned short* depth_raw, int P, int H, int W, float depth_factor,
                     const float* pixel_means_bgr3, float* image_observed, float* depth_observed, void* stream);
int dim_track_predict(const float* hist, const int* age, int P, int mode, float alpha, float* pose_out, void* stream);
int dim_track_update(const float* pose_before, const float* pose_new, const int* status_rows, int n_rows, int fatal_mask,
                     const float* score, float min_score, const float* reinit_pose, const int* reinit_valid, float lost_rot_deg,
                     float lost_trans_m, int Wn, float znear, float zfar, int P, float* hist, int* age, float* ring, int* ring_n,
                     int* ring_pos, int* flags, float* step, float* mean, void* stream);
/* Occlusion between the tracks and against the frame's depth.  Restated by tests/track_occ_reference.py.
 * dim_track_visibility: depth_rendered (P,1,H,W): the P tracks' renders at one camera; depth_frame (H,W) metres or NULL; occluder_ok
 *   (P) int32 or NULL (all 1); mode = DIM_TRACK_OCC_TRACKS | DIM_TRACK_OCC_DEPTH (one or both); delta >= 0 metres.  Per pixel and
 *   track p with rendered depth d_p, every comparison in float32:
 *     drawn_p           = 0 < d_p < +inf (NaN, +inf, 0 and negatives are not drawn)
 *     hidden_by_track_p = DIM_TRACK_OCC_TRACKS and some q != p with drawn_q, occluder_ok[q] != 0 and d_p - d_q > delta (computed as
 *                         d_p - m_p > delta, m_p the smallest such d_q: the subtraction is monotone)
 *     hidden_by_depth_p = DIM_TRACK_OCC_DEPTH, o = depth_frame[pixel] with 0 < o < +inf, and d_p - o > delta (a pixel without a
 *                         reading hides nothing)
 *   depth_visible (P,1,H,W) = the bits of d_p where drawn and not hidden, else +0.0: passed to dim_pose_score as depth_rendered it
 *   restricts the score's support to the visible pixels.  counts (P,4) int32 = {drawn, visible, hidden by a track, hidden by the
 *   frame's depth only}; the first is the sum of the other three.  No output needs initialising; integer sums, so a second call gives
 *   the same bits.  workspace: dim_track_visibility_workspace_bytes(P, H, W) bytes, 4-byte aligned, no initialisation needed.  Any W;
 *   16-byte accesses when W % 4 == 0 and depth_rendered, depth_visible and depth_frame are 16-byte aligned.  2 launches.
 *   P, H or W <= 0, mode 0 or with an unknown bit, DIM_TRACK_OCC_DEPTH with a NULL depth_frame, a negative or non-finite delta or a
 *   NULL required pointer return DIM_ERR_ARG before anything is enqueued.
 * dim_track_update_occ: dim_track_update with an occluded state: the same kernel body, in which rules 1 to 6 stand once, built a second
 *   time with the state in front of rules 2 to 6.  Additional inputs: counts (P,4) of dim_track_visibility for the render of pose_new,
 *   min_visible in [0,1], max_occluded >= 0, pose_pred (P,3,4) the pose the frame started from; additional state occ_age (P) int32: the
 *   frames the track has coasted in a row.  Per track, in this order:
 *   a. step as in rule 1.  fatal = the first three clauses of rule 3 (a fatal status bit, a non-finite pose_new, t_z out of range).
 *   b. visible[p] = float(double(counts[1]) / double(counts[0])), 0 when nothing is drawn.
 *      occluded = not fatal, counts[0] > 0 and double(counts[1]) < double(min_visible) * counts[0].
 *   c. not occluded: rules 2 to 6 as they stand above, and occ_age = 0.
 *   d. occluded: flags gain DIM_STATUS_TRACK_OCCLUDED; the step does not enter the ring, and mean is the mean of what the ring holds
 *      (0 when it holds nothing); the score and window tests are skipped.  With occ_age < max_occluded and a finite pose_pred with t_z
 *      in [znear, zfar] the track coasts: hist[0] = hist[1], hist[1] = pose_pred bit for bit, age = min(age + 1, 2), occ_age += 1,
 *      ring, ring_n and ring_pos untouched.  Otherwise it is lost by rules 5 and 6, and occ_age = 0.
 *   Then pose_track (P,3,4) = hist[1] (the accepted pose, the coasted prediction, the offered pose or the last accepted pose of a lost
 *   track) and occluder_ok (P) int32 = 0 for a track that is lost and not re-initialised on this frame, else 1.  With min_visible = 0,
 *   or counts[1] == counts[0], every tensor the two entries share gets the bits dim_track_update gives it.  min_visible outside [0, 1],
 *   max_occluded < 0 and dim_track_update's own cases return DIM_ERR_ARG. */
#define DIM_TRACK_OCC_TRACKS 1
#define DIM_TRACK_OCC_DEPTH 2
long dim_track_visibility_workspace_bytes(int P, int H, int W);
int dim_track_visibility(const float* depth_rendered, const float* depth_frame, const int* occluder_ok, int P, int H, int W, int mode,
                         float delta, void* workspace, float* depth_visible, int* counts, void* stream);
int dim_track_update_occ(const float* pose_before, const float* pose_new, const int* status_rows, int n_rows, int fatal_mask,
                         const float* score, float min_score, const float* reinit_pose, const int* reinit_valid, float lost_rot_deg,
                         float lost_trans_m, int Wn, float znear, float zfar, int P, const int* counts, float min_visible,
                         int max_occluded, const float* pose_pred, float* hist, int* age, float* ring, int* ring_n, int* ring_pos,
                         int* occ_age, int* flags, float* step, float* mean, float* visible, float* pose_track, int* occluder_ok,
                         void* stream);
/* Colour-histogram segmentation of the tracks (csrc/track_seg.hip): a mask per track and frame from foreground / background colour
 * histograms that are carried from frame to frame.  Restated by tests/track_seg_reference.py.
 * Colour bin of a frame pixel with bytes (b, g, r) in frame_bgr (H,W,3) uint8: c = ((b >> s) << 2*bits) | ((g >> s) << bits) | (r >> s)
 *   with s = 8 - bits, bits in 1..5; NB = 1 << 3*bits bins.
 * Region of track p: bbox[p] = {min_x, max_x, min_y, max_y} (inclusive, as dim_raster_render* returns it) grown by margin >= 0 pixels
 *   on every side and clipped to the frame: x in [max(min_x - margin, 0), min(max_x + margin, W - 1)], y likewise (in 64-bit
 *   arithmetic: any int32 box is safe).  A box with max < min on either axis, or one that is empty after clipping, has no region.
 * State: seg_hist (P,2,NB) float32, row 0 the foreground and row 1 the background histogram (each sums to about 1); seg_age (P) int32,
 *   the number of updates, 0 = no model.
 * dim_track_seg_mask (before the loop, on the box of the start render):
 *   raw(p,x,y) = 1 when (x,y) is in the region of p, seg_age[p] > 0 and seg_hist[p,0,c] > seg_hist[p,1,c] as a float32 comparison (a
 *   tie or a NaN is background), else 0.  mask[p,0,y,x] = 1.0f when the pixel is in the region and
 *   2 * sum_{|dx|,|dy| <= radius} raw(p, x+dx, y+dy) > (2*radius+1)^2 (neighbours outside the region count 0), else 0.0f: an integer
 *   majority filter, so the result is exact; radius in 0..4, radius 0 gives raw.  Every word of mask (P,1,H,W) is written.  counts
 *   (P,2) int32 = {region pixels, mask pixels}.  DIM_STATUS_TRACK_SEG_NO_MODEL is OR-ed into status[p] (P int32, may be NULL) when the
 *   track has no model (seg_age <= 0) or no region; its mask is then all 0.  2 launches.
 * dim_track_seg_learn (after the update, on the render of the tracked pose): depth_drawn (P,1,H,W) the track's own render, depth_fg
 *   (P,1,H,W) or NULL (= depth_drawn; with occlusion reasoning: depth_visible), bbox (P,4) of that render, flags (P) int32 or NULL.
 *   Inside the region a pixel is foreground when 0 < depth_fg < +inf; else background when depth_drawn is not in (0, +inf); else (drawn
 *   but hidden) neither.  Other tracks' pixels are background of p: they are what p is seen against.  counts (P,2) int32 = {n_f, n_b},
 *   always written.  A track is skipped, its rows of seg_hist and its seg_age left bit for bit, when flags[p] & skip_mask != 0,
 *   n_f < min_pixels or n_b < min_pixels.  Otherwise h_k[c] = float32(count_k[c]) / float32(n_k) (IEEE division; the counts are exact
 *   in float32 because H*W <= 1 << 24); with seg_age <= 0 seg_hist = h, else seg_hist = seg_hist + rate * (h - seg_hist) in float32,
 *   subtraction, multiplication and addition each rounded once (no fused multiply-add); seg_age = min(max(seg_age, 0) + 1, 1 << 30).
 *   4 launches.
 * Atomics: the other stages avoid them because a float sum depends on the order of its terms.  Here every sum is an integer (bin
 *   counts, pixel counts), so integer atomicAdd is used -- per-block LDS sub-histograms flushed by global atomics up to bits = 3, global
 *   atomics with equal bins of a wave merged first above --, the result does not depend on the order and a replay gives the same bits.
 *   The counting workspace is cleared by the entry's own kernels (no memset node: the chain is captured "kernels only").
 * Both: any W; 16-byte accesses of the float planes (and 12-byte ones of the frame) when W % 4 == 0, the planes are 16-byte and the
 *   frame is 4-byte aligned.  workspace: dim_track_seg_workspace_bytes bytes (0 for bad arguments), 16-byte aligned, no
 *   initialisation needed; the two entries use disjoint parts of it.  P, H or W <= 0, P > 65535, H*W > 1 << 24, bits outside 1..5, radius
 *   outside 0..4, margin < 0, rate outside [0,1] or not finite, min_pixels < 1, a NULL required pointer or a float / int pointer that
 *   is not 4-byte aligned return DIM_ERR_ARG before anything is enqueued. */
long dim_track_seg_workspace_bytes(int P, int H, int W, int bits);
int dim_track_seg_mask(const unsigned char* frame_bgr, const int* bbox, const float* seg_hist, const int* seg_age, int P, int H, int W,
                       int bits, int margin, int radius, void* workspace, float* mask, int* counts, int* status, void* stream);
int dim_track_seg_learn(const unsigned char* frame_bgr, const float* depth_drawn, const float* depth_fg, const int* bbox,
                        const int* flags, int skip_mask, int P, int H, int W, int bits, int margin, float rate, int min_pixels,
                        void* workspace, float* seg_hist, int* seg_age, int* counts, void* stream);

/* ---------------------------------------------------------------- pose errors of the evaluation (lib/utils/pose_error.py) on the device
 * For T pose sets of B pairs: errors (T,B,5) float64 = {re (degrees), te, add, adi, arp_2d} of poses_est[t][b] against pose_gt[b]
 * (B,3,4) float64, computed in float64 with numpy's operations in numpy's order (sums of the means in a fixed tree instead of
 * numpy's pairwise one: ~1e-13 relative at 500 points).
 *   points (Ntot,3) float64 device: the model points of all classes concatenated; table_off (n_classes+1) int32 device: class c owns
 *   points [table_off[c], table_off[c+1]); class_flags (n_classes) int32 device: DIM_POSE_ERR_ADI fills the adi column of the class
 *   (NaN without it), DIM_POSE_ERR_FLIP_Z180 is the eggbox rule of lib/dataset/evaluation.py: when the raw rotation error exceeds
 *   90 degrees, re, te and arp_2d are those of est . RT_Z = [R diag(-1,-1,1) | t]; add and adi always use the estimate itself.
 *   class_index (B) int32 device.  poses_est (T,B,3,4) float32 as the loop leaves it, or poses_est_f64 the same in float64: exactly
 *   one of the two is non-NULL.  K9_f64: HOST pointer, 9 doubles row-major, read before the call returns.
 *   add = mean |(R_e p + t_e) - (R_g p + t_g)|; adi = mean over the ground-truth points of the distance to the nearest estimate
 *   point, by exhaustive search (no tree, no float32 stage); arp_2d = mean pixel distance of the projections K (R p + t).
 * A class index outside [0, n_classes) gives a NaN row and ORs DIM_STATUS_BAD_CLASS into status[b] (B int32, may be NULL); a class
 * without points gives a NaN row.  A non-finite pose gives non-finite values in its own row only.
 * workspace: dim_pose_errors_workspace_bytes(T, B, max_points) bytes, 8-byte aligned, no initialisation needed (max_points: the
 * largest class; the candidates are staged in LDS, so it does not enter the size).  Sums: float64 per lane, across lanes, waves and
 * workgroups in a fixed order, no atomics: a second call is bit-identical.  2 launches, nothing allocated, no synchronisation.
 * T or B outside [1, 65535], n_classes <= 0, both or neither pose pointers, or a NULL required pointer return DIM_ERR_ARG before
 * anything is enqueued. */
#define DIM_POSE_ERR_ADI 1
#define DIM_POSE_ERR_FLIP_Z180 2
long dim_pose_errors_workspace_bytes(int T, int B, int max_points);
int dim_pose_errors(const double* points, const int* table_off, const int* class_flags, int n_classes, const int* class_index,
                    const float* poses_est, const double* poses_est_f64, const double* pose_gt, const double* K9_f64, int T, int B,
                    void* workspace, double* errors, int* status, void* stream);

/* ---------------------------------------------------------------- visible surface discrepancy (VSD) on the device
 * The error the reference ships the two halves of (lib/utils/visibility.py: estimate_visib_mask, _gt, _est; lib/utils/misc.py:
 * depth_im_to_dist_im) and never joins; restated in numpy by lib/utils/pose_error.py vsd().  For T pose sets of B pairs:
 *   depth_obs (B,H,W) the observed depth, depth_gt (B,H,W) the model rendered at the ground truth, depth_est (T,B,H,W) the model
 *   rendered at the estimates; float32 metres, 0 = no surface.  Camera: K_per_sample_f64 (B,9) device float64 or NULL = K9_f64 (HOST,
 *   9 doubles row-major, read before the call returns) for every pair.
 *   Per pixel (x, y), in float64: S = sqrt((X X + Y Y) + d d), X = ((x - cx) d) (1 / fx), Y = ((y - cy) d) (1 / fy) for each of the
 *   three depths.  visible(S_m) = S_m > 0 and S_obs > 0 and float32(S_m) - float32(S_obs) <= delta, compared in float32.
 *   visib_gt = visible(S_gt); visib_est = visible(S_est) or (visib_gt and S_est > 0).  On visib_gt & visib_est the cost of
 *   c = |S_gt - S_est| is (c >= tau) for DIM_VSD_COST_STEP and min(c (1 / tau), 1) for DIM_VSD_COST_TLINEAR; then
 *   e = (sum of costs + (|union| - |inter|)) / |union|, and e = 1 when the union is empty.  A NaN depth fails every `> 0`.
 *   taus: HOST, n_tau doubles (1 <= n_tau <= DIM_VSD_MAX_TAU), all scored from one read of the planes.
 *   errors (T,B,n_tau) float64; counts (T,B,4) int32 = {|visib_gt|, |union|, |inter|, pixels with S_gt > 0}.
 *   bbox_gt (B,4) / bbox_est (T,B,4) int32 device {min_x, max_x, min_y, max_y} (empty = {W,-1,H,-1}) as the rasteriser returns them for
 *   the two renders, both or neither: rows and columns outside their union are not read.  Both renders are 0 there, so the result is
 *   the one of NULL boxes bit for bit (a pixel keeps its lane and its place in the lane's sum).
 * workspace: dim_vsd_workspace_bytes(T, B) bytes, 8-byte aligned, no initialisation needed.  Sums: int32 / float64 per lane, float64
 * across lanes and workgroups in a fixed order, no atomics: a second call is bit-identical.  16-byte loads when W % 4 == 0 and the
 * planes are 16-byte aligned.  2 launches, nothing allocated, no synchronisation.  T or B outside [1, 65535], H or W <= 0, n_tau
 * outside [1, 8], an unknown cost_type, one box without the other or a NULL required pointer return DIM_ERR_ARG before anything is
 * enqueued. */
#define DIM_VSD_MAX_TAU 8
#define DIM_VSD_COST_STEP 0
#define DIM_VSD_COST_TLINEAR 1
long dim_vsd_workspace_bytes(int T, int B);
int dim_vsd_errors(const float* depth_obs, const float* depth_gt, const float* depth_est, const double* K9_f64,
                   const double* K_per_sample_f64, const int* bbox_gt, const int* bbox_est, int T, int B, int H, int W, float delta,
                   const double* taus, int n_tau, int cost_type, void* workspace, double* errors, int* counts, void* stream);

/* The step cost on BOP's grid: up to DIM_VSD_GRID_MAX_TAU taus per pair, read from the row of the pair's class in a device table
 * (BOP: ten fractions of the class diameter), scored from one read of the planes.  Planes, cameras, boxes, the visibility rule,
 * c = |S_gt - S_est| and counts (T,B,4) are those of dim_vsd_errors.
 *   class_index (B) int32 device; tau_table (n_classes, n_tau) float64 device, metres: the products are made on the host, the device
 *   only compares.  n_ge (T,B,n_tau) int32 = the pixels of the intersection with c >= tau_table[class_index[b]][k];
 *   errors (T,B,n_tau) float64 = ((double)n_ge + (double)(|union| - |inter|)) / (double)|union|, one division, and 1 when the union is
 *   empty: the bits of lib/utils/pose_error.py vsd(..., "step").
 * A class index outside [0, n_classes) gives its rows NaN errors, zero counts and zero n_ge and touches nothing else.
 * workspace: dim_vsd_grid_workspace_bytes(T, B) bytes, 8-byte aligned, no initialisation needed.  Every sum is int32 (H W < 2^31):
 * wave shuffles, LDS across waves, a finish kernel across workgroups that reads only what this call wrote; no atomics and no float
 * sum, so the result does not depend on how the pixels are dealt out.  2 launches, nothing allocated, no synchronisation.  T or B
 * outside [1, 65535], H or W <= 0, n_tau outside [1, 16], n_classes < 1, one box without the other, a misaligned workspace or a NULL
 * required pointer return DIM_ERR_ARG before anything is enqueued. */
#define DIM_VSD_GRID_MAX_TAU 16
long dim_vsd_grid_workspace_bytes(int T, int B);
int dim_vsd_grid_errors(const float* depth_obs, const float* depth_gt, const float* depth_est, const double* K9_f64,
                        const double* K_per_sample_f64, const int* bbox_gt, const int* bbox_est, const int* class_index,
                        const double* tau_table, int n_classes, int n_tau, int T, int B, int H, int W, float delta, void* workspace,
                        double* errors, int* counts, int* n_ge, void* stream);

/* ---------------------------------------------------------------- BOP symmetry-aware pose errors (MSSD, MSPD) on the device
 * lib/utils/pose_error.py mssd / mspd for T pose sets of B pairs: errors (T,B,2) float64 = {mssd, mspd} of poses_est[t][b] against
 * pose_gt[b] (B,3,4) float64 under the symmetry set of the pair's class,
 *   mssd = min over S of max over x of |(R_e x + t_e) - (R_g (S_R x + S_t) + t_g)|      (the unit of the model points)
 *   mspd = the same with both points projected by K (R p + t) and divided by the third row   (pixels)
 * computed in float64 with numpy's operations in numpy's order, except that pose_gt . S is composed once per (pose, symmetry) and
 * applied to the point in one step (about 1e-16 relative against transforming the point twice).
 *   points, table_off: the tables of dim_pose_errors.  sym (Stot,3,4) float64 device: the symmetry transformations [S_R | S_t] of all
 *   classes concatenated; sym_off (n_classes+1) int32 device: class c owns sym [sym_off[c], sym_off[c+1])
 *   (lib/utils/symmetry.py, PoseEvaluator.device_sym_tables).  class_index (B) int32 device.  poses_est (T,B,3,4) float32 as the loop
 *   leaves it, or poses_est_f64 the same in float64: exactly one of the two is non-NULL.  Camera: K_per_sample_f64 (B,9) device
 *   float64 or NULL = K9_f64 (HOST, 9 doubles row-major, read before the call returns) for every pair.
 *   best_sym (T,B,2) int32 (may be NULL): the index within the class's set that attains each minimum; ties go to the smaller index.
 * A class index outside [0, n_classes) gives a NaN row with best_sym -1 and ORs DIM_STATUS_BAD_CLASS into status[b] (B int32, may be
 * NULL); a class without points, without symmetries or with more than max_sym symmetries gives a NaN row with best_sym -1.  A
 * non-finite pose or a point at depth <= 0 gives what numpy gives (a NaN wins the maximum over the points and the minimum over the
 * symmetries, best_sym = the first such symmetry), in its own row only.
 * workspace: dim_bop_errors_workspace_bytes(T, B, max_sym) bytes, 8-byte aligned, no initialisation needed.  Maxima per lane, wave
 * and workgroup, then the minimum: exact in any order, no atomics: a second call is bit-identical and the result does not depend on
 * how the points are dealt to workgroups.  2 launches, nothing allocated, no synchronisation.
 * T or B outside [1, 65535], n_classes <= 0, max_sym <= 0, both or neither pose pointers, or a NULL required pointer return
 * DIM_ERR_ARG before anything is enqueued. */
long dim_bop_errors_workspace_bytes(int T, int B, int max_sym);
int dim_bop_errors(const double* points, const int* table_off, const double* sym, const int* sym_off, int n_classes,
                   const int* class_index, const float* poses_est, const double* poses_est_f64, const double* pose_gt,
                   const double* K9_f64, const double* K_per_sample_f64, int T, int B, int max_sym, void* workspace, double* errors,
                   int* best_sym, int* status, void* stream);

/* ---------------------------------------------------------------- data layer (test batches from raw file pixels)
 * The loader uploads what the image files hold -- obs_bgr / ren_bgr (B,H,W,3) uint8 in B,G,R order (cv2.IMREAD_COLOR), depth_rendered
 * (B,H,W) uint16 = metres * depth_factor -- and the blobs of get_data_pair_test_batch are built on the device:
 * image_observed / image_rendered (B,3,H,W) = RGB planes minus PIXEL_MEANS (given in config order B,G,R: lib/utils/image.py:709-720),
 * mask_rendered (B,1,H,W) = depth with values above mask_thr replaced by 1 (:478-488), bbox (B,4) {min_x,max_x,min_y,max_y} of
 * depth > mask_thr for dim_box_mask (TEST.INIT_MASK box_rendered, :437-460).  Any output (and its input) may be NULL.  W % 4 == 0. */
int dim_test_blobs_from_raw(const unsigned char* obs_bgr, const unsigned char* ren_bgr, const unsigned short* depth_rendered, int B, int H,
                            int W, float depth_factor, const float* pixel_means_bgr3, float mask_thr, float* image_observed,
                            float* image_rendered, float* mask_rendered, int* bbox, void* stream);

/* The general form for training AND test batches: reference lib/pair_matching/data_pair.py:22-72 (test) / :144-265 (train) through
 * lib/utils/image.py get_pair_image :65-183, get_gt_observed_depth :186-207, get_pair_depth :210-269, get_pair_mask :272-491.
 * Raw inputs, all (B,H,W[,3]) as the files hold them, any may be NULL (its outputs are then skipped):
 *   obs_bgr / ren_bgr uint8 BGR; bg_bgr uint8 BGR = the VOC background already fitted to (H,W) (image.py:125-165) -- pasted where the
 *   label image is 0 for samples with use_bg[b] != 0 (use_bg NULL: all), :166-173; depth_ren / depth_a / depth_b uint16 = metres *
 *   depth_factor; label uint8 label image with mask_idx (B) the object's label value.
 * Outputs: image_observed / image_rendered (B,3,H,W); mask_rendered (B,1,H,W) = depth with > mask_thr replaced by 1; depth_rendered,
 * depth_a_out, depth_b_out (B,1,H,W) metres; mask_label = (label == mask_idx), label_raw = (float)label (TRAIN.INIT_MASK 'mask_gt' feeds
 * the RAW label image, image.py:315-316); bbox_ren / bbox_label (B,4) {min_x,max_x,min_y,max_y} of depth > mask_thr / of mask_label for
 * dim_box_mask (INIT_MASK box_rendered / box_gt / box_gt_observed / box_).  W % 4 == 0. */
int dim_pair_blobs_from_raw(const unsigned char* obs_bgr, const unsigned char* bg_bgr, const int* use_bg, const unsigned char* ren_bgr,
                            const unsigned short* depth_ren, const unsigned short* depth_a, const unsigned short* depth_b,
                            const unsigned char* label, const int* mask_idx, int B, int H, int W, float depth_factor,
                            const float* pixel_means_bgr3, float mask_thr, float* image_observed, float* image_rendered,
                            float* mask_rendered, float* depth_rendered, float* depth_a_out, float* depth_b_out, float* mask_label,
                            float* label_raw, int* bbox_ren, int* bbox_label, void* stream);
/* mask_dilate (lib/utils/mask_dilate.py:10-55) with the random draws made by the caller: thickness4 (B,4) = {down, up, right, left}
 * displacement of the boundary copies, 0 = side skipped.  mask_out != mask_in. */
int dim_mask_dilate(const float* mask_in, const int* thickness4, float* mask_out, int B, int H, int W, void* stream);
/* Photometric augmentation of observed training images (csrc/augment.hip), one pass over the blob, the draws made by the caller
 * (lib/utils/augment.py) as for mask_dilate.  in, out: image_observed blobs (B,3,H,W) float32, mean-subtracted, plane c = BGR channel
 * 2 - c (plane 0 is red); pixel_means_bgr3 (host) = network.PIXEL_MEANS.  The kernel works on grey levels v = in + mean of the plane, all
 * in float32 with every product and every sum rounded (no fused multiply-add), for pair b in this order:
 *   on[b] == 0     out is a copy of in, bit for bit; nothing below applies
 *   blur           radius r = radius_host[b] in 0..7 (HOST array) and taps[b] (device, B x 15, the first 2 r + 1 used, normalised by the
 *                  caller): separable, rows first, then columns of the row-blurred values; coordinates clamped to the image
 *                  (replicate border); each 1-D sum starts at 0 and is accumulated in ascending tap order, acc = acc + w * v;
 *                  r = 0 skips both passes (no multiplication by 1)
 *   saturation s   gray = 0.299 R + 0.587 G + 0.114 B (float32 constants, summed left to right), v_c = gray + s * (v_c - gray)
 *   contrast k, brightness d (grey levels)   v_c = (v_c - 128) * k + 128 + d, left to right
 *   gain g_c       v_c = v_c * g_c, c the blob plane (white balance)
 *   noise sigma    v_c = v_c + sigma * n(seed[b], (c * H + y) * W + x); sigma == 0 skips the addition.  With uint32 arithmetic
 *                  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *                  h0 = mix(seed + counter * 0x9E3779B9), h1 = mix(h0 ^ 0x85EBCA6B),
 *                  n = (float)((h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070) * 2.6428997e-05f  (unit variance,
 *                  within +-3.4642)
 *   clamp to [0, 255]; with quantize != 0 rintf (half to even); out = v_c - mean
 * chain[b] (device, B x 7) = {s, k, d, g_0, g_1, g_2, sigma}; on (B) int32 and seed (B) uint32 are device arrays.
 * No workspace.  in and out must not overlap (the halo of one tile is another tile's output) and are 16-byte aligned; W % 4 == 0.
 * A NULL pointer, B, H or W <= 0, W % 4 != 0, overlapping or misaligned blobs or a radius outside 0..7 return DIM_ERR_ARG with a
 * message before anything is enqueued. */
int dim_augment_observed(const float* in, float* out, int B, int H, int W, const float* pixel_means_bgr3, const int* on,
                         const int* radius_host, const float* taps, const float* chain, const unsigned* seed, int quantize, void* stream);
/* Contour overlays for test --vis (csrc/vis.hip): the outlines of L layers blended over an observed frame, one pass, a finished 8-bit
 * frame out.  image: an image_observed blob (B,3,H,W) float32, mean-subtracted, plane c = BGR channel 2 - c, as dim_augment_observed
 * takes it; pixel_means_bgr3 (host).  layers (L,B,H,W) float32: a pixel is INSIDE layer l where its value is > 0 (a NaN is not inside):
 * rendered depth and a 0/1 mask both qualify.  style (host, L x 5 ints) = {B, G, R, edge_alpha, fill_alpha} per layer, colours 0..255,
 * alphas 0..256; it travels as kernel arguments.  out_bgr (B,H,W,3) uint8 in B,G,R order, as an image file holds it.  The rules:
 *   base colour   per channel v = image + mean (one float32 add), rintf (half to even), clamp to [0, 255]; a NaN gives 0
 *   edge pixel    of layer l: the pixel is inside, and at least one of its 4-neighbours that lies inside the frame is not inside.
 *                 Neighbours outside the frame are ignored: an object cut by the frame has no outline along the frame border and a
 *                 1 x 1 frame has no edge (the contour-point rule of dim_sil_refine)
 *   marked pixel  of layer l: some edge pixel of l lies in the (2 radius + 1)^2 square centred on the pixel, clipped to the frame
 *   painting      the layers in the order l = 0 .. L-1, each over the result of the one before it: a marked pixel blends the layer's
 *                 colour with edge_alpha; a pixel that is inside, not marked and has fill_alpha > 0 blends it with fill_alpha; any
 *                 other pixel is unchanged
 *   blend         per channel in integers: c' = (c (256 - a) + colour a + 128) >> 8  (a = 0 returns c, a = 256 the colour)
 * counts (B,L,2) int32 or NULL: per pair and layer {marked pixels, inside pixels}; what it held before the call does not matter (it is
 * zeroed on the stream first; integer atomics, exact in any order).  No workspace.  Any W; with W % 4 == 0 and 16-byte aligned image and
 * layers the kernel moves whole words of four pixels.
 * L outside 1..8, radius outside 0..3, B outside 1..65535, H or W outside 1..32767, a colour outside 0..255 or an alpha outside 0..256,
 * a NULL required pointer, or out_bgr overlapping image or layers return DIM_ERR_ARG with a message before anything is enqueued. */
int dim_vis_overlay(const float* image, const float* pixel_means_bgr3, const float* layers, int L, const int* style, int radius, int B,
                    int H, int W, unsigned char* out_bgr, int* counts, void* stream);
/* First-iteration flow labels = calc_flow (lib/pair_matching/flow.py:12-81; float64 per pixel like numpy) + the weights of
 * get_pair_flow (image.py:531-545).  depth_src = rendered depth, depth_tgt = observed depth (B,1,H,W) metres; P12 (B,3,4) float64 (device) =
 * K se3_mul(pose_tgt, se3_inverse(pose_src)) as the reference forms it on the host; Kinv9_f64 = inv(K) in float64 (host pointer).
 * weight_type 0 all / 1 viz / 2 valid; flow (B,2,H,W) in "[h, w]" order unless standard_rep; flow_weights (B,2,H,W) or NULL. */
int dim_calc_flow_labels(const float* depth_src, const float* depth_tgt, const double* P12, const double* Kinv9_f64, int B, int H, int W,
                         double thresh, int standard_rep, int weight_type, float* flow, float* flow_weights, void* stream);
/* Point-matching labels (image.py:559-600): model[b,:,j] = table[table_off[b] + idx[b,j]] (idx < 0: zero-padded slot, weight 0),
 * weights (B,3,n), observed = R_obs model + t_obs.  table (N,3) = the points.xyz of all classes concatenated. */
int dim_point_clouds(const float* table, const int* table_off, const int* idx, const float* pose_observed, int B, int n, float* model,
                     float* weights, float* observed, void* stream);

/* ---------------------------------------------------------------- rasteriser
 * Mesh table in HBM: verts (sumV,3), uvs (sumV,2), faces (sumF,3 int32, indices local to the mesh),
 * mesh_table (C,4 int32) = {vert_off, nvert, face_off, nface}; textures = concatenated uint8 RGB images
 * (row 0 = top of texture_map.png), tex_table (C,3 int32) = {byte_off, Ht, Wt}.
 * class_index (B int32) in [0, n_classes), poses (B,3,4).  workspace: dim_raster_workspace_bytes(), 8-byte aligned (16 for the fast
 * resolve); its first 256 bytes are a header that remembers "the z-buffer behind me is clear" from one render to the next (no clear
 * pass): the OWNER ZEROES THOSE 256 BYTES when the memory is allocated or has been used for anything else.  (header, z-buffer, projected vertices,
 * covered-pixel list).  status (B int32, may be NULL): DIM_STATUS_BAD_CLASS / DIM_STATUS_BAD_FACE are OR-ed in.
 * Outputs (each may be NULL): image (B,3,H,W) = RGB - plane_means3 (the next iteration's image_rendered
 * blob), depth (B,1,H,W) metres, mask (B,1,H,W) = depth > mask_thr, bgr (B,H,W,3) as Render_Py.render
 * returns it, bbox (B,4) of the mask.   Replaces render_py_multi.py:112-147 + tester.py:563-578. */
long dim_raster_workspace_bytes(int B, int vmax, int H, int W);
int dim_raster_render(const float* verts, const float* uvs, const int* faces, const int* mesh_table, int n_classes, int vmax, int fmax,
                      const unsigned char* textures, const int* tex_table, const int* class_index, const float* poses,
                      const float* K9, int B, int H, int W, float znear, float zfar, int tex_bilinear, const float* plane_means3,
                      float mask_thr, void* workspace, float* image, float* depth, float* mask, float* bgr, int* bbox, int* status,
                      void* stream);
/* Lit variant of dim_raster_render: Render_Py_Light_ModelNet_Multi.render
 * (lib/render_glumpy/render_py_light_modelnet_multi.py:36-77 fragment shader, :153-235 render).
 * normals: per-vertex normals in the same table as verts.  light_pos (B,3) in GL camera coordinates, light_int (B,3)
 * (device pointers).  Colour = texel/255 * ((1-ratio) + ratio*clamp(cos(normal, light-position),0,1)) * light_int,
 * clamped to [0,1] and quantised to 8 bits (round to nearest) like the GL framebuffer. */
int dim_raster_render_lit(const float* verts, const float* normals, const float* uvs, const int* faces, const int* mesh_table,
                          int n_classes, int vmax, int fmax, const unsigned char* textures, const int* tex_table, const int* class_index,
                          const float* poses, const float* K9, int B, int H, int W, float znear, float zfar, int tex_bilinear,
                          const float* light_pos, const float* light_int, float brightness_ratio, const float* plane_means3,
                          float mask_thr, void* workspace, float* image, float* depth, float* mask, float* bgr, int* bbox, int* status,
                          void* stream);
/* The same render -- unlit when normals is NULL -- for a caller that re-renders into planes it knows: clean_bbox (B,4) {min x, max x,
 * min y, max y} (the bbox array a previous render into the SAME image / depth / mask / bgr planes returned; a different array than
 * `bbox`) promises that those planes hold background (image = -plane_means, depth = mask = bgr = 0) outside the box; pixels outside it
 * that this render does not cover are then not written again (the refinement loop's 2nd and 3rd render: tester.py:563-590 re-renders
 * the same object a few pixels away).  NULL = dim_raster_render / dim_raster_render_lit. */
int dim_raster_render_dirty(const float* verts, const float* normals, const float* uvs, const int* faces, const int* mesh_table,
                            int n_classes, int vmax, int fmax, const unsigned char* textures, const int* tex_table, const int* class_index,
                            const float* poses, const float* K9, int B, int H, int W, float znear, float zfar, int tex_bilinear,
                            const float* light_pos, const float* light_int, float brightness_ratio, const float* plane_means3,
                            float mask_thr, void* workspace, float* image, float* depth, float* mask, float* bgr, int* bbox, int* status,
                            const int* clean_bbox, void* stream);
/* dim_raster_render_dirty with one camera per sample.  The reference's test loop starts from K = config.dataset.INTRINSIC_MATRIX
 * (deepim/core/tester.py:165) and, before every re-render, replaces it with np.loadtxt(image_observed[:-10] + "-K.txt") when that
 * file exists (:560-562), passing it to render(..., K=K).  K_per_sample: device (B,9) f32, row-major 3x3 per sample; sample b projects
 * with its fx = K[0], fy = K[4], cx = K[2], cy = K[5].  NULL = K9 for every sample (then this is dim_raster_render_dirty, same kernels,
 * same arguments); K9 is required either way.  A sample rendered in a batch is bit-identical to the same sample rendered alone with
 * K9 = its row.  A row with fx <= 0, fy <= 0 or a non-finite entry renders that sample as background and ORs DIM_STATUS_BAD_K into
 * status[b]; the other samples are unaffected. */
int dim_raster_render_k(const float* verts, const float* normals, const float* uvs, const int* faces, const int* mesh_table, int n_classes,
                        int vmax, int fmax, const unsigned char* textures, const int* tex_table, const int* class_index, const float* poses,
                        const float* K9, int B, int H, int W, float znear, float zfar, int tex_bilinear, const float* light_pos,
                        const float* light_int, float brightness_ratio, const float* plane_means3, float mask_thr, void* workspace,
                        float* image, float* depth, float* mask, float* bgr, int* bbox, int* status, const int* clean_bbox,
                        const float* K_per_sample, void* stream);

/* dim_raster_render_k under the LINEMOD light rule: Render_Py_Light.render / Render_Py_Light_MultiProgram.render
 * (lib/render_glumpy/render_py_light.py:74, render_py_light_multi_program.py:76).  The light colour scales the diffuse term only:
 *   colour = texel/255 * ((1-ratio) + ratio*clamp(cos(normal, light-position),0,1)*light_int)
 * where dim_raster_render_lit (ModelNet) computes texel/255 * ((1-ratio) + ratio*cos) * light_int.  Normal, light vector, clamp and
 * 8-bit quantisation are the same; with light_int = (1,1,1) or ratio = 1 the two rules give the same bytes.  Always lit: normals,
 * light_pos and light_int are required.  Every other argument as in dim_raster_render_k. */
int dim_raster_render_lit_lm(const float* verts, const float* normals, const float* uvs, const int* faces, const int* mesh_table,
                             int n_classes, int vmax, int fmax, const unsigned char* textures, const int* tex_table, const int* class_index,
                             const float* poses, const float* K9, int B, int H, int W, float znear, float zfar, int tex_bilinear,
                             const float* light_pos, const float* light_int, float brightness_ratio, const float* plane_means3,
                             float mask_thr, void* workspace, float* image, float* depth, float* mask, float* bgr, int* bbox, int* status,
                             const int* clean_bbox, const float* K_per_sample, void* stream);

/* deepim/core/tester.py:204-225 (and batch_updater_py_multi.py:233-255): light_pos[b] = 0.5*(dx,dy,dz) + (tx,-ty,-tz) of poses[b]. */
int dim_modelnet_light_position(const float* poses, float dx, float dy, float dz, float* light_pos, int B, void* stream);
/* mask[b] = rectangle [y0:y1, x0:x1] (end-exclusive) of bbox[b]  (data_pair.py:103-114, UPDATE_MASK box_rendered) */
/* bbox_of_mask (optional, (B,4)): bbox {min_x,max_x,min_y,max_y} of the rectangle just written, in dim_mask_bbox's convention --
 * the next iteration's ZoomMask then needs no scan of mask_observed. */
int dim_box_mask(const int* bbox, float* mask, int B, int H, int W, int* bbox_of_mask, void* stream);

/* ---------------------------------------------------------------- scene composition (csrc/scene.hip)
 * N scenes of S layers (1 <= S <= 16); one layer = one single-object render as dim_raster_render* returns it:
 *   layer_bgr (N*S,H,W,3), layer_depth (N*S,1,H,W) metres, layer_label (N*S) int32 (device); a label <= 0 marks an unused slot, which
 *   is ignored (its planes are not read).
 * Per pixel the winner is the used layer with the smallest depth that is finite and > 0; equal depths go to the lower slot; no
 * candidate = background.  Outputs (each may be NULL): scene_bgr (N,H,W,3) background 0, scene_depth (N,1,H,W), scene_label
 * (N,1,H,W) = the winner's label as a float, background 0; vis_mask (N*S,1,H,W) = 1 where that layer wins; counts (N*S,2) int32 =
 * {full, visible} pixel counts, full = the layer's own depth > 0; vis_bbox (N*S,4) int32 = box of vis_mask in dim_mask_bbox's
 * convention (empty = {W,-1,H,-1}); status (N*S int32): DIM_STATUS_LAYER_HIDDEN is OR-ed in for a used layer that wins no pixel.
 * workspace: dim_scene_compose_workspace_bytes(), 4-byte aligned, needed for counts / vis_bbox / status; its contents before the
 * call do not matter, and neither do the outputs'.  16-byte accesses when W % 4 == 0 and every plane is 16-byte aligned.
 * Deviation: toolkit/LM6d_occ_dsm_1_gen_observed_light.py:219-236 paints whole objects in order of their mean depth (an order it
 * also scrambles by indexing a reversed array); the per-pixel depth test here is what that approximates -- the same result whenever
 * objects do not interpenetrate and the order is the intended one. */
long dim_scene_compose_workspace_bytes(int N, int S, int H, int W);
int dim_scene_compose(const float* layer_bgr, const float* layer_depth, const int* layer_label, int N, int S, int H, int W,
                      void* workspace, float* scene_bgr, float* scene_depth, float* scene_label, float* vis_mask, int* counts,
                      int* vis_bbox, int* status, void* stream);

/* ---------------------------------------------------------------- convolution stack (NHWC, f32 MFMA)
 * weights: pack once from the reference layout (Cout,Cin,KH,KW).  Cin must be 8 or a multiple of 32,
 * Cout a multiple of 64.  y = LeakyReLU_slope(conv(x) + bias); slope 1.0 = linear.
 * splits > 1 = split-K through `workspace` (dim_conv2d_workspace_floats), deterministic reduce.
 * tile: 0 auto | 1 128x128 (4 waves) | 2 128x64 | 3 64x64 | 4 128x128 (8 waves) (GEMM rows x output channels per workgroup of the
 *       gathered-tap kernel) | 6 the LDS-halo first-layer kernel (Cin 8, 7x7 / stride 2, Cout 64, dense f32 output).
 * Outputs are stored through a buffer descriptor with 32-bit byte offsets: N*OH*OW*out_cstride*4 must stay below 2^31.
 *
 * Caller-owned buffers of the convolution stack (every entry point from here to the optimizer steps; pinned on guarded buffers by
 * tests/test_gpu_conv_workspace_contract.py):
 *   workspace   Its size is what the entry's dim_*_workspace_floats function returns for the same arguments, in floats; a call
 *               neither reads nor writes a byte beyond that.  The tests place it 256-byte aligned; dim_conv2d_dgrad_bf16_splitk
 *               requires 16 bytes, no entry requires more.  Its contents before the call do not matter: zero words, NaN words, +inf
 *               words and what a call of the same entry on another shape left behind give the same output bit for bit, so one buffer
 *               of the largest size may serve every layer in turn without being cleared (deepim/core/module.py does that).
 *                 dim_conv2d_fwd / _partial + dim_splitk_reduce   dim_conv2d_workspace_floats(..., splits); 0 floats for splits == 1;
 *                                                                 splits == 0 ("auto"): the bound of the split tail
 *                 dim_conv2d_fwd_winograd (forward, and the 3x3 input gradient run through it)   dim_winograd_workspace_floats
 *                 dim_conv2d_fwd_winograd3x3s2                    dim_winograd3x3s2_workspace_floats
 *                 dim_conv2d_fwd_winograd5x5s2[_map], dim_conv2d_dgrad_winograd5x5s2   dim_winograd5x5s2_workspace_floats
 *                   (the four above: V and M of one slice of the batch; a later slice overwrites the earlier one's, and the M tiles
 *                   two stream-K workgroups share are zeroed inside the call)
 *                 dim_conv2d_wgrad_winograd                       dim_conv2d_wgrad_winograd_workspace_floats
 *                 dim_conv2d_wgrad[_bf16]                         dim_conv2d_wgrad_workspace_floats(..., splits); 0 for splits == 1
 *                 dim_conv2d_wgrad_oihw                           dim_conv2d_wgrad_workspace_floats(..., splits + 1), also for splits == 1
 *                   (a split count larger than the pixel steps / 8 x 8 blocks can fill is clamped: fewer slabs are used, never more)
 *                 dim_conv2d_dgrad_bf16_splitk                    dim_conv2d_dgrad_splitk_workspace_floats
 *                 dim_conv2d_dgrad_bf16_lrelu                     dim_conv2d_dgrad_lrelu_workspace_floats
 *                 dim_bias_grad, dim_lrelu_bwd_bias_grad          dim_bias_grad_workspace_floats, dim_lrelu_bwd_bias_grad_workspace_floats
 *                 dim_fc_fwd                                      dim_fc_fwd_workspace_floats
 *                 dim_conv_small_cout_bwd                         dim_conv_small_cout_bwd_workspace_floats
 *   outputs     An entry with out_cstride / out_coff (dx_cstride, dy_coff, dz_coff: the same for a gradient) writes channels
 *               [coff, coff + C) of every row and no other byte of the buffer; a dense output is written in full, whatever it held
 *               (accumulate / accumulate_dx: added to).  The refusals the tests provoke -- a 128-wide tile on 64 filters, dim_fc_fwd
 *               with Out % 256 != 0, dim_conv2d_wgrad[_bf16] with accumulate and more than one split -- return DIM_ERR_ARG before
 *               anything is enqueued and leave workspace and outputs untouched.
 *   packers     Each writes all N elements of its output, N = the packer's dim_*_packed_weight_floats (dim_fc_pack_weight,
 *               dim_fc_dgrad_pack_weight[_bf16]: Out*C*H*W; dim_conv_small_cout_pack_weight: Cout*KH*KW*CinPad; the _padded packer:
 *               KH*KW*Cin*CoutPad), pad rows, pad columns and the three-term image behind the f32 weights (first layer, Winograd
 *               layers) included, whatever the buffer held: no kernel reads a word of a packed buffer that its packer did not write.
 *               One exception: dim_conv2d_pack_weight_bf16 for the 8-channel 7x7 first layer writes the ceil(KH*KW/4)*32*CoutPad
 *               weights and leaves the rest of a buffer of dim_conv2d_packed_weight_floats elements alone -- the f32 buffer's
 *               three-term image has no bf16 counterpart, and the bf16 kernels read the weights only. */
long dim_conv2d_packed_weight_floats(int Cout, int Cin, int KH, int KW);
int dim_conv2d_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, void* stream);
long dim_conv2d_workspace_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int splits);
int dim_conv2d_fwd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                   int Cin, int Cout, int KH, int KW, int stride, int pad, float slope, int splits, int tile, void* stream);
/* the two phases of a split-K dim_conv2d_fwd as separate calls (same kernels; lets a caller time / overlap them):
 * partial: raw K-slice sums -> workspace[splits][M][Cout];  reduce: y = LeakyReLU(sum_k slabs + bias). */
int dim_conv2d_fwd_partial(const float* x, const float* w_packed, float* workspace, int N, int H, int W, int Cin, int Cout, int KH,
                           int KW, int stride, int pad, int splits, int tile, void* stream);
int dim_splitk_reduce(const float* slabs, const float* bias, float* y, long M, int Cout, int splits, float slope, void* stream);
/* generalised dim_conv2d_fwd (no split-K): input pixel stride `in_cstride` (>= Cin), output written at channel offset
 * `out_coff` of rows `out_cstride` wide (concat buffers), and -- when osy > 0 -- scattered to
 * (oy,ox) = (ho*osy + ooy, wo*osx + oox) inside an OH x OW map (used for the phases of a deconvolution + Crop). */
/* Ho/Wo > 0: explicit output grid (asymmetric padding); pad_w >= 0: horizontal padding differs from pad; accumulate: y += result */
/* splits == 0 in dim_conv2d_fwd = "auto": all workgroups of a launch are equal, so a launch takes ceil(tiles / CUs) tile-times
 * on the busiest CU (1200 tiles on 256 CUs = 4.69 -> 5: 6 % of the chip idles).  Auto runs k*CUs tiles as one launch and the rest
 * as a split-K launch of proportionally shorter workgroups + reduce.  Needs workspace = dim_conv2d_workspace_floats(..., splits=0).
 * dim_conv2d_tail_plan reports the plan for a shape: first tile of the tail and its split count (1 = single launch). */
int dim_conv2d_tail_plan(int M, int Cout, int Cin, int KH, int KW, int tile, int* tail_begin_tile, int* tail_splits);
/* The default launch plans of the f32 forward path, in ONE place for every host (FlowNetHip in Python, dim_refiner_create in C):
 * (tile, splits) of a direct layer with M GEMM rows and `nchunks` K chunks of 32 (splits 0 = the "auto" tail plan above), and the
 * workgroup tile of a Winograd layer's plane GEMMs (3 / 4 / 5 = 64 x 64 / 128 x 128 / 128 x 256) for `tiles` transform tiles. */
int dim_conv_auto_plan(long M, int Cout, int nchunks, int cin, int* tile, int* splits);
int dim_winograd_gemm_tile(int Cout, long tiles);                          /* = ..._planes(Cout, tiles, 36) */
int dim_winograd_gemm_tile_planes(int Cout, long tiles, int planes);      /* planes: 36 (F(4x4,3x3), 5x5 / s2) or 81 (3x3 / s2) */
/* Arithmetic of the Winograd layers' plane GEMMs.  1 (default): every f32 operand enters the matrix pipe as the exact sum of three
 * bf16 terms and a product keeps the six largest term products, accumulated in f32 (error <= 3 * 2^-27 per product, below f32's own
 * rounding of the sums); 0: v_mfma_f32_32x32x2_f32 on the f32 operands.  Every packed Winograd weight buffer carries both images
 * (dim_winograd*_packed_weight_floats counts them).  Takes effect when a layer is next planned (launch or graph capture). */
int dim_set_winograd_split(int on);
int dim_get_winograd_split(void);
/* The plane GEMM of the Winograd layers on its own, planned and run exactly as the layers do (stream-K ranges, shared-tile atomics,
 * the arithmetic dim_set_winograd_split selects): M[t][p][:] = V[t][p][:] . U_p for P planes.  V [T][P][K], M [T][P][Cout], U_packed =
 * U in the chunk layout [P][K/32][Cout][32] (element (p, k, co) at ((p * K/32 + k/32) * Cout + co) * 32 + k % 32) with room for its
 * three-term image behind it: dim_winograd_plane_gemm_weight_floats floats = P*K*Cout + 6 bytes per weight;
 * dim_winograd_plane_gemm_split_weights writes that image from the first P*K*Cout floats (once per change of U).  tile: 3 .. 7 as
 * dim_winograd_gemm_tile_planes returns them; *used_split (host) = 1 if the three-term kernel ran (tiles 4, 5, 7 with the switch on).
 * The tests' entry to the arithmetic of one K chunk.  K % 32 != 0, Cout % 64 != 0, a size < 1, a NULL or a host pointer return
 * DIM_ERR_ARG before anything is enqueued. */
long dim_winograd_plane_gemm_weight_floats(int K, int Cout, int P);
int dim_winograd_plane_gemm_split_weights(float* U_packed, int K, int Cout, int P, void* stream);
int dim_winograd_plane_gemm(const float* V, const float* U_packed, float* M, int T, int K, int Cout, int P, int tile, int* used_split,
                            void* stream);
int dim_conv2d_fwd_ex(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int in_cstride,
                      int Cout, int KH, int KW, int stride, int pad, float slope, int tile, int out_cstride, int out_coff, int OH,
                      int OW, int osy, int osx, int ooy, int oox, int Ho, int Wo, int pad_w, int accumulate, void* stream);

/* Winograd form of the 3x3 / stride 1 / pad 1 layers (conv3_1, conv4_1, conv5_1, conv6_1 of
 * deepim/symbols/deepIM_flownet.py:103-191): same result as dim_conv2d_fwd up to f32 rounding (tests: 1e-4 relative).
 * m = output tile edge: 2 = F(2x2,3x3), 16 GEMMs, 2.25x fewer multiply-adds; 4 = F(4x4,3x3), 36 GEMMs, 4x fewer (Cook-Toom points
 * {0, 1, -1, 2, -1/2, inf}).  Weights are transformed once (dim_winograd_pack_weight from the (Cout,Cin,3,3) array, same m);
 * workspace = dim_winograd_workspace_floats floats.  in_cstride / out_cstride 0 = dense; y = LeakyReLU_slope(conv + bias). */
long dim_winograd_packed_weight_floats(int Cout, int Cin, int m);
long dim_winograd_workspace_floats(int N, int H, int W, int Cin, int Cout, int m);
int dim_winograd_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int m, void* stream);
/* transformed weights of the INPUT gradient of the same layer (a Winograd convolution of dY with the flipped, transposed kernel: Cin
 * output and Cout input channels), read straight from the forward (Cout, Cin, 3, 3) array; same size as dim_winograd_pack_weight's */
int dim_winograd_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int m, void* stream);
/* events4: NULL, or four hipEvent_t recorded on the stream before the input transform, before / after the batched GEMM and after
 * the output transform (how bench.py times the GEMM launch separately from the transforms). */
int dim_conv2d_fwd_winograd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                            int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, int m,
                            void** events4, void* stream);
/* 5x5 / stride 2 / pad 2 layers (conv2, conv3 of deepim/symbols/deepIM_flownet.py:95-101) through Winograd as well: the layer is
 * the sum of four 3x3 / stride-1 / pad-1 convolutions of the phase images x[2r + py][2q + px] with the sub-kernels
 * w[2u + py][2v + px]; the four F(4x4,3x3)-transformed phase tiles are concatenated along the channels, so 36 GEMMs with K = 4 Cin
 * replace the 25-tap direct form (2.78x fewer multiply-adds) and the output transform is the one of the stride-1 layers.
 * 23 of the 144 (phase, plane) weight blocks are zero by construction: the forward neither stores their V blocks nor multiplies them
 * (top of the 5x5 / stride-2 code in csrc/winograd.hip); layouts, sizes and results are unchanged.
 * Weights: MXNet layout (Cout,Cin,5,5).  Output (N, ceil(H/2), ceil(W/2), Cout).  Same f32 accuracy class as F(4x4,3x3). */
long dim_winograd5x5s2_packed_weight_floats(int Cout, int Cin);
long dim_winograd5x5s2_workspace_floats(int N, int H, int W, int Cin, int Cout);
int dim_winograd5x5s2_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream);
int dim_conv2d_fwd_winograd5x5s2(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                                 int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, void** events4,
                                 void* stream);
/* Equal live work per workgroup for the plane GEMMs of these layers (csrc/wino_balance.hip).  With the zero blocks skipped, a
 * workgroup's range of the flat chunk list holds a full, a half or a quarter of its length in live chunks, by the planes it lies in.
 * An item map is a permutation of the list's item slots that evens the live work out: ranges and cuts stay where they are, every slot
 * with a cut inside stays in place, whole items change workgroups.  The output keeps its bits.
 *   dim_wino_item_map_create   plans the layer (N, H, W, Cin, Cout, tile as dim_conv2d_fwd_winograd5x5s2 takes them), builds the table on
 *                              the host and uploads it (hipMalloc + a blocking copy: call it where layers are planned, never while a
 *                              stream is being captured).  *map is never NULL on DIM_OK; a map that gains nothing holds the identity.
 *   dim_wino_item_map_query    header (12 ints: T, K, Cout, tile, G, per, rem, largest live work of a range before / after, slots that
 *                              hold another item, items, chunks per item) and, when table != NULL, the items of all slots
 *                              (capacity >= items ints) into host memory.
 *   dim_wino_item_map_plan     the same answer for a GEMM shape without a map object: T rows, K = 4 Cin, tile, G workgroups (host
 *                              arithmetic only, no device needed; G <= 0: the G a launch on the current device would take),
 *                              skip5 = 0: the plan of a layer that multiplies every block (identity).
 *   dim_conv2d_fwd_winograd5x5s2_map   the forward with a map (NULL: identity).  The map is used when the plan of the run is the one it
 *                              was built for; any other run (another batch, a sliced run, the f32 matrix pipe) is the plain forward. */
int dim_wino_item_map_create(void** map, int N, int H, int W, int Cin, int Cout, int tile);
void dim_wino_item_map_destroy(void* map);
int dim_wino_item_map_query(const void* map, int* header12, int* table, long capacity);
int dim_wino_item_map_plan(int T, int K, int Cout, int tile, int G, int skip5, int* header12, int* table, long capacity);
int dim_conv2d_fwd_winograd5x5s2_map(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H,
                                     int W, int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile,
                                     const void* item_map, void** events4, void* stream);
/* Input gradient of the same 5x5 / stride-2 layers (training): dx (N,H,W,dx_cstride) = conv_transpose(dy (N,ceil(H/2),ceil(W/2),
 * dy_cstride), w) as ONE F(4x4,3x3) transform of dy, 36 GEMMs with K = Cout and N = 4 Cin (the four phase images of dx), and a
 * phase-scattering output transform; dx is overwritten.  Weights: dim_winograd5x5s2_dgrad_pack_weight from the same (Cout,Cin,5,5)
 * array (dim_winograd5x5s2_packed_weight_floats floats); workspace: dim_winograd5x5s2_workspace_floats floats. */
int dim_winograd5x5s2_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream);
int dim_conv2d_dgrad_winograd5x5s2(const float* dy, const float* w_packed, float* dx, float* workspace, int N, int H, int W, int Cin,
                                   int dx_cstride, int Cout, int dy_cstride, int tile, void* stream);
/* Weight gradient of the same layers through Winograd (training): dw (Cout,Cin,k,k) MXNet layout (=, or += when accumulate) =
 * scale * sum over pixels of x (*) dy.  S = 1: 3x3 / stride 1 / pad 1 (k = 3); S = 2: 5x5 / stride 2 / pad 2 (k = 5, four phase
 * images of x).  Per 4x4 tile of dy this is the correlation F(3x3,4x4): V = B^T x B (the forward's input transform), D = G4 dy G4^T,
 * 36 plane products contracted over tiles and batch on the wgrad MFMA kernel (`splits` pixel ranges, deterministic slab reduce),
 * dW = A3^T dM A3: 4x (S = 1) / 2.78x (S = 2) fewer multiply-adds than dim_conv2d_wgrad.  x (N,H,W,in_cstride), dy (N,Ho,Wo,dy_cstride). */
long dim_conv2d_wgrad_winograd_workspace_floats(int N, int H, int W, int Cin, int Cout, int S, int splits);
int dim_conv2d_wgrad_winograd(const float* x, const float* dy, float* dw_oihw, float* workspace, int N, int H, int W, int Cin, int in_cstride,
                              int Cout, int dy_cstride, int S, int splits, float scale, int accumulate, void* stream);
/* 3x3 / stride-2 / pad-1 layers (conv4, conv5: deepim/symbols/deepIM_flownet.py:118-126, 143-151) in the Winograd domain through their
 * phase images: per axis the even phase meets one tap (F(4,1) = identity), the odd phase two (F(4,2), points {0, 1, -1, 2, inf}): 81
 * multiplies per 4 x 4 output tile and channel pair against 144, 81 plane GEMMs on the stream-K kernel of the other Winograd layers.
 * x (N,H,W,in_cstride)[:Cin] -> y (N,Ho,Wo,out_cstride)[out_coff:+Cout], Ho = floor((H - 1) / 2) + 1; Cin % 32 == 0, Cout % 64 == 0.
 * Same result as dim_conv2d_fwd(3, 3, stride 2, pad 1) up to f32 rounding (1.4e-6 of max |y| at Cin = 256; direct: 3e-7). */
long dim_winograd3x3s2_packed_weight_floats(int Cout, int Cin);
int dim_winograd3x3s2_use(int H, int W, int Cin, int Cout);   /* 1: the launch plan sends this layer (input map H x W) through this path */
long dim_winograd3x3s2_workspace_floats(int N, int H, int W, int Cin, int Cout);
int dim_winograd3x3s2_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream);
int dim_conv2d_fwd_winograd3x3s2(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                                 int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, void** events4,
                                 void* stream);
/* fc6 (deepim/symbols/deepIM_flownet.py:196-198) for the small batches of the refinement loop as a weight stream: y (B,Out) =
 * LeakyReLU_slope(x (B,H,W,C NHWC) . W^T + bias) with W packed by dim_fc_pack_weight.  Every workgroup owns a contiguous range of K
 * chunks and all outputs and writes one partial tile into `workspace` (dim_fc_fwd_workspace_floats floats); a second kernel sums the
 * partials in a fixed order.  32 batch rows per pass.  Same result as dim_conv2d_fwd(KH=H, KW=W) up to the summation order. */
long dim_fc_fwd_workspace_floats(int C, int H, int W, int Out);
int dim_fc_fwd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int B, int C, int H, int W, int Out,
               float slope, void* stream);
/* dim_conv2d_pack_weight with the output channels zero-padded to CoutPad (multiple of 64) */
int dim_conv2d_pack_weight_padded(const float* w_oihw, float* w_packed, int Cout, int CoutPad, int Cin, int KH, int KW, void* stream);
/* Decoder (deepIM_flownet.py:213-299): y[..., out_coff:out_coff+Cout] = LeakyReLU(Crop(Deconvolution(x, k=4, s=2, p=0) + bias,
 * offset=(crop,crop))) as four 2x2 sub-pixel convolutions on the MFMA kernel.  Weight: MXNet layout (Cin, Cout, 4, 4). */
long dim_deconv4x4s2_packed_weight_floats(int Cin, int Cout);
int dim_deconv4x4s2_pack_weight(const float* w_iohw, float* w_packed, int Cin, int Cout, void* stream);
int dim_deconv4x4s2_fwd(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin,
                        int in_cstride, int Cout, int OH, int OW, int crop, float slope, int out_cstride, int out_coff, int tile,
                        void* stream);
/* same operator for a tiny channel count (upsample_flow6to5 / 5to4, 2 -> 2), direct; weight in MXNet layout, unpacked */
int dim_deconv4x4s2_tiny_fwd(const float* x, const float* w_iohw, const float* bias, float* y, int N, int H, int W, int Cin,
                             int in_cstride, int Cout, int OH, int OW, int crop, int out_cstride, int out_coff, void* stream);
/* 3x3 (any KHxKW, stride 1) convolution to 1 or 2 channels (Convolution1/2/3, mask_conv3), no activation.
 * Weight (Cout,Cin,KH,KW) packed to [Cout][KH][KW][CinPad], CinPad = Cin rounded up to 32 (floats: Cout*KH*KW*CinPad). */
int dim_conv_small_cout_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, void* stream);
int dim_conv_small_cout_fwd(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin,
                            int in_cstride, int Cout, int KH, int KW, int pad, int out_cstride, int out_coff, void* stream);
/* Deconvolution(k=32, s=16, num_group=C, no bias) + Crop(offset (crop,crop)) -> NCHW planes (N,C,OH,OW), times `scale`;
 * mode 1 applies a sigmoid (mask probability).  deepIM_flownet.py:326-340, :513-529, :845-872. */
int dim_upsample16_fwd(const float* x_nhwc, const float* w_c1_32_32, float* y_nchw, int N, int C, int h, int w, int OH, int OW,
                       int crop, float scale, int mode, void* stream);
/* ---------------------------------------------------------------- backward of the convolution stack (training)
 * dgrad: dx[..., :Cin] (+)= d/dx of y = conv(x, W (Cout,Cin,KH,KW), stride 1|2, pad); runs on the forward MFMA kernel with the
 * weights re-packed by dim_conv2d_dgrad_pack_weight (stride 2 = four input phases).  dx's channel stride must be >= Cin
 * rounded up to 64. */
long dim_conv2d_dgrad_packed_weight_floats(int Cout, int Cin, int KH, int KW, int stride, int pad);
int dim_conv2d_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, int stride, int pad,
                                 void* stream);
int dim_conv2d_dgrad(const float* dy, const float* w_dgrad_packed, float* dx, int N, int H, int W, int Cin, int dx_cstride, int Ho,
                     int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad, int accumulate, int tile, void* stream);
/* wgrad: dw_packed (same layout as dim_conv2d_pack_weight's output, so SGD updates the packed weights in place)
 * (+)= sum over pixels of dz (N,Ho,Wo,dz_cstride)[dz_coff:+Cout] x gathered x (N,H,W,in_cstride)[:Cin]. */
long dim_conv2d_wgrad_workspace_floats(int Cout, int Cin, int KH, int KW, int splits);
int dim_conv2d_wgrad(const float* x, const float* dz, float* dw_packed, float* workspace, int N, int H, int W, int Cin, int in_cstride,
                     int Ho, int Wo, int Cout, int dz_cstride, int dz_coff, int KH, int KW, int stride, int pad, int splits,
                     int accumulate, void* stream);
/* The same weight gradient delivered in the MXNet layout dw_oihw (Cout_rows, Cin, KH, KW) = (accumulate ? dw_oihw : 0) + scale * dW (rows
 * Cout_rows .. Cout - 1 of a channel-padded gradient are dropped): the pixel-split slabs stay in `workspace` --
 * dim_conv2d_wgrad_workspace_floats(Cout, Cin, KH, KW, splits + 1) floats, also for splits == 1 -- and the layout converter sums
 * them in slab order on its way out, so the packed intermediate, its round trip through HBM and the reduce launch of
 * dim_conv2d_wgrad + dim_conv2d_unpack_weight disappear; same bits as that pair whenever it sums slabs serially (fewer than 64 slabs or
 * slabs of >= 2^18 floats; otherwise the lane-parallel reduce runs first, as there).  bf16_mfma: products on the bf16 matrix pipe
 * (dim_conv2d_wgrad_bf16).  Replaces the weight-gradient half of the executor's backward (deepim/core/module.py:1205-1213). */
int dim_conv2d_wgrad_oihw(const float* x, const float* dz, float* dw_oihw, float* workspace, int N, int H, int W, int Cin, int in_cstride,
                          int Ho, int Wo, int Cout, int dz_cstride, int dz_coff, int KH, int KW, int stride, int pad, int splits,
                          int bf16_mfma, int Cout_rows, float scale, int accumulate, void* stream);
/* ---------------------------------------------------------------- bf16 matrix pipe (training mode, BASELINE configs[2])
 * The reference trains in fp32 (deepim/train.py:338-414); these twins of the convolution entry points run the same implicit GEMMs
 * on v_mfma_f32_32x32x16_bf16 (f32 accumulate, 16x the f32 matrix rate): activations and gradients stay fp32 in HBM and are rounded
 * to bf16 (nearest even) on the way into LDS; `w_packed_bf16` is the bf16 image -- dim_f32_to_bf16, element by element -- of the
 * SAME packed array the f32 entry point takes (dim_conv2d_pack_weight, dim_conv2d_dgrad_pack_weight, dim_deconv4x4s2_pack_weight,
 * dim_conv2d_pack_weight_padded), so every packer is shared.  Arguments otherwise as the f32 functions (dim_conv2d_fwd_bf16:
 * splits >= 1, no "auto" mode).  dim_conv2d_wgrad_bf16 returns an fp32 gradient in the packed layout, like dim_conv2d_wgrad.
 * Declared tolerance vs the fp32 path: 2^-8 relative per product, i.e. ~4e-3 L2-relative on a layer output / gradient tensor.
 * Tile 6 (the 8-channel 7x7 / stride-2 / 64-filter first layer from an LDS-resident patch) exists on both pipes.
 * bf16-only tiles: 7 = LDS-halo kernel (8 x 16 pixels x 128 channels; 3x3 / 5x5, stride 1 / 2, dense output); 8 = 128 x 256 gathered taps;
 * 9 = stride-1 patch kernel (16 x 16 pixels x 128 or 64 channels, KH, KW <= 3 with 2 .. 9 taps, Cin % 32 == 0, Cout % 64 == 0, dense or
 * scattered output, batched phases); dim_conv2d_dgrad_bf16 with tile 9 applies it to every phase of a strided gradient that has >= 2
 * taps and runs the single-tap phase on the gathered-tap kernel.  Tile 9 also has a stride-2 form (8 x 16 pixels x 128 channels, 3x3 or
 * 5x5, dense output): Cout % 128 == 0 there, so a 64-filter stride-2 request is refused.
 * What the direct entries refuse (DIM_ERR_ARG before anything is enqueued; outputs and workspace untouched; pinned by
 * tests/test_gpu_direct_conv_exact.py):
 *   forward    tiles 1 / 4 with Cout % 128 != 0; tile 4 on the 8-channel layer; tile 6 on anything but the 8-channel 7x7 / stride-2 /
 *              64-filter layer; tiles 7, 8, 9 on f32 weights; tile 7 with Cout % 128 != 0 or on a 5x5 / stride-1 layer; tile 8 with
 *              Cout % 256 != 0; tile 9 at stride 1 with KH or KW > 3; a map smaller than the kernel (H + 2 pad < KH or W + 2 pad < KW:
 *              an empty output)
 *   dgrad      tile 7 on f32 weights (tile 9 there runs every phase on the gathered-tap kernel); tiles 4 / 7 unless Cin rounded up to 64
 *              is a multiple of 128; tile 7 at stride 2 (its output is dense); the folded form (dim_conv2d_dgrad_bf16_lrelu) on a layer
 *              with a single-tap phase (3x3 / stride 2)
 *   wgrad      accumulate with more than one split (after clamping); accumulate in the bf16 patch form (3x3 / stride 1 / pad 1,
 *              Cout % 128 == 0, Ho Wo >= 1200)
 *   deconv     tile 9 on f32 weights */
/* The input gradient of a layer whose INPUT is another layer's LeakyReLU output, with that LeakyReLU' and the lower layer's bias
 * gradient folded into the epilogue (tile 9, the bf16 patch kernel: 3x3 / stride 1 and 5x5 / stride 2 layers on maps of >= 1200 pixels):
 * dz (N,H,W,Cin) = dX * (y_act > 0 ? 1 : slope), db[Cin] (+)= column sums of dz.  y_act (N,H,W,Cin) is the stored activation; Cin % 64 == 0.
 * Same dz bits as dim_conv2d_dgrad_bf16(tile 9) followed by dim_lrelu_bwd_bias_grad; db differs in summation order only.  Replaces one
 * 12-bytes-per-element pass over the gradient per layer (deepim/core/module.py:1205-1213 runs it inside MXNet's backward). */
long dim_conv2d_dgrad_lrelu_workspace_floats(int N, int H, int W, int Cin, int stride);
int dim_conv2d_dgrad_bf16_lrelu(const float* dy, const void* w_dgrad_packed_bf16, float* dz, const float* y_act, float slope, float* db,
                                float* workspace, int N, int H, int W, int Cin, int dx_cstride, int Ho, int Wo, int Cout, int dy_cstride,
                                int KH, int KW, int stride, int pad, int accumulate_db, void* stream);
int dim_f32_to_bf16(const float* src, void* dst_bf16, long n, void* stream);
int dim_bf16_to_f32(const void* src_bf16, float* dst, long n, void* stream);
/* The packers with the rounding folded in: each writes exactly dim_f32_to_bf16 of the weights its f32 twin writes (same element
 * count, same order; for the 8-channel first layer that is the 13 x 32 x CoutPad weights, not the three-term image the f32 buffer
 * carries behind them) in one pass over the MXNet-layout weights -- the training executor re-packs every layer after every update.
 * dim_conv2d_pack_weight_bf16 covers both dim_conv2d_pack_weight (CoutPad == Cout) and dim_conv2d_pack_weight_padded. */
int dim_conv2d_pack_weight_bf16(const float* w_oihw, void* w_packed_bf16, int Cout, int CoutPad, int Cin, int KH, int KW, void* stream);
int dim_conv2d_dgrad_pack_weight_bf16(const float* w_oihw, void* w_packed_bf16, int Cout, int Cin, int KH, int KW, int stride, int pad,
                                      void* stream);
int dim_deconv4x4s2_pack_weight_bf16(const float* w_iohw, void* w_packed_bf16, int Cin, int Cout, void* stream);
int dim_fc_dgrad_pack_weight_bf16(const float* w_out_in, void* w_packed_bf16, int Out, int C, int H, int W, void* stream);
int dim_conv2d_fwd_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, float* workspace, int N, int H, int W,
                        int Cin, int Cout, int KH, int KW, int stride, int pad, float slope, int splits, int tile, void* stream);
int dim_conv2d_fwd_ex_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, int N, int H, int W, int Cin,
                           int in_cstride, int Cout, int KH, int KW, int stride, int pad, float slope, int tile, int out_cstride,
                           int out_coff, int OH, int OW, int osy, int osx, int ooy, int oox, int Ho, int Wo, int pad_w, int accumulate,
                           void* stream);
int dim_conv2d_dgrad_bf16(const float* dy, const void* w_dgrad_packed_bf16, float* dx, int N, int H, int W, int Cin, int dx_cstride,
                          int Ho, int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad, int accumulate, int tile,
                          void* stream);
/* The same with the contraction (taps x output channels of dy) cut into `splits` ranges (tile 3 / 4 only): the small maps give too
 * few tiles to fill the chip.  Partial sums go to `workspace` (dim_conv2d_dgrad_splitk_workspace_floats: `splits` copies of dx) and
 * one pass adds them up in a fixed order (deterministic); every phase of a strided gradient needs >= splits K chunks. */
long dim_conv2d_dgrad_splitk_workspace_floats(int N, int H, int W, int dx_cstride, int splits);
int dim_conv2d_dgrad_bf16_splitk(const float* dy, const void* w_dgrad_packed_bf16, float* dx, float* workspace, int N, int H, int W, int Cin,
                                 int dx_cstride, int Ho, int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad,
                                 int accumulate, int tile, int splits, void* stream);
int dim_deconv4x4s2_fwd_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, int N, int H, int W, int Cin,
                             int in_cstride, int Cout, int OH, int OW, int crop, float slope, int out_cstride, int out_coff, int tile,
                             void* stream);
/* pixel-split count that makes dim_conv2d_wgrad_bf16's whole grid resident at once on n_cu compute units (size the slab workspace
 * with it: dim_conv2d_wgrad_workspace_floats) */
int dim_conv2d_wgrad_bf16_splits(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int n_cu);
int dim_conv2d_wgrad_bf16(const float* x, const float* dz, float* dw_packed, float* workspace, int N, int H, int W, int Cin, int in_cstride,
                          int Ho, int Wo, int Cout, int dz_cstride, int dz_coff, int KH, int KW, int stride, int pad, int splits,
                          int accumulate, void* stream);
/* db[c] (+)= sum_m dz[m][dz_coff + c]   (workspace: dim_bias_grad_workspace_floats) */
long dim_bias_grad_workspace_floats(int M, int C);
int dim_bias_grad(const float* dz, float* db, float* workspace, int M, int C, int dz_cstride, int dz_coff, int accumulate, void* stream);
/* LeakyReLU backward in place on a channel range: dy *= (y > 0 ? 1 : slope) */
int dim_lrelu_bwd(const float* y, int y_cstride, int y_coff, float* dy, int dy_cstride, int dy_coff, long M, int C, float slope,
                  void* stream);
/* both of the above in one pass over the gradient map: dy *= (y > 0 ? 1 : slope) in place, db[c] (+)= sum_m dy[m][dy_coff + c]
 * (the pair MXNet's LeakyReLU backward + Convolution backward-bias make; deepIM_flownet.py:67-208) */
long dim_lrelu_bwd_bias_grad_workspace_floats(int M, int C);
int dim_lrelu_bwd_bias_grad(const float* y, int y_cstride, int y_coff, float* dy, int dy_cstride, int dy_coff, float* db, float* workspace,
                            int M, int C, float slope, int accumulate, void* stream);
/* ---------------------------------------------------------------- training-only pieces (csrc/train.hip)
 * layout converters: packed conv / fc weights (or gradients) back to the MXNet layouts; fc6 dgrad weights */
int dim_conv2d_unpack_weight(const float* w_packed, float* w_oihw, int Cout, int CoutPad, int Cin, int KH, int KW, float scale,
                             int accumulate, void* stream);
int dim_fc_unpack_weight(const float* w_packed, float* w_out_in, int Out, int C, int H, int W, void* stream);
int dim_fc_dgrad_pack_weight(const float* w_out_in, float* w_packed, int Out, int C, int H, int W, void* stream);
/* loss gradients (get_loss, deepIM_flownet.py:303-560); loss_sum (1 float, may be NULL) accumulates the un-scaled loss for metrics */
int dim_flow_loss_grad(const float* flow_est, const float* flow_label, const float* flow_weights, float* grad, long n, float normalize_flow,
                       float grad_scale, float* loss_sum, void* stream);
int dim_logistic_grad(const float* logits, const float* label, float* grad, float* prob, long n, float grad_scale_over_num_output,
                      void* stream);
int dim_pm_l1_grad(const float* p_est, const float* p_obs, const float* weights, float* grad, long n, float norm_term, float grad_scale,
                   float* loss_sum, void* stream);
/* the point-matching loss with SE3_PM_LOSS_TYPE 'L1' (0, = dim_pm_l1_grad) | 'L2' (1) | 'smooth_L1' (2, mx.sym.smooth_l1 with
 * scalar = SE3_PM_SL1_SCALAR)   (deepIM_flownet.py:458-499) */
int dim_pm_loss_grad(const float* p_est, const float* p_obs, const float* weights, float* grad, long n, float norm_term, float grad_scale,
                     int loss_type, float smooth_l1_scalar, float* loss_sum, void* stream);
/* The point-matching loss against the closest of the symmetric ground truths (train_iter.SE3_PM_SYM).  p_est, points_model, weights:
 * (B,3,N) float32; tgt_pose (B,3,4) float32; sym (Stot,3,4) float32 and sym_off (n_classes+1) int32: the classes' symmetry sets [Rs | ts],
 * identity first (lib/utils/symmetry.py symmetry_tables), class c owning entries sym_off[c] .. sym_off[c+1]-1 (an empty range = the
 * identity alone); class_index (B) int32.  Per pair, with f the element loss of loss_type:
 *   G_s = [R_g Rs | R_g ts + t_g] (float64), target_s = float32(G_s x), L_s = sum over points and coordinates of w f((p_est - target_s) / norm_term)
 *   s* = the first s with the least L_s (a later s replaces only with a strictly smaller, finite sum; a NaN L_0 stays)
 *   grad = grad_scale w f'((p_est - target_s*) / norm_term) / norm_term, bit for bit dim_pm_loss_grad's for (p_est, target_out, weights);
 *   target_out (B,3,N, may be NULL) = target_s*; best_sym[b] (may be NULL) = s*; *loss_sum (may be NULL) += L_s*, one add per pair.
 * With the identity alone target_out is bit for bit dim_point_clouds' point_cloud_observed for the same pose and points.
 * A class index outside [0, n_classes), or a class with more than max_sym entries, gives the pair a zero gradient (and target_out),
 * best_sym -1, no loss contribution, and ORs DIM_STATUS_BAD_CLASS into status[b] (B int32, may be NULL).
 * workspace: dim_pm_sym_workspace_bytes(B, n_points, max_sym) bytes, 4-byte aligned, no initialisation needed.  max_sym <= 4096.
 * Two launches, no allocation or synchronisation (graph-capturable); no atomics in L_s and a summation order that depends on
 * n_points alone: best_sym and grad repeat bit for bit. */
long dim_pm_sym_workspace_bytes(int B, int n_points, int max_sym);
int dim_pm_sym_loss_grad(const float* p_est, const float* points_model, const float* weights, const float* tgt_pose, const float* sym,
                         const int* sym_off, int n_classes, const int* class_index, int B, int n_points, int max_sym, float norm_term,
                         float grad_scale, int loss_type, float smooth_l1_scalar, void* workspace, float* grad, float* target_out,
                         int* best_sym, float* loss_sum, int* status, void* stream);
/* SE3_DIST_LOSS (deepIM_flownet.py:396-437): rot_loss = 1 - (rot_gt . rot_est_norm)^2 with grad_scale LW_ROT and trans_loss =
 * TRANS_LOSS_TYPE(zoom_trans_est - zoom_trans_gt) with grad_scale LW_TRANS; zoom_trans_est = trans_w fc7 + trans_b is recomputed from
 * fc7 (B,256).  The gradients are ADDED to d_rot_norm (B,4) / d_zoom_trans (B,3), the inputs of dim_pose_head_bwd; loss_sums2 (2
 * floats, may be NULL) accumulate the un-scaled rot / trans loss sums (metrics Rot_L2Loss / Trans_L2Loss). */
int dim_se3_dist_loss_grad(const float* rot_est_norm, const float* rot_gt, const float* fc7, const float* trans_w, const float* trans_b,
                           const float* zoom_trans_gt, float* d_rot_norm, float* d_zoom_trans, int B, float lw_rot, float lw_trans,
                           int trans_loss_type, float smooth_l1_scalar, float* loss_sums2, void* stream);
/* L2Normalization(instance, eps 1e-10) of the quaternion head; backward of the pose head down to dz6 (B,256) */
int dim_quat_normalize(const float* rot, float* rot_norm, int B, void* stream);
int dim_pose_head_bwd(const float* fc6a, const float* fc7, const float* rot_raw, const float* d_rot_norm, const float* d_trans,
                      const float* fc7_w, const float* rot_w, const float* trans_w, float* d_rot, float* dz7, float* dz6, int B,
                      void* stream);
int dim_fc_wgrad(const float* dz, const float* x, float* dW, float* db, int B, int Out, int In, void* stream);
/* fc6's weight gradient straight in the MXNet layout: dW (Out, C*H*W flattened (c, h, w)) = dz (B, Out)^T . x (B, H, W, C NHWC), for batches
 * of 1 .. 32 rows, C % 16 == 0, H * W <= 80 (fc6: 8 x 10 x 1024 -> 256).  f32 products, summed over the batch in row order.  Replaces
 * dim_conv2d_wgrad(KH = H, KW = W) + dim_fc_unpack_weight: one 84 MB write instead of a packed intermediate and its conversion. */
int dim_fc_wgrad_nhwc(const float* dz, const float* x, float* dW, int B, int Out, int C, int H, int W, void* stream);
int dim_upsample16_bwd(const float* dout_nchw, const float* w_c1_32_32, float* df_nhwc, int N, int C, int h, int w, int OH, int OW, int crop,
                       float scale, void* stream);
long dim_conv_small_cout_bwd_workspace_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW);
int dim_conv_small_cout_bwd(const float* x, const float* dy, const float* w_oihw, float* dx, float* dw_oihw, float* db, float* workspace,
                            int N, int H, int W, int Cin, int in_cstride, int dx_cstride, int Cout, int KH, int KW, int pad,
                            int accumulate_dx, void* stream);
int dim_deconv4x4s2_tiny_bwd(const float* x, int x_cstride, const float* dy, int dy_cstride, int dy_coff, const float* w_iohw, float* dx,
                             float* dw_iohw, float* db, int N, int H, int W, int Cin, int Cout, int OH, int OW, int crop, void* stream);
/* mx.optimizer.SGD: mom = momentum*mom - lr*(rescale_grad*g + wd*w); w += mom */
int dim_sgd_momentum(float* w, const float* grad, float* mom, long n, float lr, float momentum, float wd, float rescale_grad, void* stream);
/* mx.optimizer.Adam step (deepim/train.py:338-375 selects it with TRAIN.optimizer == "adam"): lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t)
 * is computed by the caller from the update count t; mean / var are the two state tensors. */
int dim_adam(float* w, const float* grad, float* mean, float* var, long n, float lr_t, float beta1, float beta2, float epsilon, float wd,
             float rescale_grad, void* stream);
/* FullyConnected weight (Out, C*H*W) [mx Flatten order c,h,w] -> [(h,w,c)][Out] so fc6 is dim_conv2d_fwd
 * with KH=H, KW=W on the NHWC feature map. */
int dim_fc_pack_weight(const float* w_out_in, float* w_packed, int Out, int C, int H, int W, void* stream);
/* fc7 + LeakyReLU(0.1) + rot(4) + trans(3) + inverse ZoomTrans -> se3 (B,7)  (deepIM_flownet.py:203-208,:956-971).
 * weights in the reference (out,in) layout; fc7_out (B,256) optional. */
int dim_pose_head_fwd(const float* fc6, const float* fc7_w, const float* fc7_b, const float* rot_w, const float* rot_b,
                      const float* trans_w, const float* trans_b, const float* zoom_factor, float* se3, float* fc7_out, int B,
                      void* stream);

/* ---------------------------------------------------------------- per-class pose regressors (network.REGRESSOR_NUM = K > 1)
 * One `rot` / `trans` head per object class behind the shared fc6 / fc7: rot_w (4K,256), rot_b (4K), trans_w (3K,256), trans_b (3K),
 * class c owning rows 4c .. 4c+3 of rot and 3c .. 3c+2 of trans (one FullyConnected(num_hidden = 4K) reshaped to (B,K,4) and picked
 * by class).  The four entries below are dim_pose_head_fwd, dim_pose_head_bwd, dim_se3_dist_loss_grad and dim_fc_wgrad with
 * class_index (B int32, device) and n_regressors = K after the weights; sample b uses the rows of class class_index[b].
 *   - no allocation, no synchronisation (graph-capturable); class_index is read when the kernel runs, so a captured graph replayed
 *     after new classes are written there uses the new heads
 *   - n_regressors == 1: class_index may be NULL, and the call IS the un-suffixed entry (same kernel, same bits)
 *   - any K: sample b's outputs are bit for bit what the un-suffixed entry gives with class c_b's slice of rot / trans (same
 *     dot-product order, same shuffle tree); class c's rows of dim_fc_wgrad_cls are bit for bit dim_fc_wgrad over the samples of
 *     class c in their original order.  dim_fc_wgrad_cls writes EVERY element of dW (K*Out,In) and db (K*Out, may be NULL): zeros in
 *     the rows of a class that the batch does not hold (MXNet's dense FullyConnected gradient); no atomics, sums in ascending b
 *   - a class index outside [0, K), K > 1: dim_pose_head_fwd_cls writes the identity delta (1,0,0,0,0,0,0) (fc7_out as usual) and ORs
 *     DIM_STATUS_BAD_CLASS into status[b] (B int32, may be NULL); dim_pose_head_bwd_cls gives the sample zero d_rot / dz7 / dz6
 *     rows; dim_se3_dist_loss_grad_cls adds nothing to its rows of d_rot_norm / d_zoom_trans and nothing to loss_sums2;
 *     dim_fc_wgrad_cls skips the sample
 *   - n_regressors < 1, or class_index == NULL with n_regressors > 1: DIM_ERR_ARG before anything is enqueued */
int dim_pose_head_fwd_cls(const float* fc6, const float* fc7_w, const float* fc7_b, const float* rot_w, const float* rot_b,
                          const float* trans_w, const float* trans_b, const int* class_index, int n_regressors,
                          const float* zoom_factor, float* se3, float* fc7_out, int* status, int B, void* stream);
int dim_pose_head_bwd_cls(const float* fc6a, const float* fc7, const float* rot_raw, const float* d_rot_norm, const float* d_trans,
                          const float* fc7_w, const float* rot_w, const float* trans_w, const int* class_index, int n_regressors,
                          float* d_rot, float* dz7, float* dz6, int B, void* stream);
int dim_se3_dist_loss_grad_cls(const float* rot_est_norm, const float* rot_gt, const float* fc7, const float* trans_w,
                               const float* trans_b, const int* class_index, int n_regressors, const float* zoom_trans_gt,
                               float* d_rot_norm, float* d_zoom_trans, int B, float lw_rot, float lw_trans, int trans_loss_type,
                               float smooth_l1_scalar, float* loss_sums2, void* stream);
int dim_fc_wgrad_cls(const float* dz, const float* x, const int* class_index, int n_regressors, float* dW, float* db, int B, int Out,
                     int In, void* stream);

/* ---------------------------------------------------------------- resident refinement loop (hosts without torch)
 * The inner loop of pred_eval (deepim/core/tester.py:476-598) for a batch of B 480x640 pairs (dim_refiner_create_src: pairs of another
 * 4:3 size) that stays in HBM, FAST_TEST graph,
 * UPDATE_MASK 'box_rendered': per iteration ZoomMask + ZoomImageWithFactor + Concat -> encoder -> fc6/fc7/rot/trans -> RT_transform
 * -> render -> box mask.  dim_refiner_create packs the weights (MXNet-layout device arrays given by name: <layer>_weight / _bias of
 * the ten encoder layers, fc6, fc7, rot, trans; the bias / fc7 / rot / trans arrays are read in place and must outlive the object),
 * allocates every buffer and fixes the launch plan; dim_refiner_run only enqueues kernels on `stream` (no allocation, no sync: it
 * may be captured into a hipGraph) and never writes its six input blobs.  Outputs: poses_iter (test_iter,B,3,4), se3_iter
 * (test_iter,B,7), status_iter (test_iter,B) with the DIM_STATUS_* bits.  The mesh table pointers must outlive the object. */
typedef struct dim_refiner dim_refiner;
typedef struct {
  int B, H, W, test_iter;
  float K9[9];
  float pixel_means_bgr[3]; /* config.network.PIXEL_MEANS, in its B,G,R order */
  float T_means[3], T_stds[3];
  int rot_coord; /* 0 MODEL, 1 CAMERA, 2 CAMERA_NEW, 3 NAIVE */
  float znear, zfar;
  int tex_bilinear;
  const float* verts;
  const float* uvs;
  const int* faces;
  const int* mesh_table;
  int n_classes, vmax, fmax;
  const unsigned char* textures;
  const int* tex_table;
} dim_refiner_desc;
int dim_refiner_create(dim_refiner** out, const dim_refiner_desc* desc, const char* const* param_names, const float* const* param_ptrs,
                       int n_params, void* stream);
/* dim_refiner_create with per-class pose regressors: n_regressors = 1 (this is dim_refiner_create) or desc->n_classes, the rot /
 * trans arrays then holding (4 n_classes,256) / (4 n_classes) / (3 n_classes,256) / (3 n_classes) floats (dim_pose_head_fwd_cls);
 * dim_refiner_run / _run_k pick every pair's head by the class_index they already receive, read when the kernels run. */
int dim_refiner_create_cls(dim_refiner** out, const dim_refiner_desc* desc, int n_regressors, const char* const* param_names,
                           const float* const* param_ptrs, int n_params, void* stream);
/* dim_refiner_create_cls for a camera image of another size: desc->H x desc->W is the SOURCE size of the six blobs (4:3, H * 640 ==
 * W * 480, both >= 2) and desc->K9 the camera of that image; the network input stays 480 x 640.  The rendered planes, the box masks,
 * the boxes and the zoom window live at the source size, X and the encoder at the network size (dim_zoom_net_input_src between them).
 * dim_refiner_run / _run_k take the object as they take the others; their blobs are then (B,.,H,W) of the desc. */
int dim_refiner_create_src(dim_refiner** out, const dim_refiner_desc* desc, int n_regressors, const char* const* param_names,
                           const float* const* param_ptrs, int n_params, void* stream);
/* The zoom filter of a refiner made by any of the create functions: max_taps 0 or 1 = one bilinear sample per network pixel (the
 * default), 2..8 = the area filter (dim_zoom_net_input_area with that max_taps, also for 480 x 640 blobs, whose windows may be larger
 * than the frame).  Call it before the first dim_refiner_run / _run_k (and so before a graph capture of one): later it is refused. */
int dim_refiner_set_zoom_filter(dim_refiner* r, int max_taps);
int dim_refiner_run(dim_refiner* r, const float* image_observed, const float* image_rendered, const float* mask_observed,
                    const float* mask_rendered, const float* src_pose, const int* class_index, float* poses_iter, float* se3_iter,
                    int* status_iter, void* stream);
/* dim_refiner_run with one camera per pair (deepim/core/tester.py:165, :560-562: each re-render uses the pair's -K.txt when the
 * dataset ships one).  K_per_pair: device (B,9) f32, row-major; NULL = the desc's K9 (then this is dim_refiner_run).  As in the
 * reference, only the re-render reads it: ZoomMask / dim_zoom_factor keep desc.K9 (the reference's op attribute).  The array is read
 * when the kernels run, so a captured graph replayed after new values are written there renders with the new cameras. */
int dim_refiner_run_k(dim_refiner* r, const float* image_observed, const float* image_rendered, const float* mask_observed,
                      const float* mask_rendered, const float* src_pose, const int* class_index, float* poses_iter, float* se3_iter,
                      int* status_iter, const float* K_per_pair, void* stream);
int dim_refiner_destroy(dim_refiner* r);

#ifdef __cplusplus
}
#endif
#endif /* DEEPIM_HIP_H_ */
