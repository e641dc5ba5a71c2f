// Projective point-to-plane ICP, model to frame, after the refinement loop (RGB-D test time).  Restated in float64 numpy by
// tests/icp_reference.py; the arithmetic below follows it step by step.
//
// Per pair b: the source points are the pixels of the rendered depth D_r (inside the render's bbox) back-projected with the pair's
// K; each iteration moves them by the current correction T_delta, projects them into the observed depth D_o, takes the observed
// point q there and the normal n of its four neighbours, and linearises r = n . (p - q) in the twist (omega, v): J = (p x n, n).
//   icp_accumulate_kernel  grid (kGnBlocks, B): per lane float32 sums of the 21 + 6 + 2 terms, float64 across lanes (block_sum.h)
//                          and, in the solve kernel, workgroups, always in the same order: no atomics, a replay is bit-identical
//   gn_solve_kernel        (twist_solve.h) one workgroup per pair: sums the partials, Cholesky in float64,
//                          T_delta <- [Rodrigues(omega) | v] T_delta, stats / status, and after the last iteration pose_out = T_delta T0
//   gn_solve_views_kernel  (twist_solve.h) in its place for dim_icp_refine_views: one workgroup per group of V calibrated views
//   gn_rig_group_kernel, gn_rig_solve_kernel  (twist_solve.h) in its place for dim_icp_refine_rig: the rig's extrinsics refined along
// Two launches per iteration (three for dim_icp_refine_rig); nothing allocates or synchronises, so the stage is graph-capturable.
#include "common.h"
#include "twist_solve.h"

namespace dim {

__global__ __launch_bounds__(256) void icp_accumulate_kernel(const float* __restrict__ depth_r, const float* __restrict__ depth_o,
                                                             const float* __restrict__ mask_o, const int* __restrict__ bbox,
                                                             PinholeCam k9, const float* __restrict__ K_per_sample, int H, int W,
                                                             float max_dist, int it, const double* __restrict__ state,
                                                             double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const PinholeCam c = cam_pick(K_per_sample, k9, b);
  float R[9], t[3];
  gn_load_pose(state, b, it, R, t);
  const PixelBox box = clamp_bbox(bbox, b, H, W);
  const int x0 = box.x0, x1 = box.x1, y0 = box.y0, y1 = box.y1;
  const int bw = x1 - x0 + 1;
  const int n = (cam_ok(c) && x1 >= x0 && y1 >= y0) ? bw * (y1 - y0 + 1) : 0;
  const long plane = (long)H * W;
  const float* dr = depth_r + (long)b * plane;
  const float* dob = depth_o + (long)b * plane;
  const float* mob = mask_o ? mask_o + (long)b * plane : nullptr;
  const float md2 = max_dist * max_dist;
  float acc[kGnTerms];
#pragma unroll
  for (int k = 0; k < kGnTerms; ++k) acc[k] = 0.f;
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kGnBlocks * blockDim.x) {
    const int yy = i / bw;
    const int x = x0 + (i - yy * bw), y = y0 + yy;
    const float d = dr[(long)y * W + x];
    if (!(d > 0.f)) continue;
    // source point (the render at T0), moved by T_delta
    const float sx = d * ((float)x - c.cx) / c.fx, sy = d * ((float)y - c.cy) / c.fy, sz = d;
    const float px = R[0] * sx + R[1] * sy + R[2] * sz + t[0];
    const float py = R[3] * sx + R[4] * sy + R[5] * sz + t[1];
    const float pz = R[6] * sx + R[7] * sy + R[8] * sz + t[2];
    if (!(pz > 0.f)) continue;
    const float uf = floorf(c.fx * px / pz + c.cx + 0.5f), vf = floorf(c.fy * py / pz + c.cy + 0.5f);
    if (!(uf >= 1.f && uf <= (float)(W - 2) && vf >= 1.f && vf <= (float)(H - 2))) continue;   // NaN fails too
    const int u = (int)uf, v = (int)vf;
    const long o = (long)v * W + u;
    const float zq = dob[o];
    if (!(zq > 0.f)) continue;
    if (mob && !(mob[o] >= 0.5f)) continue;
    const float zr = dob[o + 1], zl = dob[o - 1], zd = dob[o + W], zu = dob[o - W];
    if (!(zr > 0.f && fabsf(zr - zq) < max_dist && zl > 0.f && fabsf(zl - zq) < max_dist && zd > 0.f && fabsf(zd - zq) < max_dist &&
          zu > 0.f && fabsf(zu - zq) < max_dist))
      continue;
    const float fu = (float)u, fv = (float)v;
    const float qx = zq * (fu - c.cx) / c.fx, qy = zq * (fv - c.cy) / c.fy, qz = zq;
    // central differences (q(u+1) - q(u-1)) x (q(v+1) - q(v-1))
    const float ax = zr * (fu + 1.f - c.cx) / c.fx - zl * (fu - 1.f - c.cx) / c.fx;
    const float ay = zr * (fv - c.cy) / c.fy - zl * (fv - c.cy) / c.fy;
    const float az = zr - zl;
    const float bx = zd * (fu - c.cx) / c.fx - zu * (fu - c.cx) / c.fx;
    const float by = zd * (fv + 1.f - c.cy) / c.fy - zu * (fv - 1.f - c.cy) / c.fy;
    const float bz = zd - zu;
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float nn = nx * nx + ny * ny + nz * nz;
    if (!(nn > 1e-20f)) continue;
    const float nl = sqrtf(nn);
    nx = nx / nl; ny = ny / nl; nz = nz / nl;
    if (nx * qx + ny * qy + nz * qz > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
    const float ex = px - qx, ey = py - qy, ez = pz - qz;
    if (ex * ex + ey * ey + ez * ez > md2) continue;
    const float r = nx * ex + ny * ey + nz * ez;
    const float J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    gn_add_row(acc, J, r);
    acc[27] += 1.f;
    acc[28] += r * r;
  }
  gn_store_partial(acc, partial, b);   // float64 from here on, in a fixed order
}

}  // namespace dim

using namespace dim;

extern "C" long dim_icp_workspace_bytes(int B, int H, int W) {
  (void)H;
  (void)W;
  return gn_workspace_bytes(B);
}

// all three entries: views == nullptr is dim_icp_refine, rig != nullptr (with views) dim_icp_refine_rig
static int icp_run(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox, const float* pose_in,
                   const float* K9, const float* K_per_sample, int B, int H, int W, int iters, float max_dist, void* workspace,
                   float* pose_out, float* stats, int* status, const GnViews* views, const GnRig* rig, void* stream) {
  DIM_REQUIRE(B > 0, "icp_refine: B = %d", B);
  DIM_REQUIRE(iters >= 0, "icp_refine: iters = %d", iters);
  DIM_REQUIRE(max_dist > 0.f, "icp_refine: max_dist must be > 0");
  DIM_REQUIRE(H >= 3 && W >= 3, "icp_refine: image %d x %d is smaller than 3 x 3", H, W);
  DIM_REQUIRE(depth_rendered && depth_observed && pose_in && K9 && workspace && pose_out, "icp_refine: null pointer");
  DIM_REQUIRE(!views || gn_views_ok(*views, B), "icp_refine_views: V in 1 .. %d dividing B = %d, cam_T_rig, pose_rig_in and pose_rig_out required",
              kGnMaxViews, B);
  DIM_REQUIRE(!rig || (views && rig->cam_T_rig_out), "icp_refine_rig: cam_T_rig_out required");
  if (iters == 0) {
    int rc = dim_copy_words(pose_out, pose_in, 12L * B, stream);
    if (rc == DIM_OK && views) rc = dim_copy_words(views->pose_rig_out, views->pose_rig_in, 12L * (B / views->V), stream);
    return (rc != DIM_OK || !rig) ? rc : dim_copy_words(rig->cam_T_rig_out, views->cam_T_rig, 12L * B, stream);
  }
  const PinholeCam k9 = cam_of_k9(K9);
  const GnWorkspace ws(workspace, B);
  double* group_state = (double*)((char*)workspace + gn_workspace_bytes(B));
  const auto accumulate = [&](int it) {
    hipLaunchKernelGGL(icp_accumulate_kernel, dim3(kGnBlocks, B), dim3(256), 0, as_stream(stream), depth_rendered, depth_observed,
                       mask_observed, bbox, k9, K_per_sample, H, W, max_dist, it, (const double*)ws.state, ws.partial);
  };
  if (rig)
    gn_iterate_rig<DIM_STATUS_ICP_FEW_POINTS>(ws, group_state, B, *views, *rig, iters, pose_in, pose_out, stats, status, as_stream(stream),
                                              accumulate);
  else
    gn_iterate_either<DIM_STATUS_ICP_FEW_POINTS>(ws, group_state, B, views, iters, pose_in, pose_out, stats, status, as_stream(stream),
                                                 accumulate);
  return check_launch(rig ? "icp_refine_rig" : views ? "icp_refine_views" : "icp_refine");
}

extern "C" int dim_icp_refine(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                              const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters,
                              float max_dist, void* workspace, float* pose_out, float* stats, int* status, void* stream) {
  return icp_run(depth_rendered, depth_observed, mask_observed, bbox, pose_in, K9, K_per_sample, B, H, W, iters, max_dist, workspace, pose_out,
                 stats, status, nullptr, nullptr, stream);
}

extern "C" long dim_icp_views_workspace_bytes(int B, int H, int W, int V) {
  (void)H;
  (void)W;
  return (B <= 0 || V <= 0) ? 0 : gn_workspace_bytes(B) + gn_views_state_bytes(B, V);
}

extern "C" int dim_icp_refine_views(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                                    const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters,
                                    float max_dist, void* workspace, float* pose_out, float* stats, int* status, const float* cam_T_rig,
                                    int V, const float* pose_rig_in, float* pose_rig_out, float* stats_group, void* stream) {
  const GnViews views{cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group};
  return icp_run(depth_rendered, depth_observed, mask_observed, bbox, pose_in, K9, K_per_sample, B, H, W, iters, max_dist, workspace, pose_out,
                 stats, status, &views, nullptr, stream);
}

extern "C" long dim_icp_rig_workspace_bytes(int B, int H, int W, int V) {
  (void)H;
  (void)W;
  return (B <= 0 || V <= 0) ? 0 : gn_workspace_bytes(B) + gn_views_state_bytes(B, V) + gn_rig_state_bytes(B, V);
}

extern "C" int dim_icp_refine_rig(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                                  const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters,
                                  float max_dist, void* workspace, float* pose_out, float* stats, int* status, const float* cam_T_rig, int V,
                                  const float* pose_rig_in, float* pose_rig_out, float* stats_group, float* cam_T_rig_out,
                                  float* stats_view, void* stream) {
  const GnViews views{cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group};
  const GnRig rig{cam_T_rig_out, stats_view};
  return icp_run(depth_rendered, depth_observed, mask_observed, bbox, pose_in, K9, K_per_sample, B, H, W, iters, max_dist, workspace, pose_out,
                 stats, status, &views, &rig, stream);
}
