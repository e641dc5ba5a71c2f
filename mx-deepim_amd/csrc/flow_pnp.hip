// Pose from predicted flow: a deterministic robust PnP in place of cv2.solvePnPRansac of the reference's flow2se3
// (lib/pair_matching/flow2se3.py:13-56).  Restated in float64 numpy by tests/flow_pnp_reference.py; the arithmetic below follows it
// step by step.
//
// Per pair b: every pixel (x, y) of the rendered depth D_r inside the render's bbox with D_r > 0, a finite flow and (when given)
// valid >= 0.5 AT THE SOURCE PIXEL gives the 3-D point p = d ((x - cx)/fx, (y - cy)/fy, 1) and the target (u, v) = (x, y) + flow
// (dropped outside [-0.5, W - 0.5] x [-0.5, H - 0.5]).  Gauss-Newton on T = [R | t] from the identity: m = R p + t,
// r = (fx m_x/m_z + cx - u, fy m_y/m_z + cy - v), weights 1 in the first `warm` iterations (at the identity the residual is the
// flow itself), then Huber (huber_px) under a hard gate (max_px); Jacobian in the left twist (omega, v), dm = omega x m + v.
//   flow_pnp_accumulate_kernel  grid (kGnBlocks, B): four pixels per lane (16-byte loads where the rows allow them), float64 per
//                               point and per lane, summed across lanes (block_sum.h) and, in the solve kernel, workgroups in a
//                               fixed order: no atomics, a replay is bit-identical
//   gn_solve_kernel             (twist_solve.h) one workgroup per pair: sums the partials, Cholesky in float64,
//                               T <- [Rodrigues(omega) | v] T, stats / status, and after the last iteration pose_out = T pose_src
//                               and se3_q = [quat(R), t]
// Two launches per iteration; nothing allocates or synchronises, so the stage is graph-capturable.
// Float64 per point, not float32: the stage is bound by its 2 x iters dependent launches, not by arithmetic (a pair has 5k-80k
// points), and the gate decision e > max_px then agrees with the restatement's, so the inlier counts are equal, not close.
#include "common.h"
#include "twist_solve.h"

namespace dim {

typedef float v4f __attribute__((ext_vector_type(4)));

// VEC: W % 4 == 0 and 16-byte aligned planes, so the four pixels x4 .. x4 + 3 of a row are one 16-byte load per plane
template <bool VEC>
__global__ __launch_bounds__(256) void flow_pnp_accumulate_kernel(const float* __restrict__ depth_r, const float* __restrict__ flow,
                                                                  const float* __restrict__ valid, const int* __restrict__ bbox,
                                                                  PinholeCam k9, const float* __restrict__ K_per_sample, int H, int W,
                                                                  int comp_x, int it, int warm, float huber_px, float max_px,
                                                                  const double* __restrict__ state, double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const PinholeCam c = cam_pick(K_per_sample, k9, b);
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  double R[9], t[3];
  gn_load_pose(state, b, it, R, t);
  const PixelBox box = clamp_bbox(bbox, b, H, W);
  const int x0 = box.x0, x1 = box.x1, y0 = box.y0, y1 = box.y1;
  const int xq0 = x0 & ~3;                       // the quads are aligned to 4 pixels in the row
  const int nq = ((x1 | 3) + 1 - xq0) >> 2;      // quads per row
  const int n = (cam_ok(c) && x1 >= x0 && y1 >= y0) ? nq * (y1 - y0 + 1) : 0;
  const long plane = (long)H * W;
  const float* dr = depth_r + (long)b * plane;
  const float* fxp = flow + ((long)b * 2 + comp_x) * plane;         // the x component: plane 1 in (dy, dx) order
  const float* fyp = flow + ((long)b * 2 + (1 - comp_x)) * plane;
  const float* vp = valid ? valid + (long)b * plane : nullptr;
  const bool gated = it >= warm;
  const double hub = huber_px, gate = max_px;
  const double u_hi = (double)W - 0.5, v_hi = (double)H - 0.5;
  double acc[kGnTerms];
#pragma unroll
  for (int k = 0; k < kGnTerms; ++k) acc[k] = 0.0;
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kGnBlocks * blockDim.x) {
    const int qy = i / nq;
    const int y = y0 + qy, x4 = xq0 + 4 * (i - qy * nq);
    const long o = (long)y * W + x4;
    float d[4], fu[4], fv[4], va[4] = {1.f, 1.f, 1.f, 1.f};
    if (VEC) {   // x4 + 3 < W because W % 4 == 0
      const v4f d4 = *reinterpret_cast<const v4f*>(dr + o);
      d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
      if (!(d[0] > 0.f || d[1] > 0.f || d[2] > 0.f || d[3] > 0.f)) continue;
      const v4f a4 = *reinterpret_cast<const v4f*>(fxp + o), b4 = *reinterpret_cast<const v4f*>(fyp + o);
      fu[0] = a4.x; fu[1] = a4.y; fu[2] = a4.z; fu[3] = a4.w;
      fv[0] = b4.x; fv[1] = b4.y; fv[2] = b4.z; fv[3] = b4.w;
      if (vp) {
        const v4f m4 = *reinterpret_cast<const v4f*>(vp + o);
        va[0] = m4.x; va[1] = m4.y; va[2] = m4.z; va[3] = m4.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = x4 + k <= x1;   // x1 <= W - 1: nothing is read past the row
        d[k] = in ? dr[o + k] : 0.f;
        fu[k] = in ? fxp[o + k] : 0.f;
        fv[k] = in ? fyp[o + k] : 0.f;
        if (vp) va[k] = in ? vp[o + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x4 + k;
      if (x < x0 || x > x1) continue;
      if (!(d[k] > 0.f) || !isfinite(fu[k]) || !isfinite(fv[k]) || !(va[k] >= 0.5f)) continue;
      const double u = (double)x + (double)fu[k], v = (double)y + (double)fv[k];
      if (!(u >= -0.5 && u <= u_hi && v >= -0.5 && v <= v_hi)) continue;
      const double z = d[k];
      const double sx = z * ((double)x - cx) / fx, sy = z * ((double)y - cy) / fy;
      const double mx = R[0] * sx + R[1] * sy + R[2] * z + t[0];
      const double my = R[3] * sx + R[4] * sy + R[5] * z + t[1];
      const double mz = R[6] * sx + R[7] * sy + R[8] * z + t[2];
      if (!(mz > 0.0)) continue;
      const double rx = fx * mx / mz + cx - u, ry = fy * my / mz + cy - v;
      const double e2 = rx * rx + ry * ry;
      double w = 1.0;
      if (gated) {
        const double e = sqrt(e2);
        if (e > gate) continue;   // w = 0
        if (!(e <= hub)) w = hub / e;
      }
      gn_add_pixel(acc, fx, fy, mx, my, mz, rx, ry, w, e2);
    }
  }
  gn_store_partial(acc, partial, b);
}

// iters == 0: se3_q of a pair that never updated
__global__ void flow_pnp_identity_kernel(float* __restrict__ se3_q, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 7 * B) se3_q[i] = i % 7 == 0 ? 1.f : 0.f;
}

}  // namespace dim

using namespace dim;

extern "C" long dim_flow_pnp_workspace_bytes(int B, int H, int W) {
  (void)H;
  (void)W;
  return gn_workspace_bytes(B);
}

extern "C" int dim_flow_pnp(const float* depth_rendered, const float* flow, const float* valid, const int* bbox, const float* pose_src,
                            const float* K9, const float* K_per_sample, int B, int H, int W, int standard_rep, int iters, int warm,
                            float huber_px, float max_px, void* workspace, float* pose_out, float* se3_q, float* stats, int* status,
                            void* stream) {
  DIM_REQUIRE(B > 0, "flow_pnp: B = %d", B);
  DIM_REQUIRE(iters >= 0, "flow_pnp: iters = %d", iters);
  DIM_REQUIRE(warm >= 0, "flow_pnp: warm = %d", warm);
  DIM_REQUIRE(huber_px > 0.f, "flow_pnp: huber_px must be > 0");
  DIM_REQUIRE(max_px >= huber_px, "flow_pnp: max_px must be >= huber_px");
  DIM_REQUIRE(H > 0 && W > 0, "flow_pnp: image %d x %d", H, W);
  DIM_REQUIRE(depth_rendered && flow && pose_src && K9 && workspace && pose_out, "flow_pnp: null pointer");
  if (iters == 0) {
    if (se3_q) hipLaunchKernelGGL(flow_pnp_identity_kernel, dim3(ceil_div(7L * B, 256)), dim3(256), 0, as_stream(stream), se3_q, B);
    return dim_copy_words(pose_out, pose_src, 12L * B, stream);
  }
  const PinholeCam k9 = cam_of_k9(K9);
  const GnWorkspace ws(workspace, B);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = W % 4 == 0 && al16(depth_rendered) && al16(flow) && (!valid || al16(valid));
  const int comp_x = standard_rep ? 0 : 1;   // (dy, dx) unless standard_rep
  gn_iterate<DIM_STATUS_FLOW_PNP_FEW_POINTS>(ws, B, iters, pose_src, pose_out, se3_q, stats, status, as_stream(stream), [&](int it) {
    hipLaunchKernelGGL(vec ? flow_pnp_accumulate_kernel<true> : flow_pnp_accumulate_kernel<false>, dim3(kGnBlocks, B), dim3(256), 0,
                       as_stream(stream), depth_rendered, flow, valid, bbox, k9, K_per_sample, H, W, comp_x, it, warm, huber_px, max_px,
                       (const double*)ws.state, ws.partial);
  });
  return check_launch("flow_pnp");
}
