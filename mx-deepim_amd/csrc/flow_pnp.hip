// Pose from predicted flow: a deterministic robust PnP in place of cv2.solvePnPRansac of the reference's flow2se3
// (lib/pair_matching/flow2se3.py:13-56).  Restated in float64 numpy by tests/flow_pnp_reference.py; the arithmetic below follows it
// step by step.
//
// Per pair b: every pixel (x, y) of the rendered depth D_r inside the render's bbox with D_r > 0, a finite flow and (when given)
// valid >= 0.5 AT THE SOURCE PIXEL gives the 3-D point p = d ((x - cx)/fx, (y - cy)/fy, 1) and the target (u, v) = (x, y) + flow
// (dropped outside [-0.5, W - 0.5] x [-0.5, H - 0.5]).  Gauss-Newton on T = [R | t] from the identity: m = R p + t,
// r = (fx m_x/m_z + cx - u, fy m_y/m_z + cy - v), weights 1 in the first `warm` iterations (at the identity the residual is the
// flow itself), then Huber (huber_px) under a hard gate (max_px); Jacobian in the left twist (omega, v), dm = omega x m + v.
//   flow_pnp_accumulate_kernel  grid (kPnpBlocks, B): four pixels per lane (16-byte loads where the rows allow them), float64 per
//                               point and per lane, summed across lanes and (in the solve kernel) workgroups in a fixed order:
//                               no atomics, a replay is bit-identical
//   flow_pnp_solve_kernel       one workgroup per pair: sums the partials, Cholesky in float64, T <- [Rodrigues(omega) | v] T,
//                               stats / status, and after the last iteration pose_out = T pose_src and se3_q = [quat(R), t]
// Two launches per iteration; nothing allocates or synchronises, so the stage is graph-capturable.
// Float64 per point, not float32: the stage is bound by its 2 x iters dependent launches, not by arithmetic (a pair has 5k-80k
// points), and the gate decision e > max_px then agrees with the restatement's, so the inlier counts are equal, not close.
#include "common.h"
#include "twist_solve.h"

namespace dim {

constexpr int kPnpBlocks = 16;   // workgroups per pair: 4096 lanes x 4 pixels over the bbox
constexpr int kPnpTerms = 29;    // 21 upper-triangle entries of sum w J^T J, 6 of sum w J^T r, count of w > 0, sum e^2 over them
constexpr int kPnpSlot = 32;     // doubles per partial (padded)
constexpr int kPnpState = 16;    // doubles per pair: R (9), t (3), updated (1), pad
constexpr int kPnpMinPoints = 64;
constexpr int kPnpRow = 8 * 33;  // LDS doubles per term in the cross-lane sum

struct PnpCam {
  float fx, fy, cx, cy;
};

typedef float v4f __attribute__((ext_vector_type(4)));

// VEC: W % 4 == 0 and 16-byte aligned planes, so the four pixels x4 .. x4 + 3 of a row are one 16-byte load per plane
template <bool VEC>
__global__ __launch_bounds__(256) void flow_pnp_accumulate_kernel(const float* __restrict__ depth_r, const float* __restrict__ flow,
                                                                  const float* __restrict__ valid, const int* __restrict__ bbox,
                                                                  PnpCam k9, const float* __restrict__ K_per_sample, int H, int W,
                                                                  int comp_x, int it, int warm, float huber_px, float max_px,
                                                                  const double* __restrict__ state, double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  PnpCam c = k9;
  if (K_per_sample) {
    const float* k = K_per_sample + 9 * b;
    c = PnpCam{k[0], k[4], k[2], k[5]};
  }
  const bool cam_ok = c.fx > 0.f && c.fy > 0.f && isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy);
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (it > 0) {
    const double* s = state + (long)b * kPnpState;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = s[9 + k];
  }
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (bbox) {
    x0 = max(bbox[4 * b + 0], 0); x1 = min(bbox[4 * b + 1], W - 1);
    y0 = max(bbox[4 * b + 2], 0); y1 = min(bbox[4 * b + 3], H - 1);
  }
  const int xq0 = x0 & ~3;                       // the quads are aligned to 4 pixels in the row
  const int nq = ((x1 | 3) + 1 - xq0) >> 2;      // quads per row
  const int n = (cam_ok && x1 >= x0 && y1 >= y0) ? nq * (y1 - y0 + 1) : 0;
  const long plane = (long)H * W;
  const float* dr = depth_r + (long)b * plane;
  const float* fxp = flow + ((long)b * 2 + comp_x) * plane;         // the x component: plane 1 in (dy, dx) order
  const float* fyp = flow + ((long)b * 2 + (1 - comp_x)) * plane;
  const float* vp = valid ? valid + (long)b * plane : nullptr;
  const bool gated = it >= warm;
  const double hub = huber_px, gate = max_px;
  const double u_hi = (double)W - 0.5, v_hi = (double)H - 0.5;
  double acc[kPnpTerms];
#pragma unroll
  for (int k = 0; k < kPnpTerms; ++k) acc[k] = 0.0;
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kPnpBlocks * blockDim.x) {
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
      // d(pixel)/dm = [ax 0 bx; 0 ay by], dm = omega x m + v
      const double ax = fx / mz, bx = -fx * mx / (mz * mz), ay = fy / mz, by = -fy * my / (mz * mz);
      const double Jx[6] = {bx * my, ax * mz - bx * mx, -ax * my, ax, 0.0, bx};
      const double Jy[6] = {by * my - ay * mz, -by * mx, ay * mx, 0.0, ay, by};
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int e = a; e < 6; ++e) acc[q++] += w * (Jx[a] * Jx[e] + Jy[a] * Jy[e]);
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] += w * (Jx[a] * rx + Jy[a] * ry);
      acc[27] += 1.0;
      acc[28] += e2;
    }
  }
  // the cross-lane sum of icp.hip: 8 chunks of 32 lanes per term (a chunk row padded to 33 doubles against bank conflicts), then the
  // 8 chunk sums, always in the same order
  __shared__ double red[kPnpTerms * kPnpRow];
  __shared__ double red8[kPnpTerms * 8];
  const int slot = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int k = 0; k < kPnpTerms; ++k) red[k * kPnpRow + slot] = acc[k];
  __syncthreads();
  if (tid < kPnpTerms * 8) {
    const double* r = red + (tid >> 3) * kPnpRow + (tid & 7) * 33;
    double s = 0.0;
    for (int j = 0; j < 32; ++j) s += r[j];
    red8[tid] = s;
  }
  __syncthreads();
  if (tid < kPnpTerms) {
    double s = red8[8 * tid];
    for (int w = 1; w < 8; ++w) s += red8[8 * tid + w];
    partial[((long)b * kPnpBlocks + blockIdx.x) * kPnpSlot + tid] = s;
  }
}

__global__ __launch_bounds__(64) void flow_pnp_solve_kernel(const double* __restrict__ partial, double* __restrict__ state, int it,
                                                           int iters, const float* __restrict__ pose_src, float* __restrict__ pose_out,
                                                           float* __restrict__ se3_q, float* __restrict__ stats,
                                                           int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[kPnpTerms];
  if (tid < kPnpTerms) {
    double v = 0.0;
    for (int k = 0; k < kPnpBlocks; ++k) v += partial[((long)b * kPnpBlocks + k) * kPnpSlot + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double* st = state + (long)b * kPnpState;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, updated = 0.0;
  if (it > 0) {
    for (int k = 0; k < 9; ++k) R[k] = st[k];
    for (int k = 0; k < 3; ++k) t[k] = st[9 + k];
    updated = st[12];
  }
  const double N = s[27], ee = s[28];
  if (stats) {
    stats[((long)b * iters + it) * 2 + 0] = (float)N;
    stats[((long)b * iters + it) * 2 + 1] = N > 0.0 ? (float)sqrt(ee / N) : 0.f;
  }
  bool ok = N >= (double)kPnpMinPoints;
  double xi[6];
  if (ok) {
    double A[36], g[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int e = a; e < 6; ++e, ++k) A[6 * a + e] = A[6 * e + a] = s[k];
    const double damp = 1e-9 * (A[0] + A[7] + A[14] + A[21] + A[28] + A[35]) / 6.0;
    for (int a = 0; a < 6; ++a) {
      A[6 * a + a] += damp;
      g[a] = -s[21 + a];
    }
    ok = cholesky_solve6(A, g, xi);
  }
  if (ok) {
    double Rw[9], Rn[9], tn[3];
    twist_rodrigues(xi, Rw);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rn[3 * i + j] = Rw[3 * i] * R[j] + Rw[3 * i + 1] * R[3 + j] + Rw[3 * i + 2] * R[6 + j];
      tn[i] = Rw[3 * i] * t[0] + Rw[3 * i + 1] * t[1] + Rw[3 * i + 2] * t[2] + xi[3 + i];
    }
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
    updated = 1.0;
  } else if (status) {
    status[b] |= DIM_STATUS_FLOW_PNP_FEW_POINTS;
  }
  for (int k = 0; k < 9; ++k) st[k] = R[k];
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = updated;
  if (it != iters - 1) return;
  const float* T0 = pose_src + 12 * (long)b;
  float* out = pose_out + 12 * (long)b;
  float* sq = se3_q ? se3_q + 7 * (long)b : nullptr;
  if (updated == 0.0) {   // never moved: the input pose, bit for bit, and the identity
    for (int k = 0; k < 12; ++k) out[k] = T0[k];
    if (sq)
      for (int k = 0; k < 7; ++k) sq[k] = k == 0 ? 1.f : 0.f;
    return;
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out[4 * i + j] = (float)(R[3 * i] * (double)T0[j] + R[3 * i + 1] * (double)T0[4 + j] + R[3 * i + 2] * (double)T0[8 + j]);
    out[4 * i + 3] = (float)(R[3 * i] * (double)T0[3] + R[3 * i + 1] * (double)T0[7] + R[3 * i + 2] * (double)T0[11] + t[i]);
  }
  if (sq) {
    double q[4];
    mat2quat_d(R, q);
    for (int k = 0; k < 4; ++k) sq[k] = (float)q[k];
    for (int k = 0; k < 3; ++k) sq[4 + k] = (float)t[k];
  }
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
  if (B <= 0) return 0;
  return (long)B * (kPnpState + kPnpBlocks * kPnpSlot) * (long)sizeof(double);
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
  const PnpCam k9{K9[0], K9[4], K9[2], K9[5]};
  double* state = (double*)workspace;
  double* partial = state + (long)B * kPnpState;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = W % 4 == 0 && al16(depth_rendered) && al16(flow) && (!valid || al16(valid));
  const int comp_x = standard_rep ? 0 : 1;   // (dy, dx) unless standard_rep
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(vec ? flow_pnp_accumulate_kernel<true> : flow_pnp_accumulate_kernel<false>, dim3(kPnpBlocks, B), dim3(256), 0,
                       as_stream(stream), depth_rendered, flow, valid, bbox, k9, K_per_sample, H, W, comp_x, it, warm, huber_px, max_px,
                       (const double*)state, partial);
    hipLaunchKernelGGL(flow_pnp_solve_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const double*)partial, state, it, iters, pose_src,
                       pose_out, se3_q, stats, status);
  }
  return check_launch("flow_pnp");
}
