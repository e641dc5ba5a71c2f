// Projective point-to-plane ICP, model to frame, after the refinement loop (RGB-D test time).  Restated in float64 numpy by
// tests/icp_reference.py; the arithmetic below follows it step by step.
//
// Per pair b: the source points are the pixels of the rendered depth D_r (inside the render's bbox) back-projected with the pair's
// K; each iteration moves them by the current correction T_delta, projects them into the observed depth D_o, takes the observed
// point q there and the normal n of its four neighbours, and linearises r = n . (p - q) in the twist (omega, v): J = (p x n, n).
//   icp_accumulate_kernel  grid (kIcpBlocks, B): per lane float32 sums of the 21 + 6 + 2 terms, float64 across lanes and (in
//                          icp_solve_kernel) workgroups, always in the same order: no atomics, a replay is bit-identical
//   icp_solve_kernel       one workgroup per pair: sums the partials, Cholesky in float64, T_delta <- [Rodrigues(omega) | v] T_delta,
//                          stats / status, and after the last iteration pose_out = T_delta T0
// Two launches per iteration; nothing allocates or synchronises, so the stage is graph-capturable.
#include "common.h"
#include "twist_solve.h"

namespace dim {

constexpr int kIcpBlocks = 16;   // workgroups per pair: 4096 lanes over the bbox (a LINEMOD object covers 5k-80k pixels)
constexpr int kIcpTerms = 29;    // 21 upper-triangle entries of sum J J^T, 6 of sum J r, inlier count, sum r^2
constexpr int kIcpSlot = 32;     // doubles per partial (padded)
constexpr int kIcpState = 16;    // doubles per pair: R_delta (9), t_delta (3), updated (1), pad
constexpr int kIcpMinPoints = 64;
constexpr int kIcpRow = 8 * 33;  // LDS doubles per term in the cross-lane sum

struct IcpCam {
  float fx, fy, cx, cy;
};

__device__ __forceinline__ IcpCam icp_camera(const float* __restrict__ K_per_sample, IcpCam k9, int b) {
  if (!K_per_sample) return k9;
  const float* k = K_per_sample + 9 * b;
  return IcpCam{k[0], k[4], k[2], k[5]};
}

__global__ __launch_bounds__(256) void icp_accumulate_kernel(const float* __restrict__ depth_r, const float* __restrict__ depth_o,
                                                             const float* __restrict__ mask_o, const int* __restrict__ bbox,
                                                             IcpCam k9, const float* __restrict__ K_per_sample, int H, int W,
                                                             float max_dist, int it, const double* __restrict__ state,
                                                             double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const IcpCam c = icp_camera(K_per_sample, k9, b);
  const bool cam_ok = c.fx > 0.f && c.fy > 0.f && isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy);
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
  if (it > 0) {
    const double* s = state + (long)b * kIcpState;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (float)s[9 + k];
  }
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (bbox) {
    x0 = max(bbox[4 * b + 0], 0); x1 = min(bbox[4 * b + 1], W - 1);
    y0 = max(bbox[4 * b + 2], 0); y1 = min(bbox[4 * b + 3], H - 1);
  }
  const int bw = x1 - x0 + 1;
  const int n = (cam_ok && x1 >= x0 && y1 >= y0) ? bw * (y1 - y0 + 1) : 0;
  const long plane = (long)H * W;
  const float* dr = depth_r + (long)b * plane;
  const float* dob = depth_o + (long)b * plane;
  const float* mob = mask_o ? mask_o + (long)b * plane : nullptr;
  const float md2 = max_dist * max_dist;
  float acc[kIcpTerms];
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) acc[k] = 0.f;
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kIcpBlocks * blockDim.x) {
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
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int e = a; e < 6; ++e) acc[k++] += J[a] * J[e];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
    acc[27] += 1.f;
    acc[28] += r * r;
  }
  // float64 from here on, in a fixed order: 8 chunks of 32 lanes per term (a chunk row padded to 33 doubles against bank conflicts),
  // then the 8 chunk sums.  (A shuffle butterfly per term -- 29 chains of 6 dependent 64-bit lane exchanges -- cost more than the pixels.)
  __shared__ double red[kIcpTerms * kIcpRow];
  __shared__ double red8[kIcpTerms * 8];
  const int slot = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int k = 0; k < kIcpTerms; ++k) red[k * kIcpRow + slot] = (double)acc[k];
  __syncthreads();
  if (tid < kIcpTerms * 8) {
    const double* r = red + (tid >> 3) * kIcpRow + (tid & 7) * 33;
    double s = 0.0;
    for (int j = 0; j < 32; ++j) s += r[j];
    red8[tid] = s;
  }
  __syncthreads();
  if (tid < kIcpTerms) {
    double s = red8[8 * tid];
    for (int w = 1; w < 8; ++w) s += red8[8 * tid + w];
    partial[((long)b * kIcpBlocks + blockIdx.x) * kIcpSlot + tid] = s;
  }
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ partial, double* __restrict__ state, int it, int iters,
                                                      const float* __restrict__ pose_in, float* __restrict__ pose_out,
                                                      float* __restrict__ stats, int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[kIcpTerms];
  if (tid < kIcpTerms) {
    double v = 0.0;
    for (int k = 0; k < kIcpBlocks; ++k) v += partial[((long)b * kIcpBlocks + k) * kIcpSlot + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double* st = state + (long)b * kIcpState;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, updated = 0.0;
  if (it > 0) {
    for (int k = 0; k < 9; ++k) R[k] = st[k];
    for (int k = 0; k < 3; ++k) t[k] = st[9 + k];
    updated = st[12];
  }
  const double N = s[27], rr = s[28];
  if (stats) {
    stats[((long)b * iters + it) * 2 + 0] = (float)N;
    stats[((long)b * iters + it) * 2 + 1] = N > 0.0 ? (float)sqrt(rr / N) : 0.f;
  }
  bool ok = N >= (double)kIcpMinPoints;
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
    status[b] |= DIM_STATUS_ICP_FEW_POINTS;
  }
  for (int k = 0; k < 9; ++k) st[k] = R[k];
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = updated;
  if (it == iters - 1) {
    const float* T0 = pose_in + 12 * (long)b;
    float* out = pose_out + 12 * (long)b;
    if (updated == 0.0) {   // never moved: the input pose, bit for bit
      for (int k = 0; k < 12; ++k) out[k] = T0[k];
      return;
    }
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j)
        out[4 * i + j] = (float)(R[3 * i] * (double)T0[j] + R[3 * i + 1] * (double)T0[4 + j] + R[3 * i + 2] * (double)T0[8 + j]);
      out[4 * i + 3] = (float)(R[3 * i] * (double)T0[3] + R[3 * i + 1] * (double)T0[7] + R[3 * i + 2] * (double)T0[11] + t[i]);
    }
  }
}

}  // namespace dim

using namespace dim;

extern "C" long dim_icp_workspace_bytes(int B, int H, int W) {
  (void)H;
  (void)W;
  if (B <= 0) return 0;
  return (long)B * (kIcpState + kIcpBlocks * kIcpSlot) * (long)sizeof(double);
}

extern "C" int dim_icp_refine(const float* depth_rendered, const float* depth_observed, const float* mask_observed, const int* bbox,
                              const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int iters,
                              float max_dist, void* workspace, float* pose_out, float* stats, int* status, void* stream) {
  DIM_REQUIRE(B > 0, "icp_refine: B = %d", B);
  DIM_REQUIRE(iters >= 0, "icp_refine: iters = %d", iters);
  DIM_REQUIRE(max_dist > 0.f, "icp_refine: max_dist must be > 0");
  DIM_REQUIRE(H >= 3 && W >= 3, "icp_refine: image %d x %d is smaller than 3 x 3", H, W);
  DIM_REQUIRE(depth_rendered && depth_observed && pose_in && K9 && workspace && pose_out, "icp_refine: null pointer");
  if (iters == 0) return dim_copy_words(pose_out, pose_in, 12L * B, stream);
  const IcpCam k9{K9[0], K9[4], K9[2], K9[5]};
  double* state = (double*)workspace;
  double* partial = state + (long)B * kIcpState;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(icp_accumulate_kernel, dim3(kIcpBlocks, B), dim3(256), 0, as_stream(stream), depth_rendered, depth_observed,
                       mask_observed, bbox, k9, K_per_sample, H, W, max_dist, it, (const double*)state, partial);
    hipLaunchKernelGGL(icp_solve_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const double*)partial, state, it, iters, pose_in,
                       pose_out, stats, status);
  }
  return check_launch("icp_refine");
}
