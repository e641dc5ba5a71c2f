// Visible surface discrepancy (VSD) of T pose sets of B pairs on the device, restated in numpy by lib/utils/pose_error.py vsd()
// on top of lib/utils/visibility.py and lib/utils/misc.py depth_im_to_dist_im; the arithmetic below follows them step by step.
//
// Per pose: the observed depth D_obs, the depth D_gt rendered at the ground truth and D_est rendered at the estimate (metres, 0 =
// no surface).  Per pixel, in float64: the distance from the camera centre S = sqrt((X X + Y Y) + d d) with X = ((x - cx) d) (1 / fx),
// Y = ((y - cy) d) (1 / fy); the model surface is visible where S_model > 0, S_obs > 0 and float32(S_model) - float32(S_obs) <= delta
// (a float32 comparison); the estimate is also visible where the ground truth is and S_est > 0.  On the intersection of the two
// visibility sets the cost is c = |S_gt - S_est| (step: c >= tau; tlinear: min(c (1 / tau), 1)), every other pixel of the union costs 1,
// and the error is the mean cost over the union (1 when the union is empty).
//
//   vsd_accumulate_kernel<V>  grid (kVsdBlocks, B, T), 256 lanes.  The plane is cut into chunks of 256 * V consecutive pixels; chunk c
//                             belongs to workgroup c % kVsdBlocks and pixel group c * 256 + lane to that lane, whatever the boxes
//                             say: with boxes a workgroup walks only the chunks that touch the rows of the union of the two render
//                             boxes and a lane skips a group whose columns lie outside it.  Both renders are 0 out there, such a
//                             pixel adds nothing, and every sum keeps its order: boxes or none, the result is the same bit for bit.
//                             V = 4: one 16-byte load per plane (W % 4 == 0 and 16-byte aligned planes), V = 1 otherwise.
//                             One read of the three planes serves all n_tau costs; no distance is ever written to memory.
//                             Lane sums (int32 counts, float64 costs) -> block_sum.h: a fixed order, no atomics.
//   vsd_finish_kernel         one lane per (t, b): the kVsdBlocks partials in order -> counts and e per tau.
//   vsd_grid_accumulate_kernel<V, NT> / vsd_grid_finish_kernel   dim_vsd_grid_errors: the step cost at up to 16 taus read from the row
//                             of the pair's class.  The same grid, chunks, lanes and box skipping (vsd_lane_pixels); per lane the 4
//                             counts and NT counters n_ge[k] = |{c >= tau_k}| in registers, all int32: wave shuffles, LDS across the 4
//                             waves, the kVsdBlocks partials in the finish kernel.  Integer sums have no order: no atomics, no float
//                             sum, e = ((double)n_ge + (double)(n_union - n_inter)) / (double)n_union is numpy's to the bit.
// Plain operators in numpy's order (the Makefile's -ffp-contract=off keeps them un-fused).  Nothing allocates or synchronises:
// the entry is graph-capturable.
#include "block_sum.h"
#include "common.h"

namespace dim {

constexpr int kVsdThreads = 256;
constexpr int kVsdBlocks = 16;                    // workgroups per (t, b)
constexpr int kVsdCounts = 4;                     // |visib_gt|, |union|, |inter|, |D_gt drawn|
constexpr int kVsdTerms = DIM_VSD_MAX_TAU + kVsdCounts;
constexpr int kVsdSlot = 12;                      // doubles per partial: 8 cost sums, 4 counts (exact in float64)

struct VsdParams {
  double K[9];
  double tau[DIM_VSD_MAX_TAU], inv_tau[DIM_VSD_MAX_TAU];
  float delta;
  int n_tau, cost_type;
};

// misc.py depth_im_to_dist_im for one pixel
__device__ __forceinline__ double vsd_dist(double xc, double yc, double ifx, double ify, float depth) {
  const double d = (double)depth;
  const double X = (xc * d) * ifx, Y = (yc * d) * ify;
  return sqrt((X * X + Y * Y) + d * d);
}

struct VsdAcc {
  int n_gt, n_union, n_inter, n_drawn;
  double cost[DIM_VSD_MAX_TAU];
};

// the visibility rule for one pixel at which a render drew: S_gt, S_est and the three sets
struct VsdVis {
  double s_gt, s_est;
  bool gt, vis_gt, vis_est;
};
__device__ __forceinline__ VsdVis vsd_visibility(float delta, double xc, double yc, double ifx, double ify, float d_obs, float d_gt,
                                                 float d_est) {
  VsdVis v;
  const double s_obs = vsd_dist(xc, yc, ifx, ify, d_obs);
  v.s_gt = vsd_dist(xc, yc, ifx, ify, d_gt);
  v.s_est = vsd_dist(xc, yc, ifx, ify, d_est);
  const bool obs = s_obs > 0.0, est = v.s_est > 0.0;   // a NaN fails, as numpy's comparison does
  v.gt = v.s_gt > 0.0;
  const float f_obs = (float)s_obs;
  v.vis_gt = obs && v.gt && ((float)v.s_gt - f_obs <= delta);
  v.vis_est = (obs && est && ((float)v.s_est - f_obs <= delta)) || (v.vis_gt && est);
  return v;
}

__device__ __forceinline__ void vsd_pixel(const VsdParams& p, double xc, double yc, double ifx, double ify, float d_obs, float d_gt,
                                          float d_est, VsdAcc& a) {
  if (d_gt == 0.f && d_est == 0.f) return;   // neither render drew here: not in the union, no square root
  const VsdVis vis = vsd_visibility(p.delta, xc, yc, ifx, ify, d_obs, d_gt, d_est);
  a.n_drawn += vis.gt ? 1 : 0;
  a.n_gt += vis.vis_gt ? 1 : 0;
  a.n_union += (vis.vis_gt || vis.vis_est) ? 1 : 0;
  if (vis.vis_gt && vis.vis_est) {
    a.n_inter += 1;
    const double c = fabs(vis.s_gt - vis.s_est);
#pragma unroll
    for (int k = 0; k < DIM_VSD_MAX_TAU; ++k) {
      if (k < p.n_tau) {
        double v;
        if (p.cost_type == DIM_VSD_COST_STEP) {
          v = c >= p.tau[k] ? 1.0 : 0.0;
        } else {
          v = c * p.inv_tau[k];
          v = v < 1.0 ? v : 1.0;   // np.minimum(., 1) for the finite c of two visible pixels
        }
        a.cost[k] += v;
      }
    }
  }
}

// The pixels of pair (t, b) = (blockIdx.z, blockIdx.y) that belong to this lane, in the lane's fixed order (see the top of the file):
// pixel(xc, yc, ifx, ify, d_obs, d_gt, d_est) for each of them.  K9: the camera of every pair when K_per_sample is NULL.
template <int V, class F>
__device__ __forceinline__ void vsd_lane_pixels(const float* __restrict__ depth_obs, const float* __restrict__ depth_gt,
                                                const float* __restrict__ depth_est, const double* K9,
                                                const double* __restrict__ K_per_sample, const int* __restrict__ bbox_gt,
                                                const int* __restrict__ bbox_est, int B, int H, int W, F&& pixel) {
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const double* K = K_per_sample ? K_per_sample + 9L * b : nullptr;
  const double fx = K ? K[0] : K9[0], fy = K ? K[4] : K9[4], cx = K ? K[2] : K9[2], cy = K ? K[5] : K9[5];
  const double ifx = 1.0 / fx, ify = 1.0 / fy;
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (bbox_gt && bbox_est) {   // {min_x, max_x, min_y, max_y}, empty = {W, -1, H, -1}: the union of an empty box and a box is the box
    const int* g = bbox_gt + 4L * b;
    const int* e = bbox_est + 4L * ((long)t * B + b);
    x0 = max(min(g[0], e[0]), 0); x1 = min(max(g[1], e[1]), W - 1);
    y0 = max(min(g[2], e[2]), 0); y1 = min(max(g[3], e[3]), H - 1);
  }
  if (x1 < x0 || y1 < y0) return;
  const long plane = (long)H * W;
  const float* po = depth_obs + (long)b * plane;
  const float* pg = depth_gt + (long)b * plane;
  const float* pe = depth_est + ((long)t * B + b) * plane;
  constexpr long kChunk = (long)kVsdThreads * V;
  const long c_first = ((long)y0 * W) / kChunk, c_last = ((long)y1 * W + (W - 1)) / kChunk;   // chunks that touch rows y0 .. y1
  // the first chunk >= c_first that belongs to this workgroup
  long c = c_first + (((long)blockIdx.x - c_first % kVsdBlocks) + kVsdBlocks) % kVsdBlocks;
  for (; c <= c_last; c += kVsdBlocks) {
    const long i = c * kChunk + (long)tid * V;   // first pixel of this lane's group; V == 4: W % 4 == 0, the group lies in one row
    if (i >= plane) continue;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    if (y < y0 || y > y1 || x + (V - 1) < x0 || x > x1) continue;
    const double yc = (double)y - cy;
    if (V == 4) {
      const float4 o = *reinterpret_cast<const float4*>(po + i), g = *reinterpret_cast<const float4*>(pg + i),
                   e = *reinterpret_cast<const float4*>(pe + i);
      pixel((double)x - cx, yc, ifx, ify, o.x, g.x, e.x);
      pixel((double)(x + 1) - cx, yc, ifx, ify, o.y, g.y, e.y);
      pixel((double)(x + 2) - cx, yc, ifx, ify, o.z, g.z, e.z);
      pixel((double)(x + 3) - cx, yc, ifx, ify, o.w, g.w, e.w);
    } else {
      pixel((double)x - cx, yc, ifx, ify, po[i], pg[i], pe[i]);
    }
  }
}

template <int V>
__global__ __launch_bounds__(kVsdThreads) void vsd_accumulate_kernel(const float* __restrict__ depth_obs, const float* __restrict__ depth_gt,
                                                                    const float* __restrict__ depth_est, VsdParams p,
                                                                    const double* __restrict__ K_per_sample,
                                                                    const int* __restrict__ bbox_gt, const int* __restrict__ bbox_est,
                                                                    int B, int H, int W, double* __restrict__ partial) {
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  VsdAcc a;
  a.n_gt = a.n_union = a.n_inter = a.n_drawn = 0;
#pragma unroll
  for (int k = 0; k < DIM_VSD_MAX_TAU; ++k) a.cost[k] = 0.0;
  vsd_lane_pixels<V>(depth_obs, depth_gt, depth_est, p.K, K_per_sample, bbox_gt, bbox_est, B, H, W,
                     [&](double xc, double yc, double ifx, double ify, float d_obs, float d_gt, float d_est) {
                       vsd_pixel(p, xc, yc, ifx, ify, d_obs, d_gt, d_est, a);
                     });
  // the counts ride along as float64: a plane has fewer than 2^31 pixels, so they stay exact
  double v[kVsdTerms];
#pragma unroll
  for (int k = 0; k < DIM_VSD_MAX_TAU; ++k) v[k] = a.cost[k];
  v[DIM_VSD_MAX_TAU + 0] = (double)a.n_gt;
  v[DIM_VSD_MAX_TAU + 1] = (double)a.n_union;
  v[DIM_VSD_MAX_TAU + 2] = (double)a.n_inter;
  v[DIM_VSD_MAX_TAU + 3] = (double)a.n_drawn;
  const double total = block_sum(v);
  if (tid < kVsdTerms) partial[((((long)t * B + b) * kVsdBlocks) + blockIdx.x) * kVsdSlot + tid] = total;
}

__global__ __launch_bounds__(64) void vsd_finish_kernel(const double* __restrict__ partial, int T, int B, int n_tau,
                                                        double* __restrict__ errors, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * B) return;
  double s[kVsdTerms];
#pragma unroll
  for (int k = 0; k < kVsdTerms; ++k) s[k] = 0.0;
  for (int j = 0; j < kVsdBlocks; ++j) {
    const double* q = partial + (i * kVsdBlocks + j) * kVsdSlot;
#pragma unroll
    for (int k = 0; k < kVsdTerms; ++k) s[k] += q[k];
  }
  const double n_union = s[DIM_VSD_MAX_TAU + 1], n_inter = s[DIM_VSD_MAX_TAU + 2];
#pragma unroll
  for (int k = 0; k < kVsdCounts; ++k) counts[kVsdCounts * i + k] = (int)s[DIM_VSD_MAX_TAU + k];
#pragma unroll
  for (int k = 0; k < DIM_VSD_MAX_TAU; ++k)
    if (k < n_tau) errors[(long)n_tau * i + k] = n_union > 0.0 ? (s[k] + (n_union - n_inter)) / n_union : 1.0;
}

// ---- BOP's grid: the step cost at up to DIM_VSD_GRID_MAX_TAU taus of the pair's class, as integer counts (see the header) ----
constexpr int kGridSlot = kVsdCounts + DIM_VSD_GRID_MAX_TAU;   // int32 per partial: the 4 counts, then n_ge per tau
constexpr int kVsdWaves = kVsdThreads / kWave;

struct VsdGridParams {
  double K[9];
  float delta;
  int n_tau, n_classes;
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// NT: the compile-time tau capacity (n_tau <= NT): the NT counters of a lane are registers, every loop over them is unrolled.  The taus
// are the same for the whole workgroup (one class per pair) and stay in scalar registers; a slot k >= n_tau holds NaN, which no c reaches.
template <int V, int NT>
__global__ __launch_bounds__(kVsdThreads) void vsd_grid_accumulate_kernel(const float* __restrict__ depth_obs,
                                                                         const float* __restrict__ depth_gt,
                                                                         const float* __restrict__ depth_est, VsdGridParams p,
                                                                         const double* __restrict__ K_per_sample,
                                                                         const int* __restrict__ bbox_gt, const int* __restrict__ bbox_est,
                                                                         const int* __restrict__ class_index,
                                                                         const double* __restrict__ tau_table, int B, int H, int W,
                                                                         int* __restrict__ partial) {
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const int cls = class_index[b];
  if (cls < 0 || cls >= p.n_classes) return;   // the finish kernel writes this pair's NaN row without reading a partial
  const double* row = tau_table + (long)cls * p.n_tau;
  double tau[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) tau[k] = k < p.n_tau ? row[k] : __builtin_nan("");
  int n[kVsdCounts + NT];   // {n_gt, n_union, n_inter, n_drawn}, n_ge[NT]
#pragma unroll
  for (int k = 0; k < kVsdCounts + NT; ++k) n[k] = 0;
  vsd_lane_pixels<V>(depth_obs, depth_gt, depth_est, p.K, K_per_sample, bbox_gt, bbox_est, B, H, W,
                     [&](double xc, double yc, double ifx, double ify, float d_obs, float d_gt, float d_est) {
                       if (d_gt == 0.f && d_est == 0.f) return;   // as vsd_pixel
                       const VsdVis vis = vsd_visibility(p.delta, xc, yc, ifx, ify, d_obs, d_gt, d_est);
                       n[3] += vis.gt ? 1 : 0;
                       n[0] += vis.vis_gt ? 1 : 0;
                       n[1] += (vis.vis_gt || vis.vis_est) ? 1 : 0;
                       if (vis.vis_gt && vis.vis_est) {
                         n[2] += 1;
                         const double c = fabs(vis.s_gt - vis.s_est);
#pragma unroll
                         for (int k = 0; k < NT; ++k) n[kVsdCounts + k] += c >= tau[k] ? 1 : 0;
                       }
                     });
  // lanes -> wave by shuffles, waves -> workgroup through LDS: integers, so any order gives the same sums
  __shared__ int red[kVsdWaves][kVsdCounts + NT];
#pragma unroll
  for (int k = 0; k < kVsdCounts + NT; ++k) {
    const int s = wave_sum_i32(n[k]);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave][k] = s;
  }
  __syncthreads();
  if (tid < kVsdCounts + NT) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kVsdWaves; ++w) s += red[w][tid];
    partial[((((long)t * B + b) * kVsdBlocks) + blockIdx.x) * kGridSlot + tid] = s;
  }
}

// one lane per (t, b): the kVsdBlocks partials -> counts, n_ge and e per tau; reads the slots k < 4 + n_tau, which the launch above wrote
__global__ __launch_bounds__(64) void vsd_grid_finish_kernel(const int* __restrict__ partial, const int* __restrict__ class_index,
                                                             int n_classes, int T, int B, int n_tau, double* __restrict__ errors,
                                                             int* __restrict__ counts, int* __restrict__ n_ge) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * B) return;
  const int cls = class_index[i % B];
  const bool known = cls >= 0 && cls < n_classes;
  int s[kGridSlot];
#pragma unroll
  for (int k = 0; k < kGridSlot; ++k) s[k] = 0;
  if (known) {
    for (int j = 0; j < kVsdBlocks; ++j) {
      const int* q = partial + (i * kVsdBlocks + j) * kGridSlot;
#pragma unroll
      for (int k = 0; k < kGridSlot; ++k)
        if (k < kVsdCounts + n_tau) s[k] += q[k];
    }
  }
#pragma unroll
  for (int k = 0; k < kVsdCounts; ++k) counts[kVsdCounts * i + k] = s[k];
  const int n_union = s[1], n_inter = s[2];
#pragma unroll
  for (int k = 0; k < DIM_VSD_GRID_MAX_TAU; ++k) {
    if (k < n_tau) {
      n_ge[(long)n_tau * i + k] = s[kVsdCounts + k];
      errors[(long)n_tau * i + k] = !known ? __builtin_nan("")
                                   : n_union > 0 ? ((double)s[kVsdCounts + k] + (double)(n_union - n_inter)) / (double)n_union : 1.0;
    }
  }
}

template <int NT>
static void vsd_grid_launch(bool vec, dim3 grid, hipStream_t st, const float* depth_obs, const float* depth_gt, const float* depth_est,
                            const VsdGridParams& p, const double* K_per_sample, const int* bbox_gt, const int* bbox_est,
                            const int* class_index, const double* tau_table, int B, int H, int W, int* partial) {
  if (vec)
    hipLaunchKernelGGL((vsd_grid_accumulate_kernel<4, NT>), grid, dim3(kVsdThreads), 0, st, depth_obs, depth_gt, depth_est, p, K_per_sample,
                       bbox_gt, bbox_est, class_index, tau_table, B, H, W, partial);
  else
    hipLaunchKernelGGL((vsd_grid_accumulate_kernel<1, NT>), grid, dim3(kVsdThreads), 0, st, depth_obs, depth_gt, depth_est, p, K_per_sample,
                       bbox_gt, bbox_est, class_index, tau_table, B, H, W, partial);
}

}  // namespace dim

using namespace dim;

extern "C" long dim_vsd_workspace_bytes(int T, int B) {
  if (T <= 0 || B <= 0) return 0;
  return (long)T * B * kVsdBlocks * kVsdSlot * (long)sizeof(double);
}

extern "C" int dim_vsd_errors(const float* depth_obs, const float* depth_gt, const float* depth_est, const double* K9_f64,
                              const double* K_per_sample_f64, const int* bbox_gt, const int* bbox_est, int T, int B, int H, int W,
                              float delta, const double* taus, int n_tau, int cost_type, void* workspace, double* errors, int* counts,
                              void* stream) {
  DIM_REQUIRE(T > 0 && B > 0 && T <= 65535 && B <= 65535, "vsd_errors: T = %d, B = %d", T, B);
  DIM_REQUIRE(H > 0 && W > 0, "vsd_errors: image %d x %d", H, W);
  DIM_REQUIRE(n_tau >= 1 && n_tau <= DIM_VSD_MAX_TAU, "vsd_errors: n_tau = %d outside [1, %d]", n_tau, DIM_VSD_MAX_TAU);
  DIM_REQUIRE(cost_type == DIM_VSD_COST_STEP || cost_type == DIM_VSD_COST_TLINEAR, "vsd_errors: cost_type = %d", cost_type);
  DIM_REQUIRE(depth_obs && depth_gt && depth_est && K9_f64 && taus && workspace && errors && counts, "vsd_errors: null pointer");
  DIM_REQUIRE((bbox_gt != nullptr) == (bbox_est != nullptr), "vsd_errors: both boxes or neither");
  DIM_REQUIRE(((uintptr_t)workspace % 8) == 0, "vsd_errors: workspace must be 8-byte aligned");
  VsdParams p;
  for (int k = 0; k < 9; ++k) p.K[k] = K9_f64[k];
  for (int k = 0; k < DIM_VSD_MAX_TAU; ++k) {
    p.tau[k] = k < n_tau ? taus[k] : 0.0;
    p.inv_tau[k] = k < n_tau ? 1.0 / taus[k] : 0.0;
  }
  p.delta = delta;
  p.n_tau = n_tau;
  p.cost_type = cost_type;
  double* partial = (double*)workspace;
  const dim3 grid(kVsdBlocks, B, T), fin(ceil_div((long)T * B, 64));
  hipStream_t st = as_stream(stream);
  const bool vec = W % 4 == 0 && (((uintptr_t)depth_obs | (uintptr_t)depth_gt | (uintptr_t)depth_est) % 16) == 0;
  if (vec)
    hipLaunchKernelGGL(vsd_accumulate_kernel<4>, grid, dim3(kVsdThreads), 0, st, depth_obs, depth_gt, depth_est, p, K_per_sample_f64, bbox_gt,
                       bbox_est, B, H, W, partial);
  else
    hipLaunchKernelGGL(vsd_accumulate_kernel<1>, grid, dim3(kVsdThreads), 0, st, depth_obs, depth_gt, depth_est, p, K_per_sample_f64, bbox_gt,
                       bbox_est, B, H, W, partial);
  hipLaunchKernelGGL(vsd_finish_kernel, fin, dim3(64), 0, st, (const double*)partial, T, B, n_tau, errors, counts);
  return check_launch("vsd_errors");
}

extern "C" long dim_vsd_grid_workspace_bytes(int T, int B) {
  if (T <= 0 || B <= 0) return 0;
  return (long)T * B * kVsdBlocks * kGridSlot * (long)sizeof(int);
}

extern "C" int dim_vsd_grid_errors(const float* depth_obs, const float* depth_gt, const float* depth_est, const double* K9_f64,
                                   const double* K_per_sample_f64, const int* bbox_gt, const int* bbox_est, const int* class_index,
                                   const double* tau_table, int n_classes, int n_tau, int T, int B, int H, int W, float delta,
                                   void* workspace, double* errors, int* counts, int* n_ge, void* stream) {
  DIM_REQUIRE(T > 0 && B > 0 && T <= 65535 && B <= 65535, "vsd_grid_errors: T = %d, B = %d", T, B);
  DIM_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31), "vsd_grid_errors: image %d x %d", H, W);   // int32 counts
  DIM_REQUIRE(n_tau >= 1 && n_tau <= DIM_VSD_GRID_MAX_TAU, "vsd_grid_errors: n_tau = %d outside [1, %d]", n_tau, DIM_VSD_GRID_MAX_TAU);
  DIM_REQUIRE(n_classes >= 1, "vsd_grid_errors: n_classes = %d", n_classes);
  DIM_REQUIRE(depth_obs && depth_gt && depth_est && K9_f64 && class_index && tau_table && workspace && errors && counts && n_ge,
              "vsd_grid_errors: null pointer");
  DIM_REQUIRE((bbox_gt != nullptr) == (bbox_est != nullptr), "vsd_grid_errors: both boxes or neither");
  DIM_REQUIRE(((uintptr_t)workspace % 8) == 0, "vsd_grid_errors: workspace must be 8-byte aligned");
  VsdGridParams p;
  for (int k = 0; k < 9; ++k) p.K[k] = K9_f64[k];
  p.delta = delta;
  p.n_tau = n_tau;
  p.n_classes = n_classes;
  int* partial = (int*)workspace;
  const dim3 grid(kVsdBlocks, B, T), fin(ceil_div((long)T * B, 64));
  hipStream_t st = as_stream(stream);
  const bool vec = W % 4 == 0 && (((uintptr_t)depth_obs | (uintptr_t)depth_gt | (uintptr_t)depth_est) % 16) == 0;
  const auto launch = n_tau <= 4 ? vsd_grid_launch<4> : n_tau <= 8 ? vsd_grid_launch<8> : n_tau <= 12 ? vsd_grid_launch<12> : vsd_grid_launch<16>;
  launch(vec, grid, st, depth_obs, depth_gt, depth_est, p, K_per_sample_f64, bbox_gt, bbox_est, class_index, tau_table, B, H, W, partial);
  hipLaunchKernelGGL(vsd_grid_finish_kernel, fin, dim3(64), 0, st, (const int*)partial, class_index, n_classes, T, B, n_tau, errors, counts,
                     n_ge);
  return check_launch("vsd_grid_errors");
}
