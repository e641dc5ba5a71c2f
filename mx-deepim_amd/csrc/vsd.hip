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

__device__ __forceinline__ void vsd_pixel(const VsdParams& p, double xc, double yc, double ifx, double ify, float d_obs, float d_gt,
                                          float d_est, VsdAcc& a) {
  if (d_gt == 0.f && d_est == 0.f) return;   // neither render drew here: not in the union, no square root
  const double s_obs = vsd_dist(xc, yc, ifx, ify, d_obs), s_gt = vsd_dist(xc, yc, ifx, ify, d_gt), s_est = vsd_dist(xc, yc, ifx, ify, d_est);
  const bool obs = s_obs > 0.0, gt = s_gt > 0.0, est = s_est > 0.0;   // a NaN fails, as numpy's comparison does
  const float f_obs = (float)s_obs;
  const bool vis_gt = obs && gt && ((float)s_gt - f_obs <= p.delta);
  const bool vis_est = (obs && est && ((float)s_est - f_obs <= p.delta)) || (vis_gt && est);
  a.n_drawn += gt ? 1 : 0;
  a.n_gt += vis_gt ? 1 : 0;
  a.n_union += (vis_gt || vis_est) ? 1 : 0;
  if (vis_gt && vis_est) {
    a.n_inter += 1;
    const double c = fabs(s_gt - s_est);
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

template <int V>
__global__ __launch_bounds__(kVsdThreads) void vsd_accumulate_kernel(const float* __restrict__ depth_obs, const float* __restrict__ depth_gt,
                                                                    const float* __restrict__ depth_est, VsdParams p,
                                                                    const double* __restrict__ K_per_sample,
                                                                    const int* __restrict__ bbox_gt, const int* __restrict__ bbox_est,
                                                                    int B, int H, int W, double* __restrict__ partial) {
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const double* K = K_per_sample ? K_per_sample + 9L * b : nullptr;
  const double fx = K ? K[0] : p.K[0], fy = K ? K[4] : p.K[4], cx = K ? K[2] : p.K[2], cy = K ? K[5] : p.K[5];
  const double ifx = 1.0 / fx, ify = 1.0 / fy;
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (bbox_gt && bbox_est) {   // {min_x, max_x, min_y, max_y}, empty = {W, -1, H, -1}: the union of an empty box and a box is the box
    const int* g = bbox_gt + 4L * b;
    const int* e = bbox_est + 4L * ((long)t * B + b);
    x0 = max(min(g[0], e[0]), 0); x1 = min(max(g[1], e[1]), W - 1);
    y0 = max(min(g[2], e[2]), 0); y1 = min(max(g[3], e[3]), H - 1);
  }
  const long plane = (long)H * W;
  const float* po = depth_obs + (long)b * plane;
  const float* pg = depth_gt + (long)b * plane;
  const float* pe = depth_est + ((long)t * B + b) * plane;
  VsdAcc a;
  a.n_gt = a.n_union = a.n_inter = a.n_drawn = 0;
#pragma unroll
  for (int k = 0; k < DIM_VSD_MAX_TAU; ++k) a.cost[k] = 0.0;
  if (x1 >= x0 && y1 >= y0) {
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
        vsd_pixel(p, (double)x - cx, yc, ifx, ify, o.x, g.x, e.x, a);
        vsd_pixel(p, (double)(x + 1) - cx, yc, ifx, ify, o.y, g.y, e.y, a);
        vsd_pixel(p, (double)(x + 2) - cx, yc, ifx, ify, o.z, g.z, e.z, a);
        vsd_pixel(p, (double)(x + 3) - cx, yc, ifx, ify, o.w, g.w, e.w, a);
      } else {
        vsd_pixel(p, (double)x - cx, yc, ifx, ify, po[i], pg[i], pe[i], a);
      }
    }
  }
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
