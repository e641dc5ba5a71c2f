// Pose errors of lib/utils/pose_error.py on the device, in float64 as numpy computes them: re (degrees), te, ADD, ADD-S (adi) and the
// 2-D reprojection error arp_2d, for T pose sets of B pairs against one ground truth per pair.
//
//   pose_err_kernel   grid (kErrBlocks, B, T), 256 lanes.  A workgroup walks the query tiles qt = blockIdx.x, + kErrBlocks, ... of its
//                     pair's class (kErrQTile = 512 model points, two per lane).  Per query point: g = R_g p + t_g, e = R_e p + t_e ->
//                     |e - g| (ADD) and the pixel distance of K e' and K g (arp_2d; e' under the flipped estimate when the class's
//                     flip rule applies).  ADD-S: every estimate point e_j is transformed once per workgroup as its tile of
//                     kErrCTile = 256 candidates is staged in LDS (three float64 planes, 6 KB); each lane reads a candidate as three
//                     8-byte broadcasts and keeps min_j |g - e_j|^2 for its two queries (sqrt is monotone: one sqrt per query).
//                     Lane sums -> xor butterfly -> waves in order -> one partial per workgroup (no atomics).
//   pose_err_finish   one lane per (t, b): the kErrBlocks partials in order, the means, re / te, NaN rows and the status bit.
// Transforms and projections in numpy's order of operations come from pose_geom.h (see there); the norms are sqrt of the sum of
// squares.
// Nothing allocates or synchronises: the entry is graph-capturable.
#include "block_sum.h"
#include "common.h"
#include "pose_geom.h"

namespace dim {

constexpr int kErrThreads = 256;
constexpr int kErrQPL = 2;                           // query points per lane: 18 f64 VALU ops per three LDS broadcasts
constexpr int kErrQTile = kErrThreads * kErrQPL;     // query points per workgroup pass
constexpr int kErrCTile = kErrThreads;               // candidates staged per LDS tile, one per lane
constexpr int kErrBlocks = 16;                       // workgroups per (t, b): the host does not know the class sizes
constexpr int kErrSlot = 4;                          // doubles per partial: add, arp_2d, adi, pad

// pose_error.re: degrees(arccos(clip((trace(R_est^T R_gt) - 1) / 2, -1, 1))); a NaN stays a NaN as np.clip keeps it
__device__ __forceinline__ double err_rot_deg(const double* Pe, const double* Pg) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) tr += (Pe[i] * Pg[i] + Pe[4 + i] * Pg[4 + i]) + Pe[8 + i] * Pg[8 + i];
  double c = (tr - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  return acos(c) * (180.0 / 3.14159265358979323846);
}

// evaluation.py's eggbox rule: est . RT_Z = [R diag(-1, -1, 1) | t] when the raw rotation error exceeds 90 degrees
__device__ __forceinline__ void err_flip_z180(double* P) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    P[4 * r] = -P[4 * r];
    P[4 * r + 1] = -P[4 * r + 1];
  }
}

// class of pair b -> first point, point count and flags; false: the row is NaN (index out of range, or a table that runs backwards)
__device__ __forceinline__ bool err_class(const int* __restrict__ table_off, const int* __restrict__ class_flags, int n_classes, int cls,
                                          int& off, int& n, int& flags) {
  flags = 0;
  if (!class_points(table_off, n_classes, cls, off, n)) return false;
  flags = class_flags[cls];
  if (off < 0 || n < 0) n = 0;
  return true;
}

template <typename PT>
__global__ __launch_bounds__(kErrThreads) void pose_err_kernel(const double* __restrict__ points, const int* __restrict__ table_off,
                                                               const int* __restrict__ class_flags, int n_classes,
                                                               const int* __restrict__ class_index, const PT* __restrict__ poses_est,
                                                               const double* __restrict__ pose_gt, CamK K, int B,
                                                               double* __restrict__ partial) {
  __shared__ double cand[3][kErrCTile];
  __shared__ double red[kErrThreads / kWave][3];
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  int off, n, flags;
  const bool valid = err_class(table_off, class_flags, n_classes, class_index[b], off, n, flags);
  double s_add = 0.0, s_arp = 0.0, s_adi = 0.0;
  const int ntiles = valid ? (n + kErrQTile - 1) / kErrQTile : 0;
  if ((int)blockIdx.x < ntiles) {   // workgroup-uniform: the barriers below are reached by every lane or by none
    double Pe[12], Pg[12], Pf[12];
    load_pose(poses_est + 12L * ((long)t * B + b), Pe);
    load_pose(pose_gt + 12L * b, Pg);
#pragma unroll
    for (int k = 0; k < 12; ++k) Pf[k] = Pe[k];
    if ((flags & DIM_POSE_ERR_FLIP_Z180) && err_rot_deg(Pe, Pg) > 90.0) err_flip_z180(Pf);
    const double* pts = points + 3L * off;
    const bool adi = (flags & DIM_POSE_ERR_ADI) != 0;
    for (int qt = blockIdx.x; qt < ntiles; qt += kErrBlocks) {
      double gx[kErrQPL], gy[kErrQPL], gz[kErrQPL], best[kErrQPL];
      bool ok[kErrQPL];
#pragma unroll
      for (int q = 0; q < kErrQPL; ++q) {
        const int i = qt * kErrQTile + q * kErrThreads + tid;
        ok[q] = i < n;
        const double x = ok[q] ? pts[3L * i] : 0.0, y = ok[q] ? pts[3L * i + 1] : 0.0, z = ok[q] ? pts[3L * i + 2] : 0.0;
        double ex, ey, ez, fx, fy, fz, ue, ve, ug, vg;
        transform(Pg, x, y, z, gx[q], gy[q], gz[q]);
        transform(Pe, x, y, z, ex, ey, ez);
        transform(Pf, x, y, z, fx, fy, fz);
        project(K, fx, fy, fz, ue, ve);
        project(K, gx[q], gy[q], gz[q], ug, vg);
        const double dx = ex - gx[q], dy = ey - gy[q], dz = ez - gz[q], du = ue - ug, dv = ve - vg;
        if (ok[q]) {
          s_add += sqrt((dx * dx + dy * dy) + dz * dz);
          s_arp += sqrt(du * du + dv * dv);
        }
        best[q] = INFINITY;
      }
      if (adi) {
        for (int c0 = 0; c0 < n; c0 += kErrCTile) {
          __syncthreads();   // the previous tile has been read by every wave
          const int j = c0 + tid;
          if (j < n) {
            double ex, ey, ez;
            transform(Pe, pts[3L * j], pts[3L * j + 1], pts[3L * j + 2], ex, ey, ez);
            cand[0][tid] = ex;
            cand[1][tid] = ey;
            cand[2][tid] = ez;
          }
          __syncthreads();
          const int m = min(kErrCTile, n - c0);
#pragma unroll 4
          for (int c = 0; c < m; ++c) {
            const double cx = cand[0][c], cy = cand[1][c], cz = cand[2][c];
#pragma unroll
            for (int q = 0; q < kErrQPL; ++q) {
              const double dx = gx[q] - cx, dy = gy[q] - cy, dz = gz[q] - cz;
              best[q] = fmin(best[q], (dx * dx + dy * dy) + dz * dz);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < kErrQPL; ++q)
          if (ok[q]) s_adi += sqrt(best[q]);
      }
    }
  }
  // lanes: xor butterfly (the same order on every run); waves: in wave order through LDS
  const double w_add = wave_sum(s_add), w_arp = wave_sum(s_arp), w_adi = wave_sum(s_adi);
  const int wave = tid / kWave, lane = tid % kWave;
  if (lane == 0) {
    red[wave][0] = w_add;
    red[wave][1] = w_arp;
    red[wave][2] = w_adi;
  }
  __syncthreads();
  if (tid < 3) {
    double v = red[0][tid];
    for (int w = 1; w < kErrThreads / kWave; ++w) v += red[w][tid];
    partial[(((long)t * B + b) * kErrBlocks + blockIdx.x) * kErrSlot + tid] = v;
  }
}

template <typename PT>
__global__ __launch_bounds__(64) void pose_err_finish(const int* __restrict__ table_off, const int* __restrict__ class_flags, int n_classes,
                                                      const int* __restrict__ class_index, const PT* __restrict__ poses_est,
                                                      const double* __restrict__ pose_gt, int T, int B,
                                                      const double* __restrict__ partial, double* __restrict__ errors,
                                                      int* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * B) return;
  const int b = (int)(i % B);
  int off, n, flags;
  const bool valid = err_class(table_off, class_flags, n_classes, class_index[b], off, n, flags);
  double* e = errors + 5L * i;
  if (!valid || n == 0) {
    for (int k = 0; k < 5; ++k) e[k] = NAN;
    if (!valid && status && i < B) status[b] |= DIM_STATUS_BAD_CLASS;   // one lane per pair (t = 0) touches status[b]
    return;
  }
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < kErrBlocks; ++j) {
    const double* q = partial + (i * kErrBlocks + j) * kErrSlot;
    for (int k = 0; k < 3; ++k) s[k] += q[k];
  }
  double Pe[12], Pg[12];
  load_pose(poses_est + 12L * i, Pe);
  load_pose(pose_gt + 12L * b, Pg);
  double re = err_rot_deg(Pe, Pg);
  if ((flags & DIM_POSE_ERR_FLIP_Z180) && re > 90.0) {
    err_flip_z180(Pe);   // the translation of est . RT_Z is the estimate's
    re = err_rot_deg(Pe, Pg);
  }
  const double dx = Pg[3] - Pe[3], dy = Pg[7] - Pe[7], dz = Pg[11] - Pe[11];
  e[0] = re;
  e[1] = sqrt((dx * dx + dy * dy) + dz * dz);
  e[2] = s[0] / (double)n;
  e[3] = (flags & DIM_POSE_ERR_ADI) ? s[2] / (double)n : NAN;
  e[4] = s[1] / (double)n;
}

}  // namespace dim

using namespace dim;

extern "C" long dim_pose_errors_workspace_bytes(int T, int B, int max_points) {
  if (T <= 0 || B <= 0 || max_points < 0) return 0;
  return (long)T * B * kErrBlocks * kErrSlot * (long)sizeof(double);   // the candidates live in LDS: independent of max_points
}

extern "C" int dim_pose_errors(const double* points, const int* table_off, const int* class_flags, int n_classes, const int* class_index,
                               const float* poses_est, const double* poses_est_f64, const double* pose_gt, const double* K9_f64, int T,
                               int B, void* workspace, double* errors, int* status, void* stream) {
  DIM_REQUIRE(T > 0 && B > 0 && n_classes > 0 && T <= 65535 && B <= 65535, "pose_errors: T = %d, B = %d, n_classes = %d", T, B, n_classes);
  DIM_REQUIRE((poses_est != nullptr) != (poses_est_f64 != nullptr), "pose_errors: exactly one of poses_est / poses_est_f64");
  DIM_REQUIRE(points && table_off && class_flags && class_index && pose_gt && K9_f64 && workspace && errors, "pose_errors: null pointer");
  DIM_REQUIRE(((uintptr_t)workspace % 8) == 0, "pose_errors: workspace must be 8-byte aligned");
  CamK K;
  for (int k = 0; k < 9; ++k) K.k[k] = K9_f64[k];
  double* partial = (double*)workspace;
  const dim3 grid(kErrBlocks, B, T), fin(ceil_div((long)T * B, 64));
  hipStream_t st = as_stream(stream);
  if (poses_est) {
    hipLaunchKernelGGL(pose_err_kernel<float>, grid, dim3(kErrThreads), 0, st, points, table_off, class_flags, n_classes, class_index,
                       poses_est, pose_gt, K, B, partial);
    hipLaunchKernelGGL(pose_err_finish<float>, fin, dim3(64), 0, st, table_off, class_flags, n_classes, class_index, poses_est, pose_gt, T,
                       B, (const double*)partial, errors, status);
  } else {
    hipLaunchKernelGGL(pose_err_kernel<double>, grid, dim3(kErrThreads), 0, st, points, table_off, class_flags, n_classes, class_index,
                       poses_est_f64, pose_gt, K, B, partial);
    hipLaunchKernelGGL(pose_err_finish<double>, fin, dim3(64), 0, st, table_off, class_flags, n_classes, class_index, poses_est_f64,
                       pose_gt, T, B, (const double*)partial, errors, status);
  }
  return check_launch("pose_errors");
}
