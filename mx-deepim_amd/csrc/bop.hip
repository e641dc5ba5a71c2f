// The two symmetry-aware pose errors of the BOP protocol on the device, in float64 as lib/utils/pose_error.py mssd / mspd compute them,
// for T pose sets of B pairs against one ground truth per pair and the symmetry set of the pair's class:
//   mssd = min over S of max over x of |(R_e x + t_e) - (R_g (S_R x + S_t) + t_g)|
//   mspd = the same with both points projected by K (R p + t) and divided by the third row, in pixels.
//
//   bop_err_kernel   grid (kBopBlocks, B, T), 256 lanes.  A workgroup walks the point tiles qt = blockIdx.x, + kBopBlocks, ... of its
//                    pair's class (kBopTile = 512 model points, two per lane).  A lane transforms and projects its two points under the
//                    estimate ONCE and keeps them in registers (10 doubles) across the symmetry loop, so the estimate's two divisions
//                    are not repeated per symmetry.  The symmetries go by in chunks of kBopChunk = 64: the workgroup composes
//                    M_s = pose_gt . S_s once per (pose, symmetry) into LDS (6 KB) and every lane reads a matrix as twelve 8-byte
//                    broadcasts.  Per symmetry: g = M_s x, the squared 3-D and pixel distances, the lane's maximum of each; the two
//                    maxima cross the wave in ONE butterfly (the first exchange hands the 3-D values to the lower and the pixel
//                    values to the upper half-wave), the four waves meet in LDS, and after the chunk one lane per (symmetry, error)
//                    writes the workgroup's maximum to the workspace (a second tile of the same workgroup joins what the first left).
//   bop_err_finish   grid (B, T), 256 lanes: per symmetry the maximum over the workgroups that had points, then the minimum and its
//                    index over the symmetries (lanes, waves), one sqrt per error, NaN rows and the status bit.
// Composing pose_gt . S once per symmetry instead of transforming every point twice changes a transformed point by about 1e-16
// relative (one rounding of each matrix entry instead of one of each intermediate coordinate).
// Maximum and minimum are exact in any order, so the result does not depend on how the points are dealt to lanes and workgroups; a NaN
// wins every maximum and every minimum as in numpy (np.max, np.argmin: the first NaN), ties go to the smaller index.  Squared
// distances are reduced and the square root is taken of the result only (monotone and correctly rounded: the same bits).
// Transforms and projections are pose_err_kernel's, from pose_geom.h (see there for the order of operations).  No atomics, nothing
// allocates or synchronises: the entry is graph-capturable, and the workspace needs no initialisation (only what this call wrote is
// read).
#include "common.h"
#include "pose_geom.h"

namespace dim {

constexpr int kBopThreads = 256;
constexpr int kBopWaves = kBopThreads / kWave;
constexpr int kBopQPL = 2;                           // points per lane: two independent chains per LDS matrix read
constexpr int kBopTile = kBopThreads * kBopQPL;      // points per workgroup pass
constexpr int kBopBlocks = 16;                       // workgroups per (t, b): the host does not know the class sizes
constexpr int kBopChunk = 64;                        // symmetries composed into LDS at a time

// np.max of two: a NaN on either side stays
__device__ __forceinline__ double bop_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }

struct BopClass {
  int off, n, soff, ns;
};

// class of pair b -> its points and its symmetries; 0: fine, 1: NaN row, 2: NaN row and DIM_STATUS_BAD_CLASS
__device__ __forceinline__ int bop_class(const int* __restrict__ table_off, const int* __restrict__ sym_off, int n_classes, int max_sym,
                                         int cls, BopClass& c) {
  c.soff = c.ns = 0;
  if (!class_points(table_off, n_classes, cls, c.off, c.n)) return 2;
  c.soff = sym_off[cls];
  c.ns = sym_off[cls + 1] - c.soff;
  if (c.off < 0 || c.n <= 0 || c.soff < 0 || c.ns <= 0 || c.ns > max_sym) return 1;
  return 0;
}

template <typename PT>
__global__ __launch_bounds__(kBopThreads) void bop_err_kernel(const double* __restrict__ points, const int* __restrict__ table_off,
                                                              const double* __restrict__ sym, const int* __restrict__ sym_off,
                                                              int n_classes, const int* __restrict__ class_index,
                                                              const PT* __restrict__ poses_est, const double* __restrict__ pose_gt,
                                                              CamK K_all, const double* __restrict__ K_per_sample, int B, int max_sym,
                                                              double* __restrict__ partial) {
  __shared__ double M[kBopChunk][12];
  __shared__ double red[kBopChunk][2][kBopWaves];
  const int t = blockIdx.z, b = blockIdx.y, tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid % kWave;
  BopClass c;
  if (bop_class(table_off, sym_off, n_classes, max_sym, class_index[b], c) != 0) return;
  const int ntiles = (c.n + kBopTile - 1) / kBopTile;
  if ((int)blockIdx.x >= ntiles) return;   // workgroup-uniform, like the return above: the barriers below are reached by all or none
  const CamK K = cam_k_pick(K_all, K_per_sample, b);
  double Pe[12];
  load_pose(poses_est + 12L * ((long)t * B + b), Pe);
  const double* pts = points + 3L * c.off;
  const double* Pg = pose_gt + 12L * b;
  const double* S_cls = sym + 12L * c.soff;
  double* out = partial + (((long)t * B + b) * kBopBlocks + blockIdx.x) * (long)max_sym * 2;
  const bool upper = lane >= kWave / 2;
  bool first = true;
  for (int qt = blockIdx.x; qt < ntiles; qt += kBopBlocks, first = false) {
    double x[kBopQPL], y[kBopQPL], z[kBopQPL], ex[kBopQPL], ey[kBopQPL], ez[kBopQPL], ue[kBopQPL], ve[kBopQPL];
#pragma unroll
    for (int q = 0; q < kBopQPL; ++q) {
      // a lane past the end takes the last point again: a repeated point changes no maximum
      const int i = min(qt * kBopTile + q * kBopThreads + tid, c.n - 1);
      x[q] = pts[3L * i];
      y[q] = pts[3L * i + 1];
      z[q] = pts[3L * i + 2];
      transform(Pe, x[q], y[q], z[q], ex[q], ey[q], ez[q]);
      project(K, ex[q], ey[q], ez[q], ue[q], ve[q]);
    }
    for (int s0 = 0; s0 < c.ns; s0 += kBopChunk) {
      const int m = min(kBopChunk, c.ns - s0);
      __syncthreads();   // the previous chunk's matrices and wave maxima have been read
      // M_s = pose_gt . S_s, entry by entry: [R_g S_R | R_g S_t + t_g]
      for (int e = tid; e < m * 12; e += kBopThreads) {
        const int s = e / 12, k = e % 12, r = k / 4, col = k % 4;
        const double* S = S_cls + 12L * (s0 + s);
        const double* g = Pg + 4 * r;
        double v = (g[0] * S[col] + g[1] * S[4 + col]) + g[2] * S[8 + col];
        if (col == 3) v += g[3];
        M[s][k] = v;
      }
      __syncthreads();
      for (int s = 0; s < m; ++s) {
        double Ms[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Ms[k] = M[s][k];
        double d3 = 0.0, d2 = 0.0;
#pragma unroll
        for (int q = 0; q < kBopQPL; ++q) {
          double gx, gy, gz, ug, vg;
          transform(Ms, x[q], y[q], z[q], gx, gy, gz);
          project(K, gx, gy, gz, ug, vg);
          const double dx = ex[q] - gx, dy = ey[q] - gy, dz = ez[q] - gz, du = ue[q] - ug, dv = ve[q] - vg;
          d3 = bop_nanmax(d3, (dx * dx + dy * dy) + dz * dz);
          d2 = bop_nanmax(d2, du * du + dv * dv);
        }
        // one butterfly for both: the lower half-wave collects the 3-D maxima, the upper half the pixel maxima
        double v = bop_nanmax(upper ? d2 : d3, __shfl_xor(upper ? d3 : d2, kWave / 2, kWave));
#pragma unroll
        for (int o = kWave / 4; o > 0; o >>= 1) v = bop_nanmax(v, __shfl_xor(v, o, kWave));
        if (lane == 0) red[s][0][wave] = v;
        if (lane == kWave / 2) red[s][1][wave] = v;
      }
      __syncthreads();
      if (tid < 2 * m) {
        const int s = tid >> 1, k = tid & 1;
        double v = red[s][k][0];
#pragma unroll
        for (int w = 1; w < kBopWaves; ++w) v = bop_nanmax(v, red[s][k][w]);
        double* o = out + 2L * (s0 + s) + k;
        if (!first) v = bop_nanmax(v, *o);   // written by this very lane on the previous tile
        *o = v;
      }
    }
  }
}

// the better of two (value, index) candidates for np.argmin: a NaN beats every number, equal values (and two NaNs) go to the smaller
// index; index INT_MAX = no candidate
__device__ __forceinline__ bool bop_better(double av, int ai, double bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av < bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(kBopThreads) void bop_err_finish(const int* __restrict__ table_off, const int* __restrict__ sym_off,
                                                              int n_classes, const int* __restrict__ class_index, int B, int max_sym,
                                                              const double* __restrict__ partial, double* __restrict__ errors,
                                                              int* __restrict__ best_sym, int* __restrict__ status) {
  __shared__ double red_v[2][kBopWaves];
  __shared__ int red_i[2][kBopWaves];
  const int t = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid % kWave;
  const long i = (long)t * B + b;
  BopClass c;
  const int bad = bop_class(table_off, sym_off, n_classes, max_sym, class_index[b], c);
  if (bad != 0) {   // workgroup-uniform
    if (tid < 2) {
      errors[2 * i + tid] = NAN;
      if (best_sym) best_sym[2 * i + tid] = -1;
    }
    if (bad == 2 && status && t == 0 && tid == 0) status[b] |= DIM_STATUS_BAD_CLASS;   // one lane per pair touches status[b]
    return;
  }
  const int nblk = min(kBopBlocks, (c.n + kBopTile - 1) / kBopTile);   // the workgroups that wrote
  const double* p = partial + i * kBopBlocks * (long)max_sym * 2;
  double bv[2] = {INFINITY, INFINITY};
  int bi[2] = {INT_MAX, INT_MAX};
  for (int s = tid; s < c.ns; s += kBopThreads) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double v = p[2L * s + k];
      for (int j = 1; j < nblk; ++j) v = bop_nanmax(v, p[((long)j * max_sym + s) * 2 + k]);
      if (bop_better(v, s, bv[k], bi[k])) {
        bv[k] = v;
        bi[k] = s;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv[k], o, kWave);
      const int oi = __shfl_xor(bi[k], o, kWave);
      if (bop_better(ov, oi, bv[k], bi[k])) {
        bv[k] = ov;
        bi[k] = oi;
      }
    }
    if (lane == 0) {
      red_v[k][wave] = bv[k];
      red_i[k][wave] = bi[k];
    }
  }
  __syncthreads();
  if (tid < 2) {
    double v = red_v[tid][0];
    int s = red_i[tid][0];
    for (int w = 1; w < kBopWaves; ++w)
      if (bop_better(red_v[tid][w], red_i[tid][w], v, s)) {
        v = red_v[tid][w];
        s = red_i[tid][w];
      }
    errors[2 * i + tid] = v != v ? NAN : sqrt(v);
    if (best_sym) best_sym[2 * i + tid] = s;
  }
}

}  // namespace dim

using namespace dim;

extern "C" long dim_bop_errors_workspace_bytes(int T, int B, int max_sym) {
  if (T <= 0 || B <= 0 || max_sym <= 0) return 0;
  return (long)T * B * kBopBlocks * max_sym * 2 * (long)sizeof(double);
}

extern "C" int dim_bop_errors(const double* points, const int* table_off, const double* sym, const int* sym_off, int n_classes,
                              const int* class_index, const float* poses_est, const double* poses_est_f64, const double* pose_gt,
                              const double* K9_f64, const double* K_per_sample_f64, int T, int B, int max_sym, void* workspace,
                              double* errors, int* best_sym, int* status, void* stream) {
  DIM_REQUIRE(T > 0 && B > 0 && n_classes > 0 && max_sym > 0 && T <= 65535 && B <= 65535,
              "bop_errors: T = %d, B = %d, n_classes = %d, max_sym = %d", T, B, n_classes, max_sym);
  DIM_REQUIRE((poses_est != nullptr) != (poses_est_f64 != nullptr), "bop_errors: exactly one of poses_est / poses_est_f64");
  DIM_REQUIRE(points && table_off && sym && sym_off && class_index && pose_gt && K9_f64 && workspace && errors, "bop_errors: null pointer");
  DIM_REQUIRE(((uintptr_t)workspace % 8) == 0, "bop_errors: workspace must be 8-byte aligned");
  CamK K;
  for (int k = 0; k < 9; ++k) K.k[k] = K9_f64[k];
  double* partial = (double*)workspace;
  const dim3 grid(kBopBlocks, B, T), fin(B, T);
  hipStream_t st = as_stream(stream);
  if (poses_est)
    hipLaunchKernelGGL(bop_err_kernel<float>, grid, dim3(kBopThreads), 0, st, points, table_off, sym, sym_off, n_classes, class_index,
                       poses_est, pose_gt, K, K_per_sample_f64, B, max_sym, partial);
  else
    hipLaunchKernelGGL(bop_err_kernel<double>, grid, dim3(kBopThreads), 0, st, points, table_off, sym, sym_off, n_classes, class_index,
                       poses_est_f64, pose_gt, K, K_per_sample_f64, B, max_sym, partial);
  hipLaunchKernelGGL(bop_err_finish, fin, dim3(kBopThreads), 0, st, table_off, sym_off, n_classes, class_index, B, max_sym,
                     (const double*)partial, errors, best_sym, status);
  return check_launch("bop_errors");
}
