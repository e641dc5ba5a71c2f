// Coarse pose from a 2-D detection box: M candidate rotations per pair, each with the translation at which the projected model
// fills the pair's box, and the k best-scoring candidates of every pair.  Restated in float64 numpy by tests/coarse_reference.py.
//
// Samples are pair-major: sample b = p * M + m.
//   pose_from_box_kernel   grid (M, P), 256 lanes, one workgroup per candidate.  Per iteration every model point is projected under
//                          [R_m | t]; the extents of the projection against the box give one scale s and the shift of the centre:
//                            s = ((umax - umin) / bw + (vmax - vmin) / bh) / 2,  tz' = tz s,
//                            tx' = tx s + (cu - (umin + umax) / 2) tz' / fx,     ty' likewise.
//                          R_m x does not change between the iterations: it is kept in LDS (three float64 planes) when the class has at
//                          most kCoarseLdsPoints points and recomputed from the table otherwise.  Extents: per lane, xor butterfly,
//                          then the four waves through LDS; min / max do not depend on the order, so the result is numpy's bit for bit.
//                          Every lane computes the same update.
//   hyp_topk_kernel        one workgroup per pair: k rounds, each the largest (score, -m) key below the previous round's (a 64-bit
//                          key: the order-preserving image of the float32 score above the complement of m), so ties go to the
//                          smaller m and nothing is marked or removed.  No atomics: a replay is bit-identical.
// The third entry of the stage, dim_pose_score_indexed, shares the kernels of dim_pose_score and lives next to them in hyp.hip.
// Nothing allocates or synchronises: every entry is graph-capturable.
#include "block_sum.h"
#include "common.h"
#include "pose_geom.h"

namespace dim {

constexpr int kCoarseThreads = 256;
constexpr int kCoarseWaves = kCoarseThreads / kWave;
constexpr int kCoarseLdsPoints = 2048;   // 3 x 2048 float64 = 48 KB: LINEMOD's evaluation clouds and the usual meshes stay below it
constexpr int kTopkMax = 64;

__global__ __launch_bounds__(kCoarseThreads) void pose_from_box_kernel(const double* __restrict__ points, const int* __restrict__ table_off,
                                                                       int n_classes, const int* __restrict__ class_index,
                                                                       const float* __restrict__ rot_table, const float* __restrict__ boxes,
                                                                       CamK K_uniform, const double* __restrict__ K_per_sample, int M,
                                                                       int iters, double z_init, float* __restrict__ pose_out,
                                                                       double* __restrict__ pose_out_f64, int* __restrict__ status) {
  __shared__ double rot[3][kCoarseLdsPoints];
  __shared__ double red[kCoarseWaves][5];
  const int m = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const long b = (long)p * M + m;
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (double)rot_table[9L * m + k];
  const CamK K = cam_k_pick(K_uniform, K_per_sample, p);
  const double fx = K.k[0], fy = K.k[4], cx = K.k[2], cy = K.k[5];
  const double x0 = (double)boxes[4 * p], x1 = (double)boxes[4 * p + 1], y0 = (double)boxes[4 * p + 2], y1 = (double)boxes[4 * p + 3];
  int off, n, bits = 0;
  if (!class_points(table_off, n_classes, class_index[p], off, n)) bits |= DIM_STATUS_BAD_CLASS;
  const bool box_ok = isfinite(x0) && isfinite(x1) && isfinite(y0) && isfinite(y1) && x1 > x0 && y1 > y0;
  if (!box_ok || (!bits && (off < 0 || n <= 0))) bits |= DIM_STATUS_COARSE_BAD_BOX;
  const double bw = x1 - x0, bh = y1 - y0, cu = 0.5 * (x0 + x1), cv = 0.5 * (y0 + y1);
  double tx = (cu - cx) * z_init / fx, ty = (cv - cy) * z_init / fy, tz = z_init;
  if (!bits) {   // workgroup-uniform from here on: the barriers are reached by every lane or by none
    const double* pts = points + 3L * off;
    const bool in_lds = n <= kCoarseLdsPoints;
    if (in_lds) {
      for (int i = tid; i < n; i += kCoarseThreads) {
        const double x = pts[3L * i], y = pts[3L * i + 1], z = pts[3L * i + 2];
        rot[0][i] = (R[0] * x + R[1] * y) + R[2] * z;
        rot[1][i] = (R[3] * x + R[4] * y) + R[5] * z;
        rot[2][i] = (R[6] * x + R[7] * y) + R[8] * z;
      }
      __syncthreads();
    }
    for (int it = 0; it < iters; ++it) {
      double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, behind = 0.0;
      for (int i = tid; i < n; i += kCoarseThreads) {
        double rx, ry, rz;
        if (in_lds) {
          rx = rot[0][i]; ry = rot[1][i]; rz = rot[2][i];
        } else {
          const double x = pts[3L * i], y = pts[3L * i + 1], z = pts[3L * i + 2];
          rx = (R[0] * x + R[1] * y) + R[2] * z;
          ry = (R[3] * x + R[4] * y) + R[5] * z;
          rz = (R[6] * x + R[7] * y) + R[8] * z;
        }
        const double X = rx + tx, Y = ry + ty, Z = rz + tz;   // pose_geom.h's transform: the rotated point, then + t
        const double c = (K.k[6] * X + K.k[7] * Y) + K.k[8] * Z;
        if (!(c > 0.0)) behind = 1.0;
        double u, v;
        project(K, X, Y, Z, u, v);
        umin = fmin(umin, u); umax = fmax(umax, u);
        vmin = fmin(vmin, v); vmax = fmax(vmax, v);
      }
      umin = wave_min(umin); umax = wave_max(umax);
      vmin = wave_min(vmin); vmax = wave_max(vmax);
      behind = wave_max(behind);
      if (tid % kWave == 0) {
        double* r = red[tid / kWave];
        r[0] = umin; r[1] = umax; r[2] = vmin; r[3] = vmax; r[4] = behind;
      }
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kCoarseWaves; ++w) {
        umin = fmin(umin, red[w][0]); umax = fmax(umax, red[w][1]);
        vmin = fmin(vmin, red[w][2]); vmax = fmax(vmax, red[w][3]);
        behind = fmax(behind, red[w][4]);
      }
      __syncthreads();   // red is read before the next iteration writes it
      const double s = 0.5 * ((umax - umin) / bw + (vmax - vmin) / bh);
      if (behind != 0.0 || !isfinite(s)) {
        bits |= DIM_STATUS_COARSE_BAD_BOX;
        break;   // the same in every lane
      }
      const double tzn = tz * s;
      tx = tx * s + (cu - 0.5 * (umin + umax)) * tzn / fx;
      ty = ty * s + (cv - 0.5 * (vmin + vmax)) * tzn / fy;
      tz = tzn;
    }
  }
  if (tid == 0) {
    if (bits) {
      tx = ty = 0.0;
      tz = z_init;
      status[b] |= bits;
    }
    const double t[3] = {tx, ty, tz};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        pose_out[12 * b + 4 * r + c] = rot_table[9L * m + 3 * r + c];
        if (pose_out_f64) pose_out_f64[12 * b + 4 * r + c] = R[3 * r + c];
      }
      pose_out[12 * b + 4 * r + 3] = (float)t[r];
      if (pose_out_f64) pose_out_f64[12 * b + 4 * r + 3] = t[r];
    }
  }
}

// (score, m) -> a key whose unsigned order is: larger score first, then smaller m; 0 = not a candidate (no finite score maps to it:
// the low word of a candidate is >= 0xFFFF0000)
__device__ __forceinline__ unsigned long long topk_key(float s, int m) {
  s += 0.0f;   // -0 -> +0: the two compare equal, so they tie
  const unsigned u = __float_as_uint(s);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)m);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(kCoarseThreads) void hyp_topk_kernel(const float* __restrict__ score, const int* __restrict__ status_in,
                                                                  int reject_mask, int M, int k, const float* __restrict__ poses_in,
                                                                  int* __restrict__ idx_out, float* __restrict__ score_out,
                                                                  float* __restrict__ poses_out, int* __restrict__ status_out) {
  __shared__ unsigned long long red[kCoarseWaves];
  __shared__ int sel[kTopkMax];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* sc = score + (long)p * M;
  const int* st = status_in ? status_in + (long)p * M : nullptr;
  unsigned long long prev = ~0ull;
  int found = 0;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;
    for (int m = tid; m < M; m += kCoarseThreads) {
      const float s = sc[m];
      if (!isfinite(s) || (st && (st[m] & reject_mask))) continue;
      const unsigned long long key = topk_key(s, m);
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (tid % kWave == 0) red[tid / kWave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kCoarseWaves; ++w) best = red[w] > best ? red[w] : best;
    __syncthreads();   // red is read before the next round writes it
    if (best == 0ull) break;   // the same in every lane: the pair has no further candidate
    if (tid == 0) sel[j] = (int)(0xFFFFFFFFu - (unsigned)best);
    prev = best;
    ++found;
  }
  __syncthreads();
  for (int i = tid; i < k * 12; i += kCoarseThreads) {
    const int j = i / 12, e = i - 12 * j;
    const int m = found ? sel[j < found ? j : 0] : 0;
    const long src = (long)p * M + m, dst = (long)p * k + j;
    poses_out[12 * dst + e] = poses_in[12 * src + e];
    if (e == 0) {
      idx_out[dst] = m;
      score_out[dst] = sc[m];
      status_out[dst] = (st ? st[m] : 0) | (j < found ? 0 : DIM_STATUS_HYP_NO_SCORE);
    }
  }
}

}  // namespace dim

using namespace dim;

extern "C" int dim_pose_from_box(const double* points, const int* table_off, int n_classes, const int* class_index, const float* rot_table,
                                 const float* boxes, const double* K9_f64, const double* K_per_sample, int P, int M, int iters,
                                 double z_init, float* pose_out, double* pose_out_f64, int* status, void* stream) {
  DIM_REQUIRE(P >= 1 && P <= 65535 && M >= 1 && M <= 65535, "pose_from_box: P = %d, M = %d (each 1 .. 65535)", P, M);
  DIM_REQUIRE(iters >= 1, "pose_from_box: iters = %d", iters);
  DIM_REQUIRE(std::isfinite(z_init) && z_init > 0.0, "pose_from_box: z_init = %g must be finite and > 0", z_init);
  DIM_REQUIRE(n_classes > 0, "pose_from_box: n_classes = %d", n_classes);
  DIM_REQUIRE(points && table_off && class_index && rot_table && boxes && K9_f64 && pose_out && status, "pose_from_box: null pointer");
  CamK K;
  for (int k = 0; k < 9; ++k) K.k[k] = K9_f64[k];
  hipLaunchKernelGGL(pose_from_box_kernel, dim3(M, P), dim3(kCoarseThreads), 0, as_stream(stream), points, table_off, n_classes,
                     class_index, rot_table, boxes, K, K_per_sample, M, iters, z_init, pose_out, pose_out_f64, status);
  return check_launch("pose_from_box");
}

extern "C" int dim_hyp_topk(const float* score, const int* status_in, int reject_mask, int P, int M, int k, const float* poses_in,
                            int* idx_out, float* score_out, float* poses_out, int* status_out, void* stream) {
  DIM_REQUIRE(P >= 1 && P <= 65535 && M >= 1 && M <= 65535, "hyp_topk: P = %d, M = %d (each 1 .. 65535)", P, M);
  DIM_REQUIRE(k >= 1 && k <= M && k <= kTopkMax, "hyp_topk: k = %d must be in 1 .. min(M, %d)", k, kTopkMax);
  DIM_REQUIRE(score && poses_in && idx_out && score_out && poses_out && status_out, "hyp_topk: null pointer");
  hipLaunchKernelGGL(hyp_topk_kernel, dim3(P), dim3(kCoarseThreads), 0, as_stream(stream), score, status_in, reject_mask, M, k, poses_in,
                     idx_out, score_out, poses_out, status_out);
  return check_launch("hyp_topk");
}
