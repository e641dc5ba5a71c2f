// Multi-hypothesis refinement: several starting poses per pair, refined side by side in one batch, scored against the observed
// image after the loop and reduced to one pose per pair.  Restated in float64 numpy by tests/hyp_reference.py.
//
// Samples are pair-major: sample b = p * N + h.
//   hyp_expand_kernel      pose_out[p*N+h] = [R_h R_p | t_p]; h = 0 is a bit-exact copy of the pair's pose
//   hyp_broadcast_kernel   the rows of pair p (a plane, a K, a class index) into its N sample rows, float4 where aligned
//   pose_score_kernel      grid (kScoreBlocks, B) over the render's bbox: float64 per-lane sums of the ZNCC terms and the depth
//                          counts, float64 across lanes and waves in a fixed order, one partial per workgroup (no atomics).  The
//                          observed planes are the sample's own row, or the row an index names (dim_pose_score_indexed: the
//                          candidates of csrc/coarse.hip share the one observed frame of their pair)
//   pose_score_finish      one lane per sample: the kScoreBlocks partials in order, the score in float64, the status bit
//   hyp_select_kernel      one lane per pair: argmax of the finite scores (ties: smaller h), then the gathers
// Nothing allocates or synchronises: every entry is graph-capturable.
#include "block_sum.h"
#include "common.h"

namespace dim {

constexpr int kScoreBlocks = 16;   // workgroups per sample (16 x 256 = 4096 lanes over the bbox)
constexpr int kScoreThreads = 256;
constexpr int kScoreTerms = 12;    // n, sa, sr, saa, srr, sar, depth counted, depth hits, min a, max a, min r, max r
constexpr int kScoreSlot = 16;     // doubles per partial (padded)
constexpr int kScoreMinPixels = 64;

__global__ __launch_bounds__(256) void hyp_expand_kernel(const float* __restrict__ rot_table, const float* __restrict__ pose_in, int P,
                                                         int N, float* __restrict__ pose_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * N) return;
  const int p = i / N, h = i - p * N;
  const float* src = pose_in + 12L * p;
  float* dst = pose_out + 12L * i;
  if (h == 0) {
    for (int k = 0; k < 12; ++k) dst[k] = src[k];
    return;
  }
  const float* R = rot_table + 9L * h;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      dst[4 * r + c] = (float)((double)R[3 * r] * (double)src[c] + (double)R[3 * r + 1] * (double)src[4 + c] +
                               (double)R[3 * r + 2] * (double)src[8 + c]);
    dst[4 * r + 3] = src[4 * r + 3];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void hyp_broadcast_kernel(float* __restrict__ dst, const float* __restrict__ src, int P, int N,
                                                            long row_words) {
  const long per_row = VEC ? row_words / 4 : row_words;
  const long total = (long)P * per_row;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long p = i / per_row, k = i - p * per_row;
    if (VEC) {
      const float4 v = reinterpret_cast<const float4*>(src + p * row_words)[k];
      for (int h = 0; h < N; ++h) reinterpret_cast<float4*>(dst + (p * N + h) * row_words)[k] = v;
    } else {
      const float v = src[p * row_words + k];
      for (int h = 0; h < N; ++h) dst[(p * N + h) * row_words + k] = v;
    }
  }
}

struct ScoreAcc {
  double s[6];   // n, sa, sr, saa, srr, sar (shifted values)
  double cnt, hit;
  double amin, amax, rmin, rmax;
};

__device__ __forceinline__ void score_pixel(ScoreAcc& a, float o0, float o1, float o2, float r0, float r1, float r2, float dr, float dob,
                                            double ref_a, double ref_r, int mode, float tau) {
  if (!(dr > 0.f)) return;   // S: drawn pixels of the render (NaN fails)
  if (mode == DIM_HYP_SCORE_RGB) {
    const double va = (double)o0 + (double)o1 + (double)o2, vr = (double)r0 + (double)r1 + (double)r2;
    const double x = va - ref_a, y = vr - ref_r;
    a.s[0] += 1.0;
    a.s[1] += x;
    a.s[2] += y;
    a.s[3] += x * x;
    a.s[4] += y * y;
    a.s[5] += x * y;
    a.amin = fmin(a.amin, va); a.amax = fmax(a.amax, va);
    a.rmin = fmin(a.rmin, vr); a.rmax = fmax(a.rmax, vr);
  } else {
    if (!(dob > 0.f)) return;
    a.cnt += 1.0;
    if (fabsf(dr - dob) < tau) a.hit += 1.0;
  }
}

// VEC: W % 4 == 0 and every plane 16-byte aligned -> the bbox columns are covered by aligned float4 groups, masked at both ends
template <bool VEC>
__global__ __launch_bounds__(kScoreThreads) void pose_score_kernel(const float* __restrict__ img_o, const float* __restrict__ img_r,
                                                                   const float* __restrict__ dep_o, const float* __restrict__ dep_r,
                                                                   const int* __restrict__ bbox, const int* __restrict__ obs_row,
                                                                   int n_obs, int H, int W, int mode, float tau,
                                                                   double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long plane = (long)H * W;
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (bbox) {
    x0 = max(bbox[4 * b + 0], 0); x1 = min(bbox[4 * b + 1], W - 1);
    y0 = max(bbox[4 * b + 2], 0); y1 = min(bbox[4 * b + 3], H - 1);
  }
  // the observed row of the sample: its own, or obs_row[b] of n_obs (an index outside them: nothing is read and nothing counted)
  long ob = b;
  bool empty = x1 < x0 || y1 < y0;
  if (obs_row) {
    ob = obs_row[b];
    if (ob < 0 || ob >= n_obs) {
      ob = 0;
      empty = true;
    }
  }
  const float* o = img_o + ob * 3 * plane;
  const float* r = img_r + (long)b * 3 * plane;
  const float* dr = dep_r + (long)b * plane;
  const float* dob = dep_o ? dep_o + ob * plane : nullptr;
  // a per-sample shift (the bbox's first pixel) keeps a large common offset from cancelling in the second moments
  double ref_a = 0.0, ref_r = 0.0;
  if (!empty && mode == DIM_HYP_SCORE_RGB) {
    const long q = (long)y0 * W + x0;
    ref_a = (double)o[q] + (double)o[plane + q] + (double)o[2 * plane + q];
    ref_r = (double)r[q] + (double)r[plane + q] + (double)r[2 * plane + q];
    if (!isfinite(ref_a)) ref_a = 0.0;
    if (!isfinite(ref_r)) ref_r = 0.0;
  }
  ScoreAcc a;
#pragma unroll
  for (int k = 0; k < 6; ++k) a.s[k] = 0.0;
  a.cnt = a.hit = 0.0;
  a.amin = a.rmin = INFINITY;
  a.amax = a.rmax = -INFINITY;
  if (!empty) {
    if (VEC) {
      const int xa = x0 & ~3, nq = (x1 - xa) / 4 + 1;
      const int n = nq * (y1 - y0 + 1);
      for (int i = blockIdx.x * kScoreThreads + tid; i < n; i += kScoreBlocks * kScoreThreads) {
        const int yy = i / nq, xq = xa + 4 * (i - yy * nq);
        const long q = (long)(y0 + yy) * W + xq;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool rgb = mode == DIM_HYP_SCORE_RGB;   // the depth score reads no colour
        const float4 a0 = rgb ? *reinterpret_cast<const float4*>(o + q) : z4, a1 = rgb ? *reinterpret_cast<const float4*>(o + plane + q) : z4,
                     a2 = rgb ? *reinterpret_cast<const float4*>(o + 2 * plane + q) : z4;
        const float4 r0 = rgb ? *reinterpret_cast<const float4*>(r + q) : z4, r1 = rgb ? *reinterpret_cast<const float4*>(r + plane + q) : z4,
                     r2 = rgb ? *reinterpret_cast<const float4*>(r + 2 * plane + q) : z4;
        float4 d = *reinterpret_cast<const float4*>(dr + q);
        const float4 e = dob ? *reinterpret_cast<const float4*>(dob + q) : z4;
        if (xq < x0) { d.x = 0.f; if (xq + 1 < x0) { d.y = 0.f; if (xq + 2 < x0) d.z = 0.f; } }
        if (xq + 3 > x1) { d.w = 0.f; if (xq + 2 > x1) { d.z = 0.f; if (xq + 1 > x1) d.y = 0.f; } }
        score_pixel(a, a0.x, a1.x, a2.x, r0.x, r1.x, r2.x, d.x, e.x, ref_a, ref_r, mode, tau);
        score_pixel(a, a0.y, a1.y, a2.y, r0.y, r1.y, r2.y, d.y, e.y, ref_a, ref_r, mode, tau);
        score_pixel(a, a0.z, a1.z, a2.z, r0.z, r1.z, r2.z, d.z, e.z, ref_a, ref_r, mode, tau);
        score_pixel(a, a0.w, a1.w, a2.w, r0.w, r1.w, r2.w, d.w, e.w, ref_a, ref_r, mode, tau);
      }
    } else {
      const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
      for (int i = blockIdx.x * kScoreThreads + tid; i < n; i += kScoreBlocks * kScoreThreads) {
        const int yy = i / bw;
        const long q = (long)(y0 + yy) * W + x0 + (i - yy * bw);
        if (mode == DIM_HYP_SCORE_RGB)
          score_pixel(a, o[q], o[plane + q], o[2 * plane + q], r[q], r[plane + q], r[2 * plane + q], dr[q], 0.f, ref_a, ref_r, mode, tau);
        else
          score_pixel(a, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, dr[q], dob[q], 0.0, 0.0, mode, tau);
      }
    }
  }
  // lanes: xor butterfly (the same order on every run); waves: in wave order through LDS
  // (only the terms of the mode: the other ones are their identities in every lane)
  double t[kScoreTerms];
  if (mode == DIM_HYP_SCORE_RGB) {
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = wave_sum(a.s[k]);
    t[6] = t[7] = 0.0;
    t[8] = wave_min(a.amin);
    t[9] = wave_max(a.amax);
    t[10] = wave_min(a.rmin);
    t[11] = wave_max(a.rmax);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = 0.0;
    t[6] = wave_sum(a.cnt);
    t[7] = wave_sum(a.hit);
    t[8] = t[10] = INFINITY;
    t[9] = t[11] = -INFINITY;
  }
  __shared__ double red[kScoreThreads / kWave][kScoreTerms];
  const int wave = tid / kWave, lane = tid % kWave;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kScoreTerms; ++k) red[wave][k] = t[k];
  }
  __syncthreads();
  if (tid < kScoreTerms) {
    double v = red[0][tid];
    for (int w = 1; w < kScoreThreads / kWave; ++w) {
      const double u = red[w][tid];
      v = tid == 8 || tid == 10 ? fmin(v, u) : tid == 9 || tid == 11 ? fmax(v, u) : v + u;
    }
    partial[((long)b * kScoreBlocks + blockIdx.x) * kScoreSlot + tid] = v;
  }
}

__global__ __launch_bounds__(64) void pose_score_finish(const double* __restrict__ partial, int B, int mode, float* __restrict__ score,
                                                        int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s[kScoreTerms];
  for (int k = 0; k < kScoreTerms; ++k) s[k] = partial[(long)b * kScoreBlocks * kScoreSlot + k];
  for (int j = 1; j < kScoreBlocks; ++j) {
    const double* q = partial + ((long)b * kScoreBlocks + j) * kScoreSlot;
    for (int k = 0; k < 8; ++k) s[k] += q[k];
    s[8] = fmin(s[8], q[8]);
    s[9] = fmax(s[9], q[9]);
    s[10] = fmin(s[10], q[10]);
    s[11] = fmax(s[11], q[11]);
  }
  double v = -INFINITY;
  if (mode == DIM_HYP_SCORE_RGB) {
    const double n = s[0];
    if (n >= (double)kScoreMinPixels && s[9] > s[8] && s[11] > s[10]) {   // both planes vary over S
      const double ma = s[1] / n, mr = s[2] / n;
      const double va = s[3] - n * ma * ma, vr = s[4] - n * mr * mr, c = s[5] - n * ma * mr;
      if (va > 0.0 && vr > 0.0) v = fmin(fmax(c / sqrt(va * vr), -1.0), 1.0);
    }
  } else if (s[6] >= (double)kScoreMinPixels) {
    v = s[7] / s[6];
  }
  if (!isfinite(v)) v = -INFINITY;   // a NaN pixel in S
  score[b] = (float)v;
  if (v == -INFINITY && status) status[b] |= DIM_STATUS_HYP_NO_SCORE;
}

__global__ __launch_bounds__(64) void hyp_select_kernel(const float* __restrict__ score, int P, int N, int T, const float* __restrict__ poses_iter,
                                                        const int* __restrict__ status_iter, const int* __restrict__ status_load,
                                                        const float* __restrict__ pose_icp,
                                                        int* __restrict__ choice, float* __restrict__ poses_sel, int* __restrict__ status_sel,
                                                        float* __restrict__ pose_icp_sel) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int best = -1;
  float bv = 0.f;
  for (int h = 0; h < N; ++h) {
    const float v = score[(long)p * N + h];
    if (isfinite(v) && (best < 0 || v > bv)) {
      best = h;
      bv = v;
    }
  }
  const bool none = best < 0;
  if (none) best = 0;
  const long B = (long)P * N, src = (long)p * N + best;
  choice[p] = best;
  for (int t = 0; t < T; ++t) {
    const float* ps = poses_iter + (t * B + src) * 12;
    float* pd = poses_sel + ((long)t * P + p) * 12;
    for (int k = 0; k < 12; ++k) pd[k] = ps[k];
    if (status_iter && status_sel) {
      int st = status_iter[t * B + src];
      if (t == T - 1) {
        if (none) st |= DIM_STATUS_HYP_NO_SCORE;
        if (status_load) st |= status_load[src];
      }
      status_sel[(long)t * P + p] = st;
    }
  }
  if (pose_icp && pose_icp_sel)
    for (int k = 0; k < 12; ++k) pose_icp_sel[12L * p + k] = pose_icp[12 * src + k];
}

}  // namespace dim

using namespace dim;

extern "C" int dim_hyp_expand(const float* rot_table, const float* pose_in, int P, int N, float* pose_out, void* stream) {
  DIM_REQUIRE(P > 0 && N > 0, "hyp_expand: P = %d, N = %d", P, N);
  DIM_REQUIRE(rot_table && pose_in && pose_out, "hyp_expand: null pointer");
  hipLaunchKernelGGL(hyp_expand_kernel, dim3(ceil_div((long)P * N, 256)), dim3(256), 0, as_stream(stream), rot_table, pose_in, P, N,
                     pose_out);
  return check_launch("hyp_expand");
}

extern "C" int dim_hyp_broadcast(void* dst, const void* src, int P, int N, long row_words, void* stream) {
  DIM_REQUIRE(P > 0 && N > 0 && row_words > 0, "hyp_broadcast: P = %d, N = %d, row_words = %ld", P, N, row_words);
  DIM_REQUIRE(dst && src, "hyp_broadcast: null pointer");
  const bool vec = row_words % 4 == 0 && ((uintptr_t)dst % 16) == 0 && ((uintptr_t)src % 16) == 0;
  const long items = (long)P * (vec ? row_words / 4 : row_words);
  const int grid = (int)std::min<long>(ceil_div(items, 256), 4096);
  if (vec)
    hipLaunchKernelGGL(hyp_broadcast_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), (float*)dst, (const float*)src, P, N,
                       row_words);
  else
    hipLaunchKernelGGL(hyp_broadcast_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), (float*)dst, (const float*)src, P, N,
                       row_words);
  return check_launch("hyp_broadcast");
}

extern "C" long dim_pose_score_workspace_bytes(int B, int H, int W) {
  (void)H;
  (void)W;
  if (B <= 0) return 0;
  return (long)B * kScoreBlocks * kScoreSlot * (long)sizeof(double);
}

// dim_pose_score (obs_row NULL: sample b reads observed row b) and dim_pose_score_indexed (row obs_row[b] of n_obs)
static int launch_pose_score(const char* who, const float* image_observed, const float* image_rendered, const float* depth_observed,
                             const float* depth_rendered, const int* bbox, const int* obs_row, int n_obs, int B, int H, int W, int mode,
                             float tau, void* workspace, float* score, int* status, void* stream) {
  DIM_REQUIRE(B > 0 && H > 0 && W > 0, "%s: B = %d, H = %d, W = %d", who, B, H, W);
  DIM_REQUIRE(mode == DIM_HYP_SCORE_RGB || mode == DIM_HYP_SCORE_DEPTH, "%s: mode = %d", who, mode);
  DIM_REQUIRE(image_observed && image_rendered && depth_rendered && workspace && score, "%s: null pointer", who);
  DIM_REQUIRE(mode != DIM_HYP_SCORE_DEPTH || depth_observed, "%s: the depth score needs depth_observed", who);
  DIM_REQUIRE(mode != DIM_HYP_SCORE_DEPTH || tau > 0.f, "%s: tau must be > 0", who);
  const float* dob = mode == DIM_HYP_SCORE_DEPTH ? depth_observed : nullptr;
  auto al = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
  const bool vec = W % 4 == 0 && al(image_observed) && al(image_rendered) && al(depth_rendered) && (!dob || al(dob));
  double* partial = (double*)workspace;
  if (vec)
    hipLaunchKernelGGL(pose_score_kernel<true>, dim3(kScoreBlocks, B), dim3(kScoreThreads), 0, as_stream(stream), image_observed,
                       image_rendered, dob, depth_rendered, bbox, obs_row, n_obs, H, W, mode, tau, partial);
  else
    hipLaunchKernelGGL(pose_score_kernel<false>, dim3(kScoreBlocks, B), dim3(kScoreThreads), 0, as_stream(stream), image_observed,
                       image_rendered, dob, depth_rendered, bbox, obs_row, n_obs, H, W, mode, tau, partial);
  hipLaunchKernelGGL(pose_score_finish, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), (const double*)partial, B, mode, score,
                     status);
  return check_launch(who);
}

extern "C" int dim_pose_score(const float* image_observed, const float* image_rendered, const float* depth_observed,
                              const float* depth_rendered, const int* bbox, int B, int H, int W, int mode, float tau, void* workspace,
                              float* score, int* status, void* stream) {
  return launch_pose_score("pose_score", image_observed, image_rendered, depth_observed, depth_rendered, bbox, nullptr, 0, B, H, W, mode,
                           tau, workspace, score, status, stream);
}

extern "C" int dim_pose_score_indexed(const float* image_observed, const float* image_rendered, const float* depth_observed,
                                      const float* depth_rendered, const int* bbox, const int* obs_row, int n_obs, int B, int H, int W,
                                      int mode, float tau, void* workspace, float* score, int* status, void* stream) {
  DIM_REQUIRE(obs_row, "pose_score_indexed: null pointer (obs_row)");
  DIM_REQUIRE(n_obs > 0, "pose_score_indexed: n_obs = %d", n_obs);
  return launch_pose_score("pose_score_indexed", image_observed, image_rendered, depth_observed, depth_rendered, bbox, obs_row, n_obs, B, H,
                           W, mode, tau, workspace, score, status, stream);
}

extern "C" int dim_hyp_select(const float* score, int P, int N, int T, const float* poses_iter, const int* status_iter, const int* status_load,
                              const float* pose_icp, int* choice, float* poses_sel, int* status_sel, float* pose_icp_sel, void* stream) {
  DIM_REQUIRE(P > 0 && N > 0 && T > 0, "hyp_select: P = %d, N = %d, T = %d", P, N, T);
  DIM_REQUIRE(score && poses_iter && choice && poses_sel, "hyp_select: null pointer");
  hipLaunchKernelGGL(hyp_select_kernel, dim3(ceil_div(P, 64)), dim3(64), 0, as_stream(stream), score, P, N, T, poses_iter, status_iter,
                     status_load, pose_icp, choice, poses_sel, status_sel, pose_icp_sel);
  return check_launch("hyp_select");
}
