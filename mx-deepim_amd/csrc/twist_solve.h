// Float64 device helpers shared by the Gauss-Newton pose stages (icp.hip, flow_pnp.hip, photo.hip, sil.hip) and the pose algebra (se3.hip): the 6x6
// Cholesky solve of the normal equations, the Rodrigues rotation of a twist's omega, and rotation matrix -> quaternion; and what
// the Gauss-Newton stages have in common: the workspace layout, the camera and box of a pair, the solve kernel, the pieces of an
// accumulate kernel (pose load, normal-equation terms, partial store) and the host loop over the two launches of an iteration; and the
// joint solve over the calibrated views of one object (gn_solve_views_kernel, gn_iterate_views) with the rigid 3x4 algebra it and
// views.hip share; and the same with the rig's extrinsics refined along (gn_rig_group_kernel, gn_rig_solve_kernel, gn_iterate_rig).
#pragma once
#include "block_sum.h"
#include "common.h"

namespace dim {

// ---- layout of a Gauss-Newton stage: per iteration an accumulate kernel, grid (kGnBlocks, B), writes one partial per workgroup,
// and gn_solve_kernel, one workgroup per pair, adds them in order.  Workspace: [state B x kGnState][partial B x kGnBlocks x kGnSlot]
constexpr int kGnBlocks = 16;      // workgroups per pair: 4096 lanes over the bbox (a LINEMOD object covers 5k-80k pixels)
constexpr int kGnTerms = 29;       // 21 upper-triangle entries of sum J J^T, 6 of sum J r, point count, sum of squared residuals
                                   // (terms 27 and 28 only feed stats and the point test: icp.hip, flow_pnp.hip and sil.hip put the unweighted
                                   // sum of r^2 over the counted points into 28, photo.hip the weighted one, sum of w r^2)
constexpr int kGnSlot = 32;        // doubles per partial (padded)
constexpr int kGnState = 16;       // doubles per pair: R (9), t (3), updated (1), pad
constexpr int kGnMinPoints = 64;   // fewer points: no update, the stage's status bit

inline long gn_workspace_bytes(int B) { return B <= 0 ? 0 : (long)B * (kGnState + kGnBlocks * kGnSlot) * (long)sizeof(double); }

struct PinholeCam {
  float fx, fy, cx, cy;
};

__host__ __device__ inline PinholeCam cam_of_k9(const float* K9) { return PinholeCam{K9[0], K9[4], K9[2], K9[5]}; }

// the pair's camera: row b of K_per_sample (B, 9) when given, else the one K of the call
__device__ __forceinline__ PinholeCam cam_pick(const float* __restrict__ K_per_sample, PinholeCam k9, int b) {
  return K_per_sample ? cam_of_k9(K_per_sample + 9 * b) : k9;
}

__device__ __forceinline__ bool cam_ok(const PinholeCam& c) {
  return c.fx > 0.f && c.fy > 0.f && isfinite(c.fx) && isfinite(c.fy) && isfinite(c.cx) && isfinite(c.cy);
}

// bbox row b = {min_x, max_x, min_y, max_y} clamped to the frame (no bbox: the frame); empty when x1 < x0 or y1 < y0
struct PixelBox {
  int x0, x1, y0, y1;
};
__device__ __forceinline__ PixelBox clamp_bbox(const int* __restrict__ bbox, int b, int H, int W) {
  if (!bbox) return PixelBox{0, W - 1, 0, H - 1};
  return PixelBox{max(bbox[4 * b + 0], 0), min(bbox[4 * b + 1], W - 1), max(bbox[4 * b + 2], 0), min(bbox[4 * b + 3], H - 1)};
}

__device__ inline void twist_rodrigues(const double* w, double* Rw) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double Wx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double a = 1.0, bq = 0.0;
  if (th >= 1e-12) {
    a = sin(th) / th;
    bq = (1.0 - cos(th)) / (th * th);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double w2 = 0.0;
      for (int k = 0; k < 3; ++k) w2 += Wx[3 * i + k] * Wx[3 * k + j];
      Rw[3 * i + j] = (i == j ? 1.0 : 0.0) + a * Wx[3 * i + j] + bq * w2;
    }
}

// -> false when A is not positive definite
__device__ inline bool cholesky_solve6(const double* A, const double* rhs, double* x) {
  double L[36] = {};
  for (int j = 0; j < 6; ++j) {
    double s = A[6 * j + j];
    for (int k = 0; k < j; ++k) s -= L[6 * j + k] * L[6 * j + k];
    if (!(s > 0.0)) return false;
    L[6 * j + j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
      for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / L[6 * j + j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = rhs[i];
    for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
    y[i] = v / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * x[k];
    x[i] = v / L[6 * i + i];
  }
  return true;
}

// rotation matrix -> (w,x,y,z), w >= 0.  The reference takes the dominant eigenvector of the
// Bar-Itzhack matrix (mat2quat, RT_transform.py:446-523); for a rotation matrix that vector is
// the usual quaternion, computed here with Shepperd's branch selection and normalised.
__device__ inline void mat2quat_d(const double M[9], double q[4]) {
  double tr = M[0] + M[4] + M[8];
  double w, x, y, z;
  if (tr > M[0] && tr > M[4] && tr > M[8]) {
    w = 1.0 + tr; x = M[7] - M[5]; y = M[2] - M[6]; z = M[3] - M[1];
  } else if (M[0] > M[4] && M[0] > M[8]) {
    x = 1.0 + M[0] - M[4] - M[8]; w = M[7] - M[5]; y = M[1] + M[3]; z = M[2] + M[6];
  } else if (M[4] > M[8]) {
    y = 1.0 - M[0] + M[4] - M[8]; w = M[2] - M[6]; x = M[1] + M[3]; z = M[5] + M[7];
  } else {
    z = 1.0 - M[0] - M[4] + M[8]; w = M[3] - M[1]; x = M[2] + M[6]; y = M[5] + M[7];
  }
  double n = sqrt(w * w + x * x + y * y + z * z);
  if (w < 0) n = -n;
  q[0] = w / n; q[1] = x / n; q[2] = y / n; q[3] = z / n;
}

// One Gauss-Newton step of pair b = blockIdx.x (64 lanes): sums the kGnBlocks partials in order, solves the damped normal equations
// by Cholesky, T <- [Rodrigues(omega) | v] T, writes stats (B, iters, 2) = (term 27, sqrt(term 28 / term 27)) = (points, rms residual
// as the stage defines term 28) when given, and ORs FAIL_BIT into
// status[b] when the step was skipped (fewer than kGnMinPoints points or a singular system).  After the last iteration
// pose_out = T pose_in and, when se3_q is given, se3_q = [quat(R), t]; a pair that never updated gets pose_in bit for bit and the
// identity.
template <int FAIL_BIT>
__global__ __launch_bounds__(64) void gn_solve_kernel(const double* __restrict__ partial, double* __restrict__ state, int it, int iters,
                                                     const float* __restrict__ pose_in, float* __restrict__ pose_out,
                                                     float* __restrict__ se3_q, float* __restrict__ stats, int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[kGnTerms];
  if (tid < kGnTerms) {
    double v = 0.0;
    for (int k = 0; k < kGnBlocks; ++k) v += partial[((long)b * kGnBlocks + k) * kGnSlot + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double* st = state + (long)b * kGnState;
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
  bool ok = N >= (double)kGnMinPoints;
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
    status[b] |= FAIL_BIT;
  }
  for (int k = 0; k < 9; ++k) st[k] = R[k];
  for (int k = 0; k < 3; ++k) st[9 + k] = t[k];
  st[12] = updated;
  if (it != iters - 1) return;
  const float* T0 = pose_in + 12 * (long)b;
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

// ---- several calibrated views of one object (B = G x V samples, sample b = g V + v; cam_T_rig row b = X_b = [R_b | t_b], p_cam = X_b p_rig)

constexpr int kGnMaxViews = 16;    // views per group: the solve keeps V x kGnTerms sums in LDS

// rigid 3x4 algebra in float64, rows [R | t] as 9 + 3 doubles: (Rc | tc) = (Ra | ta) (Rb | tb)
__device__ inline void rigid_mul(const double* Ra, const double* ta, const double* Rb, const double* tb, double* Rc, double* tc) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rc[3 * i + j] = Ra[3 * i] * Rb[j] + Ra[3 * i + 1] * Rb[3 + j] + Ra[3 * i + 2] * Rb[6 + j];
    tc[i] = Ra[3 * i] * tb[0] + Ra[3 * i + 1] * tb[1] + Ra[3 * i + 2] * tb[2] + ta[i];
  }
}
// X^-1 = [R^T | -R^T t] (exact only for a rigid X: nothing here checks that)
__device__ inline void rigid_inverse(const double* R, const double* t, double* Ri, double* ti) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Ri[3 * i + j] = R[3 * j + i];
    ti[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  }
}
__device__ inline void rigid_load(const float* __restrict__ T, double* R, double* t) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)T[4 * i + j];
    t[i] = (double)T[4 * i + 3];
  }
}
// rounded once
__device__ inline void rigid_store(const double* R, const double* t, float* __restrict__ T) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
    T[4 * i + 3] = (float)t[i];
  }
}

// One joint Gauss-Newton step of group g = blockIdx.x (64 lanes) over its V samples b = g V + v, after the stage's unchanged
// accumulate launch over all B samples.  s_v = the 16 partials of sample b added in block order, as gn_solve_kernel adds them;
// stats (B, iters, 2) rows as gn_solve_kernel writes them.  With Ad_v = [[R_v, 0], [[t_v]x R_v, R_v]] (twists ordered (omega, v)):
// A = sum_v Ad_v^T A_v Ad_v, g = sum_v Ad_v^T g_v, N = sum_v N_v, rr = sum_v rr_v in ascending v, float64, on one lane;
// stats_group (G, iters, 2) = (N, sqrt(rr / N)).  The step is taken when N >= kGnMinPoints (the GROUP's points) and the damped
// system passes cholesky_solve6; it moves the rig-frame correction D_g <- [Rodrigues(omega) | v] D_g (identity at it == 0), kept in
// the group's state row, and every sample's state row -- what its accumulate kernel reads through gn_load_pose -- is rewritten as
// the conjugate X_b D_g X_b^-1, so the samples' corrections are one rig correction by construction.  A skipped step ORs FAIL_BIT
// into the status of all V samples and leaves D_g.  After the last iteration pose_out[b] = state_b pose_in[b] and
// pose_rig_out[g] = D_g pose_rig_in[g]; a group that never stepped gets pose_in and pose_rig_in bit for bit.
// The matrices of the fusion live in LDS (one lane indexes them in loops), the sums are positional: no atomics, no scratch.
template <int FAIL_BIT>
__global__ __launch_bounds__(64) void gn_solve_views_kernel(const double* __restrict__ partial, double* __restrict__ state,
                                                           double* __restrict__ group_state, const float* __restrict__ cam_T_rig, int V,
                                                           int it, int iters, const float* __restrict__ pose_in,
                                                           float* __restrict__ pose_out, const float* __restrict__ pose_rig_in,
                                                           float* __restrict__ pose_rig_out, float* __restrict__ stats,
                                                           float* __restrict__ stats_group, int* __restrict__ status) {
  const int g = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[kGnMaxViews][kGnSlot];
  __shared__ double Av[36], Ad[36], M[36], A[36];
  for (int idx = tid; idx < V * kGnSlot; idx += 64) {
    const int v = idx / kGnSlot, term = idx % kGnSlot;
    if (term < kGnTerms) {
      const long b = (long)g * V + v;
      double sum = 0.0;
      for (int k = 0; k < kGnBlocks; ++k) sum += partial[(b * kGnBlocks + k) * kGnSlot + term];
      s[v][term] = sum;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  double* gs = group_state + (long)g * kGnState;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, updated = 0.0;
  if (it > 0) {
    for (int k = 0; k < 9; ++k) R[k] = gs[k];
    for (int k = 0; k < 3; ++k) t[k] = gs[9 + k];
    updated = gs[12];
  }
  double gsum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, N = 0.0, rr = 0.0;
  for (int k = 0; k < 36; ++k) A[k] = 0.0;
  for (int v = 0; v < V; ++v) {
    const long b = (long)g * V + v;
    const double Nv = s[v][27], rrv = s[v][28];
    if (stats) {
      stats[(b * iters + it) * 2 + 0] = (float)Nv;
      stats[(b * iters + it) * 2 + 1] = Nv > 0.0 ? (float)sqrt(rrv / Nv) : 0.f;
    }
    double Rx[9], tx[3];
    rigid_load(cam_T_rig + 12 * b, Rx, tx);
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int e = a; e < 6; ++e, ++k) Av[6 * a + e] = Av[6 * e + a] = s[v][k];
    const double Tx[9] = {0.0, -tx[2], tx[1], tx[2], 0.0, -tx[0], -tx[1], tx[0], 0.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        Ad[6 * i + j] = Ad[6 * (3 + i) + 3 + j] = Rx[3 * i + j];
        Ad[6 * i + 3 + j] = 0.0;
        Ad[6 * (3 + i) + j] = Tx[3 * i] * Rx[j] + Tx[3 * i + 1] * Rx[3 + j] + Tx[3 * i + 2] * Rx[6 + j];
      }
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        double m = 0.0;
        for (int q = 0; q < 6; ++q) m += Av[6 * i + q] * Ad[6 * q + j];
        M[6 * i + j] = m;
      }
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 6; ++j) {
        double m = 0.0;
        for (int q = 0; q < 6; ++q) m += Ad[6 * q + i] * M[6 * q + j];
        A[6 * i + j] += m;
      }
      double m = 0.0;
      for (int q = 0; q < 6; ++q) m += Ad[6 * q + i] * s[v][21 + q];
      gsum[i] += m;
    }
    N += Nv;
    rr += rrv;
  }
  if (stats_group) {
    stats_group[((long)g * iters + it) * 2 + 0] = (float)N;
    stats_group[((long)g * iters + it) * 2 + 1] = N > 0.0 ? (float)sqrt(rr / N) : 0.f;
  }
  bool ok = N >= (double)kGnMinPoints;
  double xi[6];
  if (ok) {
    const double damp = 1e-9 * (A[0] + A[7] + A[14] + A[21] + A[28] + A[35]) / 6.0;
    double rhs[6];
    for (int a = 0; a < 6; ++a) {
      A[6 * a + a] += damp;
      rhs[a] = -gsum[a];
    }
    ok = cholesky_solve6(A, rhs, xi);
  }
  if (ok) {
    double Rw[9], Rn[9], tn[3];
    twist_rodrigues(xi, Rw);
    rigid_mul(Rw, xi + 3, R, t, Rn, tn);
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
    updated = 1.0;
  }
  for (int k = 0; k < 9; ++k) gs[k] = R[k];
  for (int k = 0; k < 3; ++k) gs[9 + k] = t[k];
  gs[12] = updated;
  const bool last = it == iters - 1;
  for (int v = 0; v < V; ++v) {
    const long b = (long)g * V + v;
    if (!ok && status) status[b] |= FAIL_BIT;
    double Rx[9], tx[3], Ri[9], ti[3], Rm[9], tm[3], Rs[9], ts[3];
    rigid_load(cam_T_rig + 12 * b, Rx, tx);
    rigid_inverse(Rx, tx, Ri, ti);
    rigid_mul(R, t, Ri, ti, Rm, tm);
    rigid_mul(Rx, tx, Rm, tm, Rs, ts);
    double* st = state + b * kGnState;
    for (int k = 0; k < 9; ++k) st[k] = Rs[k];
    for (int k = 0; k < 3; ++k) st[9 + k] = ts[k];
    st[12] = updated;
    if (!last) continue;
    const float* T0 = pose_in + 12 * b;
    float* out = pose_out + 12 * b;
    if (updated == 0.0) {   // never moved: the input pose, bit for bit
      for (int k = 0; k < 12; ++k) out[k] = T0[k];
      continue;
    }
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j)
        out[4 * i + j] = (float)(Rs[3 * i] * (double)T0[j] + Rs[3 * i + 1] * (double)T0[4 + j] + Rs[3 * i + 2] * (double)T0[8 + j]);
      out[4 * i + 3] = (float)(Rs[3 * i] * (double)T0[3] + Rs[3 * i + 1] * (double)T0[7] + Rs[3 * i + 2] * (double)T0[11] + ts[i]);
    }
  }
  if (!last) return;
  const float* T0 = pose_rig_in + 12 * (long)g;
  float* out = pose_rig_out + 12 * (long)g;
  if (updated == 0.0) {
    for (int k = 0; k < 12; ++k) out[k] = T0[k];
    return;
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out[4 * i + j] = (float)(R[3 * i] * (double)T0[j] + R[3 * i + 1] * (double)T0[4 + j] + R[3 * i + 2] * (double)T0[8 + j]);
    out[4 * i + 3] = (float)(R[3 * i] * (double)T0[3] + R[3 * i + 1] * (double)T0[7] + R[3 * i + 2] * (double)T0[11] + t[i]);
  }
}

// ---- the rig's extrinsics refined together with the object poses (tests/rig_reference.py restates the rule, include/deepim_hip.h
// states it).  Unknowns: a correction C_v per camera, X'_v = C_v X_v with C_0 = I for good, and a rig-frame correction D_g per group;
// X_v = cam_T_rig row v of group 0.  Two launches per iteration after the stage's accumulate launch:
//   gn_rig_group_kernel  one workgroup per group: the block-order sums s_gv, W_gv = A_gv Ad(X'_v), H_ee = sum_v Ad_v^T W_gv,
//                        r_e = -sum_v Ad_v^T g_gv, the 6x6 Cholesky of the damped H_ee and through it Y_gv = H_ee^-1 W_gv^T and
//                        z = H_ee^-1 r_e, all into the group's block of the workspace
//   gn_rig_solve_kernel  one workgroup: who takes part, the Schur complement S over the free views as a packed triangle in LDS, its
//                        Cholesky with one lane per row, alpha, eta_g = z_g - sum_v Y_gv alpha_v, the updates and every state row
// Workspace after the joint layout: [rig state V x kGnState = {R, t of C_v, moved, pad}] then per group gn_rig_group_doubles(V) doubles:
// [s V x kGnSlot][W V x 36][Y V x 36][z 6, active, H_ee passed the Cholesky].  Every word that is read was written in the same
// iteration (or, state, in the one before): no initialisation.  Sums are positional and ascending: no atomics.
constexpr int kGnRigLanes = 256;   // of gn_rig_solve_kernel; at most 6 (kGnMaxViews - 1) = 90 rows in S
constexpr int kGnRigRows = 6 * (kGnMaxViews - 1);

__host__ __device__ inline long gn_rig_group_doubles(int V) { return (long)V * (kGnSlot + 72) + 8; }

// index of (a, e), a <= e, among the 21 upper-triangle terms; the symmetric entry (a, e) of A from the 29 sums
__device__ __forceinline__ int gn_tri(int a, int e) { return a * 6 - a * (a - 1) / 2 + (e - a); }
__device__ __forceinline__ double gn_sym(const double* s, int a, int e) { return a <= e ? s[gn_tri(a, e)] : s[gn_tri(e, a)]; }

// X'_v = C_v X_v; a camera that never moved keeps its nominal row exactly
__device__ inline void gn_rig_extrinsic(const float* __restrict__ cam_T_rig, const double* rig_state, int v, bool have_state, double* Rx,
                                        double* tx) {
  double Rn[9], tn[3];
  rigid_load(cam_T_rig + 12 * v, Rn, tn);
  const double* c = rig_state + (long)v * kGnState;
  if (have_state && c[12] != 0.0) {
    double Rc[9], tc[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rc[k] = c[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tc[k] = c[9 + k];
    rigid_mul(Rc, tc, Rn, tn, Rx, tx);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) Rx[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tx[k] = tn[k];
  }
}

// T pose (3x4 float32) in float64, rounded once
__device__ inline void rigid_apply_store(const double* R, const double* t, const float* __restrict__ T0, float* __restrict__ out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      out[4 * i + j] = (float)(R[3 * i] * (double)T0[j] + R[3 * i + 1] * (double)T0[4 + j] + R[3 * i + 2] * (double)T0[8 + j]);
    out[4 * i + 3] = (float)(R[3 * i] * (double)T0[3] + R[3 * i + 1] * (double)T0[7] + R[3 * i + 2] * (double)T0[11] + t[i]);
  }
}

// group g = blockIdx.x.  The operations on H_ee and its solve are those of gn_solve_views_kernel and cholesky_solve6 in their order
// (the pivots recomputed by every lane, the rows and the right-hand sides spread over lanes), so with no free view z is that kernel's xi.
template <int LANES>   // a template so that the header may hold it: the driver launches it with 128
__global__ __launch_bounds__(LANES) void gn_rig_group_kernel(const double* __restrict__ partial, const double* __restrict__ rig_state,
                                                          double* __restrict__ rig_group, const float* __restrict__ cam_T_rig, int V, int it,
                                                          int iters, float* __restrict__ stats, float* __restrict__ stats_group) {
  const int g = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[kGnMaxViews][kGnSlot];
  __shared__ double Ad[kGnMaxViews][36], Wl[kGnMaxViews][36];
  __shared__ double H[36], L[36], gs[8];   // gs: sum_v Ad_v^T g_v (6), N, rr
  double* o_s = rig_group + (long)g * gn_rig_group_doubles(V);
  double* o_W = o_s + V * kGnSlot;
  double* o_Y = o_W + V * 36;
  double* o_tail = o_Y + V * 36;
  for (int idx = tid; idx < V * kGnSlot; idx += LANES) {
    const int v = idx / kGnSlot, term = idx % kGnSlot;
    if (term < kGnTerms) {
      const long b = (long)g * V + v;
      double sum = 0.0;
      for (int k = 0; k < kGnBlocks; ++k) sum += partial[(b * kGnBlocks + k) * kGnSlot + term];
      s[v][term] = sum;
      o_s[idx] = sum;
    }
  }
  if (tid < V) {
    double Rx[9], tx[3];
    gn_rig_extrinsic(cam_T_rig, rig_state, tid, it > 0, Rx, tx);
    const double Tx[9] = {0.0, -tx[2], tx[1], tx[2], 0.0, -tx[0], -tx[1], tx[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Ad[tid][6 * i + j] = Ad[tid][6 * (3 + i) + 3 + j] = Rx[3 * i + j];
        Ad[tid][6 * i + 3 + j] = 0.0;
        Ad[tid][6 * (3 + i) + j] = Tx[3 * i] * Rx[j] + Tx[3 * i + 1] * Rx[3 + j] + Tx[3 * i + 2] * Rx[6 + j];
      }
    }
  }
  __syncthreads();
  if (tid < V && stats) {
    const long b = (long)g * V + tid;
    const double Nv = s[tid][27], rrv = s[tid][28];
    stats[(b * iters + it) * 2 + 0] = (float)Nv;
    stats[(b * iters + it) * 2 + 1] = Nv > 0.0 ? (float)sqrt(rrv / Nv) : 0.f;
  }
  for (int idx = tid; idx < V * 36; idx += LANES) {
    const int v = idx / 36, i = (idx % 36) / 6, j = idx % 6;
    double m = 0.0;
    for (int q = 0; q < 6; ++q) m += gn_sym(s[v], i, q) * Ad[v][6 * q + j];
    Wl[v][6 * i + j] = m;
    o_W[idx] = m;
  }
  __syncthreads();
  if (tid < 36) {
    const int i = tid / 6, j = tid % 6;
    double a = 0.0;
    for (int v = 0; v < V; ++v) {
      double m = 0.0;
      for (int q = 0; q < 6; ++q) m += Ad[v][6 * q + i] * Wl[v][6 * q + j];
      a += m;
    }
    H[tid] = a;
  } else if (tid < 42) {
    const int i = tid - 36;
    double a = 0.0;
    for (int v = 0; v < V; ++v) {
      double m = 0.0;
      for (int q = 0; q < 6; ++q) m += Ad[v][6 * q + i] * s[v][21 + q];
      a += m;
    }
    gs[i] = a;
  } else if (tid == 42) {
    double N = 0.0, rr = 0.0;
    for (int v = 0; v < V; ++v) {
      N += s[v][27];
      rr += s[v][28];
    }
    gs[6] = N;
    gs[7] = rr;
    if (stats_group) {
      stats_group[((long)g * iters + it) * 2 + 0] = (float)N;
      stats_group[((long)g * iters + it) * 2 + 1] = N > 0.0 ? (float)sqrt(rr / N) : 0.f;
    }
  }
  __syncthreads();
  const bool active = gs[6] >= (double)kGnMinPoints;
  bool ok = active;
  if (active) {   // the same for every lane
    const double damp = 1e-9 * (H[0] + H[7] + H[14] + H[21] + H[28] + H[35]) / 6.0;
    for (int j = 0; j < 6; ++j) {
      double sp = H[7 * j] + damp;
      for (int k = 0; k < j; ++k) sp -= L[6 * j + k] * L[6 * j + k];
      if (!(sp > 0.0)) ok = false;   // what follows is never used; the barriers stay
      const double d = sqrt(sp);
      if (tid == j) {
        L[7 * j] = d;
      } else if (tid > j && tid < 6) {
        double v = H[6 * tid + j];
        for (int k = 0; k < j; ++k) v -= L[6 * tid + k] * L[6 * j + k];
        L[6 * tid + j] = v / d;
      }
      __syncthreads();
    }
  }
  if (ok) {
    for (int c = tid; c <= 6 * V; c += LANES) {   // the columns of W_g^T, then r_e
      const int v = c / 6, k = c % 6;
      double rhs[6], y[6], x[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) rhs[i] = c < 6 * V ? Wl[v][6 * k + i] : -gs[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double a = rhs[i];
#pragma unroll
        for (int q = 0; q < i; ++q) a -= L[6 * i + q] * y[q];
        y[i] = a / L[7 * i];
      }
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double a = y[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) a -= L[6 * q + i] * x[q];
        x[i] = a / L[7 * i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (c < 6 * V)
          o_Y[v * 36 + 6 * i + k] = x[i];
        else
          o_tail[i] = x[i];
      }
    }
  }
  if (tid == 0) {
    o_tail[6] = active ? 1.0 : 0.0;
    o_tail[7] = ok ? 1.0 : 0.0;
  }
}

// entry (i, j), i >= j, of the packed lower triangle
__device__ __forceinline__ int gn_packed(int i, int j) { return i * (i + 1) / 2 + j; }

// sum over the active groups, in ascending g, of term(the group's block).  Four groups at a time: their flags and operands are loaded
// before any is added, so a lane waits for memory once per four groups and not twice per group (an inactive group's term is computed
// from whatever its block holds and dropped)
template <class Term>
__device__ __forceinline__ double gn_rig_sum_active(const double* __restrict__ rig_group, long gd, int oT, int G, Term term) {
  double t = 0.0;
  for (int g0 = 0; g0 < G; g0 += 4) {
    double m[4];
    bool on[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double* blk = rig_group + min(g0 + u, G - 1) * gd;
      on[u] = g0 + u < G && blk[oT + 6] != 0.0;
      m[u] = term(blk);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (on[u]) t += m[u];
  }
  return t;
}

template <int FAIL_BIT>
__global__ __launch_bounds__(kGnRigLanes) void gn_rig_solve_kernel(double* __restrict__ state, double* __restrict__ group_state,
                                                                  double* __restrict__ rig_state, const double* __restrict__ rig_group,
                                                                  const float* __restrict__ cam_T_rig, int B, int V, int it, int iters,
                                                                  const float* __restrict__ pose_in, float* __restrict__ pose_out,
                                                                  const float* __restrict__ pose_rig_in, float* __restrict__ pose_rig_out,
                                                                  float* __restrict__ cam_T_rig_out, float* __restrict__ stats_view,
                                                                  int* __restrict__ status) {
  const int tid = threadIdx.x, G = B / V;
  const long gd = gn_rig_group_doubles(V);
  const int oW = V * kGnSlot, oY = oW + V * 36, oT = oY + V * 36;
  __shared__ double S[kGnRigRows * (kGnRigRows + 1) / 2];
  __shared__ double Haa[kGnMaxViews][42];   // H_aa (36) and r_a (6) of the free views, in the order of fl
  __shared__ double rs[kGnRigRows], dg[kGnRigRows];
  __shared__ int fl[kGnMaxViews], slot[kGnMaxViews], n_free;
  const bool last = it == iters - 1;
  // ---- who takes part, from the counts alone
  if (tid < V) {
    double N = 0.0, rr = 0.0, shared = 0.0;
    for (int g = 0; g < G; ++g) {
      const double* blk = rig_group + g * gd;
      const double Ngv = blk[tid * kGnSlot + 27];
      N += Ngv;
      rr += blk[tid * kGnSlot + 28];
      if (blk[oT + 6] != 0.0 && blk[27] >= (double)kGnMinPoints) shared += Ngv;
    }
    if (stats_view) {
      stats_view[((long)tid * iters + it) * 2 + 0] = (float)N;
      stats_view[((long)tid * iters + it) * 2 + 1] = N > 0.0 ? (float)sqrt(rr / N) : 0.f;
    }
    slot[tid] = (tid >= 1 && shared >= (double)kGnMinPoints) ? 0 : -1;
  }
  int bad = 0;   // an active group whose H_ee is not positive definite
  for (int g = tid; g < G; g += kGnRigLanes) bad |= (rig_group[g * gd + oT + 6] != 0.0 && rig_group[g * gd + oT + 7] == 0.0) ? 1 : 0;
  const bool any_bad = __syncthreads_or(bad) != 0;
  if (tid == 0) {
    int F = 0;
    for (int v = 0; v < V; ++v)
      if (slot[v] == 0) {
        slot[v] = F;
        fl[F++] = v;
      }
    n_free = F;
  }
  __syncthreads();
  const int F = n_free, n = 6 * F;
  bool taken = F > 0 && !any_bad;
  if (taken) {
    // ---- H_aa, r_a: sums over the active groups in ascending g
    for (int idx = tid; idx < F * 42; idx += kGnRigLanes) {
      const int v = fl[idx / 42], e = idx % 42;
      const int term = e < 36 ? (e / 6 <= e % 6 ? gn_tri(e / 6, e % 6) : gn_tri(e % 6, e / 6)) : 21 + (e - 36);
      const double a = gn_rig_sum_active(rig_group, gd, oT, G, [&](const double* blk) { return blk[v * kGnSlot + term]; });
      Haa[idx / 42][e] = e < 36 ? a : -a;
    }
    __syncthreads();
    // ---- S = H_aa (damped) - sum_g W_g Y_g, rs = r_a - sum_g W_g z_g
    for (int idx = tid; idx < n * n; idx += kGnRigLanes) {
      const int i = idx / n, j = idx % n;
      if (j > i) continue;
      const int fv = i / 6, a = i % 6, fw = j / 6, c = j % 6;
      const int wo = oW + fl[fv] * 36 + 6 * a, yo = oY + fl[fw] * 36 + c;
      const double t = gn_rig_sum_active(rig_group, gd, oT, G, [&](const double* blk) {
        double m = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) m += blk[wo + q] * blk[yo + 6 * q];
        return m;
      });
      double base = 0.0;
      if (fv == fw) {
        base = Haa[fv][6 * a + c];
        if (a == c) base += 1e-9 * (Haa[fv][0] + Haa[fv][7] + Haa[fv][14] + Haa[fv][21] + Haa[fv][28] + Haa[fv][35]) / 6.0;
      }
      S[gn_packed(i, j)] = base - t;
    }
    if (tid < n) {
      const int fv = tid / 6, a = tid % 6;
      const int wo = oW + fl[fv] * 36 + 6 * a;
      const double t = gn_rig_sum_active(rig_group, gd, oT, G, [&](const double* blk) {
        double m = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) m += blk[wo + q] * blk[oT + q];
        return m;
      });
      rs[tid] = Haa[fv][36 + a] - t;
    }
    __syncthreads();
    // ---- Cholesky in place, column by column: lane i owns row i, every lane recomputes the pivot, one barrier per column
    for (int j = 0; j < n; ++j) {
      double sp = S[gn_packed(j, j)];
      for (int k = 0; k < j; ++k) sp -= S[gn_packed(j, k)] * S[gn_packed(j, k)];
      if (!(sp > 0.0)) taken = false;   // the same for every lane; what follows is never used
      const double d = sqrt(sp);
      if (tid == j) {
        dg[j] = d;
      } else if (tid > j && tid < n) {
        double v = S[gn_packed(tid, j)];
        for (int k = 0; k < j; ++k) v -= S[gn_packed(tid, k)] * S[gn_packed(j, k)];
        S[gn_packed(tid, j)] = v / d;
      }
      __syncthreads();
    }
    // ---- L y = rs, L^T alpha = y: the lane's own entry in a register, the solved ones in rs
    double mine = tid < n ? rs[tid] : 0.0;
    for (int j = 0; j < n; ++j) {
      if (tid == j) rs[j] = mine / dg[j];
      __syncthreads();
      if (tid > j && tid < n) mine -= S[gn_packed(tid, j)] * rs[j];
    }
    __syncthreads();
    mine = tid < n ? rs[tid] : 0.0;
    for (int j = n - 1; j >= 0; --j) {
      if (tid == j) rs[j] = mine / dg[j];
      __syncthreads();
      if (tid < j) mine -= S[gn_packed(j, tid)] * rs[j];
    }
    __syncthreads();
  }
  // ---- the updates: D_g by lane g, C_v by lane v
  for (int g = tid; g < G; g += kGnRigLanes) {
    const double* blk = rig_group + g * gd;
    double* gsr = group_state + (long)g * kGnState;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, updated = 0.0;
    if (it > 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = gsr[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = gsr[9 + k];
      updated = gsr[12];
    }
    const bool steps = blk[oT + 6] != 0.0 && (F > 0 ? taken : blk[oT + 7] != 0.0);
    if (steps) {
      double xi[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double a = blk[oT + i];
        for (int f = 0; f < F; ++f) {
          const double* Yg = blk + oY + fl[f] * 36;
#pragma unroll
          for (int c = 0; c < 6; ++c) a -= Yg[6 * i + c] * rs[6 * f + c];
        }
        xi[i] = a;
      }
      double Rw[9], Rn[9], tn[3];
      twist_rodrigues(xi, Rw);
      rigid_mul(Rw, xi + 3, R, t, Rn, tn);
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = tn[k];
      updated = 1.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) gsr[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) gsr[9 + k] = t[k];
    gsr[12] = updated;
    if (last) {
      const float* T0 = pose_rig_in + 12 * (long)g;
      float* out = pose_rig_out + 12 * (long)g;
      if (updated == 0.0) {   // never stepped: the input, bit for bit
        for (int k = 0; k < 12; ++k) out[k] = T0[k];
      } else {
        rigid_apply_store(R, t, T0, out);
      }
    }
  }
  if (tid < V) {
    double* c = rig_state + (long)tid * kGnState;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, moved = 0.0;
    if (it > 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = c[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = c[9 + k];
      moved = c[12];
    }
    if (taken && slot[tid] >= 0) {
      double xi[6], Rw[9], Rn[9], tn[3];
#pragma unroll
      for (int k = 0; k < 6; ++k) xi[k] = rs[6 * slot[tid] + k];
      twist_rodrigues(xi, Rw);
      rigid_mul(Rw, xi + 3, R, t, Rn, tn);
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = tn[k];
      moved = 1.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[9 + k] = t[k];
    c[12] = moved;
  }
  __syncthreads();   // the rows just written are read below, by other lanes of this workgroup
  // ---- every sample: its bits, its state row X'_v D_g X_v^-1, and after the last iteration its outputs
  for (int b = tid; b < B; b += kGnRigLanes) {
    const int g = b / V, v = b % V;
    const double* blk = rig_group + g * gd;
    const bool active = blk[oT + 6] != 0.0;
    int bits = 0;
    if (!active || (F > 0 ? !taken : blk[oT + 7] == 0.0)) bits |= FAIL_BIT;
    if (v >= 1 && slot[v] < 0) bits |= DIM_STATUS_VIEWS_CALIB_HELD;
    if (status && bits) status[b] |= bits;
    double Rn[9], tn[3], Rx[9], tx[3], Ri[9], ti[3], Rd[9], td[3], Rm[9], tm[3], Rs[9], ts[3];
    rigid_load(cam_T_rig + 12 * v, Rn, tn);
    gn_rig_extrinsic(cam_T_rig, rig_state, v, true, Rx, tx);
    const double* gsr = group_state + (long)g * kGnState;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rd[k] = gsr[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) td[k] = gsr[9 + k];
    const double updated = gsr[12];
    rigid_inverse(Rn, tn, Ri, ti);
    rigid_mul(Rd, td, Ri, ti, Rm, tm);
    rigid_mul(Rx, tx, Rm, tm, Rs, ts);
    double* st = state + (long)b * kGnState;
#pragma unroll
    for (int k = 0; k < 9; ++k) st[k] = Rs[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) st[9 + k] = ts[k];
    st[12] = updated;
    if (!last) continue;
    const float* T0 = pose_in + 12 * (long)b;
    float* out = pose_out + 12 * (long)b;
    if (updated == 0.0) {   // a group that never stepped: the input pose, bit for bit
      for (int k = 0; k < 12; ++k) out[k] = T0[k];
    } else {
      rigid_apply_store(Rs, ts, T0, out);
    }
    float* xo = cam_T_rig_out + 12 * (long)b;
    if (rig_state[(long)v * kGnState + 12] == 0.0) {   // a view that never moved: its nominal row, bit for bit
      for (int k = 0; k < 12; ++k) xo[k] = cam_T_rig[12 * v + k];
    } else {
      rigid_store(Rx, tx, xo);
    }
  }
}

// ---- what the accumulate kernels share.  All of it is inlined: the kGnTerms accumulators of a lane are registers of the kernel.

// the correction T_delta = [R | t] an iteration linearises at: the identity at it == 0, else the state row of pair b as T
template <class T>
__device__ __forceinline__ void gn_load_pose(const double* __restrict__ state, int b, int it, T (&R)[9], T (&t)[3]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = k % 4 == 0 ? (T)1 : (T)0;
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = (T)0;
  if (it > 0) {
    const double* s = state + (long)b * kGnState;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (T)s[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (T)s[9 + k];
  }
}

// one scalar residual r with Jacobian J: terms 0..20 += J J^T (upper triangle), terms 21..26 += J r.  Terms 27 and 28 are the caller's.
template <class T>
__device__ __forceinline__ void gn_add_row(T (&acc)[kGnTerms], const T (&J)[6], T r) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int e = a; e < 6; ++e) acc[k++] += J[a] * J[e];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
}
// the same under the weight w: += (w J[a]) J[e] and (w J[a]) r
template <class T>
__device__ __forceinline__ void gn_add_row(T (&acc)[kGnTerms], const T (&J)[6], T r, T w) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const T wa = w * J[a];
#pragma unroll
    for (int e = a; e < 6; ++e) acc[k++] += wa * J[e];
    acc[21 + a] += wa * r;
  }
}

// one reprojected point m = (mx, my, mz), mz > 0, with pixel residual (rx, ry), e2 = rx^2 + ry^2, under the weight w: both rows of
// d(pixel)/dm = [ax 0 bx; 0 ay by], dm = omega x m + v, into terms 0..26, the point into 27 and e2 (unweighted) into 28
__device__ __forceinline__ void gn_add_pixel(double (&acc)[kGnTerms], double fx, double fy, double mx, double my, double mz, double rx,
                                             double ry, double w, double e2) {
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

// the workgroup's sums (block_sum.h: every lane must call) into its slot of pair b = partial[b][blockIdx.x]
__device__ __forceinline__ void gn_store_partial(const double (&acc)[kGnTerms], double* __restrict__ partial, int b) {
  const double total = block_sum(acc);
  if (threadIdx.x < kGnTerms) partial[((long)b * kGnBlocks + blockIdx.x) * kGnSlot + threadIdx.x] = total;
}
// per-lane float32 sums: float64 from here on, in a fixed order
__device__ __forceinline__ void gn_store_partial(const float (&acc)[kGnTerms], double* __restrict__ partial, int b) {
  double acc64[kGnTerms];
#pragma unroll
  for (int k = 0; k < kGnTerms; ++k) acc64[k] = (double)acc[k];
  gn_store_partial(acc64, partial, b);
}

// ---- host side of a stage's driver
struct GnWorkspace {
  double* state;
  double* partial;
  GnWorkspace(void* workspace, int B) : state((double*)workspace), partial(state + (long)B * kGnState) {}
};

// the two launches of each of `total` iterations: accumulate(it), the stage's own launch into ws.partial, then the solve
template <int FAIL_BIT, class Accumulate>
inline void gn_iterate(const GnWorkspace& ws, int B, int total, const float* pose_in, float* pose_out, float* se3_q, float* stats,
                       int* status, hipStream_t st, Accumulate accumulate) {
  for (int it = 0; it < total; ++it) {
    accumulate(it);
    hipLaunchKernelGGL(gn_solve_kernel<FAIL_BIT>, dim3(B), dim3(64), 0, st, (const double*)ws.partial, ws.state, it, total, pose_in,
                       pose_out, se3_q, stats, status);
  }
}

// the same for groups of V views: `views` names what the joint solve needs besides; the group state rows follow the stage's own
// workspace at group_state (gn_views_state_bytes more bytes)
struct GnViews {
  const float* cam_T_rig;
  int V;
  const float* pose_rig_in;
  float* pose_rig_out;
  float* stats_group;
};

inline long gn_views_state_bytes(int B, int V) { return (B <= 0 || V <= 0) ? 0 : (long)(B / V) * kGnState * (long)sizeof(double); }

inline bool gn_views_ok(const GnViews& vw, int B) {
  return vw.V >= 1 && vw.V <= kGnMaxViews && B % vw.V == 0 && vw.cam_T_rig && vw.pose_rig_in && vw.pose_rig_out;
}

template <int FAIL_BIT, class Accumulate>
inline void gn_iterate_views(const GnWorkspace& ws, double* group_state, int B, const GnViews& vw, int total, const float* pose_in,
                             float* pose_out, float* stats, int* status, hipStream_t st, Accumulate accumulate) {
  for (int it = 0; it < total; ++it) {
    accumulate(it);
    hipLaunchKernelGGL(gn_solve_views_kernel<FAIL_BIT>, dim3(B / vw.V), dim3(64), 0, st, (const double*)ws.partial, ws.state, group_state,
                       vw.cam_T_rig, vw.V, it, total, pose_in, pose_out, vw.pose_rig_in, vw.pose_rig_out, stats, vw.stats_group, status);
  }
}

// one driver for a stage's two entries: views == nullptr is the single-view stage, launch for launch what gn_iterate enqueues
template <int FAIL_BIT, class Accumulate>
inline void gn_iterate_either(const GnWorkspace& ws, double* group_state, int B, const GnViews* views, int total, const float* pose_in,
                              float* pose_out, float* stats, int* status, hipStream_t st, Accumulate accumulate) {
  if (views)
    gn_iterate_views<FAIL_BIT>(ws, group_state, B, *views, total, pose_in, pose_out, stats, status, st, accumulate);
  else
    gn_iterate<FAIL_BIT>(ws, B, total, pose_in, pose_out, nullptr, stats, status, st, accumulate);
}

// the same with the rig's extrinsics refined along (gn_rig_group_kernel, gn_rig_solve_kernel): three launches per iteration.  The rig
// state and the groups' blocks follow the group state rows (gn_rig_state_bytes more bytes)
struct GnRig {
  float* cam_T_rig_out;
  float* stats_view;
};

inline long gn_rig_state_bytes(int B, int V) {
  return (B <= 0 || V <= 0) ? 0 : ((long)V * kGnState + (long)(B / V) * gn_rig_group_doubles(V)) * (long)sizeof(double);
}

template <int FAIL_BIT, class Accumulate>
inline void gn_iterate_rig(const GnWorkspace& ws, double* group_state, int B, const GnViews& vw, const GnRig& rig, int total,
                           const float* pose_in, float* pose_out, float* stats, int* status, hipStream_t st, Accumulate accumulate) {
  const int G = B / vw.V;
  double* rig_state = group_state + (long)G * kGnState;
  double* rig_group = rig_state + (long)vw.V * kGnState;
  for (int it = 0; it < total; ++it) {
    accumulate(it);
    hipLaunchKernelGGL(gn_rig_group_kernel<128>, dim3(G), dim3(128), 0, st, (const double*)ws.partial, (const double*)rig_state, rig_group,
                       vw.cam_T_rig, vw.V, it, total, stats, vw.stats_group);
    hipLaunchKernelGGL(gn_rig_solve_kernel<FAIL_BIT>, dim3(1), dim3(kGnRigLanes), 0, st, ws.state, group_state, rig_state,
                       (const double*)rig_group, vw.cam_T_rig, B, vw.V, it, total, pose_in, pose_out, vw.pose_rig_in, vw.pose_rig_out,
                       rig.cam_T_rig_out, rig.stats_view, status);
  }
}

}  // namespace dim
