// Pose tracking through a video: the temporal layer around the refinement loop.  P tracks share one camera; everything a frame
// needs between two runs of the loop stays on the device.  Restated in float64 numpy by tests/track_reference.py.
//   track_ingest_kernel    one camera frame (uint8 BGR, optional uint16 depth) -> the observed blobs of the P tracks.  One thread per
//                          4 consecutive pixels: 12 bytes of colour (three dwords) and 8 of depth in, then P times three (four) float4
//                          out -- the frame bytes are loaded once, every store is 16 bytes.  Per pixel the bits of
//                          pair_blobs_from_raw_kernel (data.hip): plane c = bgr[2 - c] - mean[2 - c], depth = __fdiv_rn(raw, factor)
//   track_predict_kernel   one lane per track: the pose the frame starts from, from the last two accepted poses (hold / damped
//                          constant velocity), float64 inside, one rounding to float32
//   track_update_kernel<OCC>  one lane per track: the last iteration's step into a ring, its window means, the lost test, and the
//                          history / re-initialisation state machine.  Every pose written into the history is a bit-for-bit copy.
//                          The rules stand once, numbered as in deepim_hip.h.  OCC = false is dim_track_update.  OCC = true is
//                          dim_track_update_occ: an "occluded" state in front of rules 2 to 6 -- a track of which too little is
//                          visible coasts on the predicted pose, within a budget of frames, instead of being lost -- and a track
//                          that is not occluded takes the same statements, so min_visible = 0 gives the bits of OCC = false.  Each
//                          entry is pinned on its own: tests/track_reference.py (false), tests/track_occ_reference.py (true)
//   track_visibility_kernel  occlusion between the tracks and against the frame's depth: one lane per 4 (or 1) pixels, P the inner
//                          loop.  Each render is read (twice when tracks hide tracks: the two smallest depths first) and written
//                          once with its hidden pixels zeroed -- a depth plane dim_pose_score takes as it is -- and the pixel counts
//                          leave as one packed word per (wave, track); track_visibility_finish adds them: integers, no atomics.
//                          Restated by tests/track_occ_reference.py
// Nothing allocates or synchronises: every entry is graph-capturable.
#include "common.h"
#include "twist_solve.h"

namespace dim {

__global__ __launch_bounds__(256) void track_ingest_kernel(const unsigned char* __restrict__ frame_bgr,
                                                           const unsigned short* __restrict__ depth_raw, int P, int plane,
                                                           float depth_factor, float mb, float mg, float mr,
                                                           float* __restrict__ image_observed, float* __restrict__ depth_observed) {
  const int pix = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (pix >= plane) return;   // plane % 4 == 0: a live thread owns four whole pixels
  const float means[3] = {mb, mg, mr};
  const uint3 raw = *reinterpret_cast<const uint3*>(frame_bgr + (long)pix * 3);   // 12 bytes = 4 pixels x (B, G, R)
  const unsigned w[3] = {raw.x, raw.y, raw.z};
  float v[4][3];
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k / 3][k % 3] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
  float4 out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)   // plane c holds BGR channel 2 - c
    out[c] = make_float4(v[0][2 - c] - means[2 - c], v[1][2 - c] - means[2 - c], v[2][2 - c] - means[2 - c], v[3][2 - c] - means[2 - c]);
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool with_depth = depth_raw && depth_observed;
  if (with_depth) {
    const uint2 dr = *reinterpret_cast<const uint2*>(depth_raw + pix);
    d = make_float4(__fdiv_rn((float)(dr.x & 0xFFFFu), depth_factor), __fdiv_rn((float)(dr.x >> 16), depth_factor),
                    __fdiv_rn((float)(dr.y & 0xFFFFu), depth_factor), __fdiv_rn((float)(dr.y >> 16), depth_factor));
  }
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(image_observed + ((long)p * 3 + c) * plane + pix) = out[c];
    if (with_depth) *reinterpret_cast<float4*>(depth_observed + (long)p * plane + pix) = d;
  }
}

__device__ __forceinline__ bool pose_finite(const float* T) {
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && isfinite(T[k]);
  return ok;
}

// D = A B^T of the rotation parts of two (3,4) float32 poses, float64
__device__ __forceinline__ void rel_rotation(const float* A, const float* B, double* D) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      D[3 * i + j] = (double)A[4 * i] * (double)B[4 * j] + (double)A[4 * i + 1] * (double)B[4 * j + 1] + (double)A[4 * i + 2] * (double)B[4 * j + 2];
}

// half the antisymmetric part of D as a vector (= sin(angle) axis), its length, and cos(angle) = (tr D - 1) / 2
__device__ __forceinline__ void rotation_sin_cos(const double* D, double* v, double* s, double* c) {
  v[0] = 0.5 * (D[7] - D[5]);
  v[1] = 0.5 * (D[2] - D[6]);
  v[2] = 0.5 * (D[3] - D[1]);
  *s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  *c = 0.5 * (D[0] + D[4] + D[8] - 1.0);
}

// Axis-angle logarithm of a rotation matrix: w = angle * axis with angle = atan2(s, c) in [0, pi].
//   c >= -0.5, s < 1e-8: w = v (angle / sin(angle) = 1 to 1e-17 there; exactly 0 at the identity)
//   c >= -0.5 otherwise: the axis is v / s
//   c <  -0.5:           sin(angle) fades towards pi, so the axis comes from the symmetric part: (D + D^T) / 2 = c I + (1 - c) a a^T;
//                        its largest diagonal entry gives |a_k|, row k the other two, and the sign is the one of v (any at pi itself)
__device__ inline void rotation_log(const double* D, double* w) {
  double v[3], s, c;
  rotation_sin_cos(D, v, &s, &c);
  const double angle = atan2(s, c);
  if (c >= -0.5 && s < 1e-8) {
    for (int k = 0; k < 3; ++k) w[k] = v[k];
    return;
  }
  double a[3];
  if (c >= -0.5) {
    for (int k = 0; k < 3; ++k) a[k] = v[k] / s;
  } else {
    double M[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) M[3 * i + j] = (0.5 * (D[3 * i + j] + D[3 * j + i]) - (i == j ? c : 0.0)) / (1.0 - c);
    int k = 0;
    if (M[4] > M[0]) k = 1;
    if (M[8] > M[4 * k]) k = 2;
    const double ak = sqrt(fmax(M[4 * k], 0.0));
    if (!(ak > 0.0)) {   // no rotation matrix at all: no motion
      for (int j = 0; j < 3; ++j) w[j] = 0.0;
      return;
    }
    for (int j = 0; j < 3; ++j) a[j] = j == k ? ak : M[3 * k + j] / ak;
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double sign = (a[0] * v[0] + a[1] * v[1] + a[2] * v[2]) < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; ++j) a[j] *= sign / n;
  }
  for (int k = 0; k < 3; ++k) w[k] = angle * a[k];
}

__global__ __launch_bounds__(64) void track_predict_kernel(const float* __restrict__ hist, const int* __restrict__ age, int P, int mode,
                                                           double alpha, float* __restrict__ pose_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* prev = hist + 24L * p;
  const float* last = prev + 12;
  float* out = pose_out + 12L * p;
  bool hold = mode != DIM_TRACK_MOTION_VELOCITY || age[p] < 2 || !pose_finite(prev) || !pose_finite(last);
  hold = hold || !(prev[11] > 0.f) || !(last[11] > 0.f);
  if (hold) {
    for (int k = 0; k < 12; ++k) out[k] = last[k];
    return;
  }
  double D[9], w[3], Rw[9];
  rel_rotation(last, prev, D);   // the camera-frame rotation from the frame before to the last one
  rotation_log(D, w);
  for (int k = 0; k < 3; ++k) w[k] *= alpha;
  twist_rodrigues(w, Rw);
  // translation in the network's untangled coordinates: u = tx / tz and v = ty / tz linear, log tz linear
  const double zp = prev[11], zl = last[11];
  const double up = (double)prev[3] / zp, vp = (double)prev[7] / zp, ul = (double)last[3] / zl, vl = (double)last[7] / zl;
  const double z = zl * pow(zl / zp, alpha);
  const double u = ul + alpha * (ul - up), v = vl + alpha * (vl - vp);
  const double t[3] = {u * z, v * z, z};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out[4 * i + j] = (float)(Rw[3 * i] * (double)last[j] + Rw[3 * i + 1] * (double)last[4 + j] + Rw[3 * i + 2] * (double)last[8 + j]);
    out[4 * i + 3] = (float)t[i];
  }
}

struct TrackUpdateArgs {
  const float* pose_before;
  const float* pose_new;
  const int* status_rows;
  int n_rows, fatal_mask;
  const float* score;
  float min_score;
  const float* reinit_pose;
  const int* reinit_valid;
  float lost_rot_deg, lost_trans_m;
  int Wn;
  float znear, zfar;
  int P;
  float* hist;
  int* age;
  float* ring;
  int* ring_n;
  int* ring_pos;
  int* flags;
  float* step;
  float* mean;
  // dim_track_update_occ only (null / 0 otherwise: OCC = false reads and writes none of them)
  const int* counts;
  float min_visible;
  int max_occluded;
  const float* pose_pred;
  int* occ_age;
  float* visible;
  float* pose_track;
  int* occluder_ok;
};

template <bool OCC>
__global__ __launch_bounds__(64) void track_update_kernel(TrackUpdateArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.P) return;
  const int Wn = a.Wn;
  const float* Tb = a.pose_before + 12L * p;
  const float* Tn = a.pose_new + 12L * p;
  int status = 0;
  for (int r = 0; r < a.n_rows; ++r) status |= a.status_rows[(long)r * a.P + p];
  // 1. the step of the loop's last iteration
  double D[9], v[3], s, c;
  rel_rotation(Tn, Tb, D);
  rotation_sin_cos(D, v, &s, &c);
  double step_rot = atan2(s, c) * (180.0 / 3.14159265358979323846);
  const double dx = (double)Tn[3] - (double)Tb[3], dy = (double)Tn[7] - (double)Tb[7], dz = (double)Tn[11] - (double)Tb[11];
  double step_trans = sqrt(dx * dx + dy * dy + dz * dz);
  if (!isfinite(step_rot)) step_rot = INFINITY;
  if (!isfinite(step_trans)) step_trans = INFINITY;
  a.step[2 * p] = (float)step_rot;
  a.step[2 * p + 1] = (float)step_trans;
  // the fatal clauses of 3.: with them there is nothing to judge a visibility on
  bool lost = (status & a.fatal_mask) != 0 || !pose_finite(Tn);
  lost = lost || !(Tn[11] >= a.znear && Tn[11] <= a.zfar);
  bool occluded = false;   // too little of the drawn render is visible
  if (OCC) {
    const int drawn = a.counts[4 * p], seen = a.counts[4 * p + 1];
    a.visible[p] = drawn > 0 ? (float)((double)seen / (double)drawn) : 0.f;
    occluded = !lost && drawn > 0 && (double)seen < (double)a.min_visible * (double)drawn;
  }
  float* ring = a.ring + 2L * Wn * p;
  int pos = a.ring_pos[p], n = a.ring_n[p];
  if (pos < 0 || pos >= Wn) pos = 0;
  n = min(max(n, 0), Wn);
  float* h0 = a.hist + 24L * p;
  float* h1 = h0 + 12;
  int age = min(max(a.age[p], 0), 2);
  int occ_age = OCC ? max(a.occ_age[p], 0) : 0;
  bool reinit = false;
  if (!occluded) {
    // 2. into the ring over its oldest entry
    ring[2 * pos] = (float)step_rot;
    ring[2 * pos + 1] = (float)step_trans;
    pos = pos + 1 == Wn ? 0 : pos + 1;
    n = min(n + 1, Wn);
  }
  // the means over the ring's entries as they are stored, oldest first (an occluded track: of what was stored before, 0 of nothing)
  double sum_rot = 0.0, sum_trans = 0.0;
  for (int k = 0; k < n; ++k) {
    const int q = (pos - n + k + Wn) % Wn;
    sum_rot += (double)ring[2 * q];
    sum_trans += (double)ring[2 * q + 1];
  }
  const bool some = !OCC || n > 0;   // only an occluded track's ring can hold nothing here
  const double mean_rot = some ? sum_rot / n : 0.0, mean_trans = some ? sum_trans / n : 0.0;
  a.mean[2 * p] = (float)mean_rot;
  a.mean[2 * p + 1] = (float)mean_trans;
  bool coast = false;
  if (occluded) {
    const float* Tp = a.pose_pred + 12L * p;
    coast = occ_age < a.max_occluded && pose_finite(Tp) && Tp[11] >= a.znear && Tp[11] <= a.zfar;
    status |= DIM_STATUS_TRACK_OCCLUDED;
    if (coast) {   // hidden, within the budget: the motion model's pose is the frame's pose
      for (int k = 0; k < 12; ++k) h0[k] = h1[k];
      for (int k = 0; k < 12; ++k) h1[k] = Tp[k];
      age = min(age + 1, 2);
      occ_age += 1;
    } else {
      lost = true;
    }
  } else {
    // 3. lost?
    if (a.score) lost = lost || !(a.score[p] >= a.min_score);
    if (n == Wn) lost = lost || mean_rot > (double)a.lost_rot_deg || mean_trans > (double)a.lost_trans_m;
  }
  if (!coast) {
    occ_age = 0;
    if (!lost) {                                              // 4. accepted
      for (int k = 0; k < 12; ++k) h0[k] = h1[k];
      for (int k = 0; k < 12; ++k) h1[k] = Tn[k];
      age = min(age + 1, 2);
    } else if (a.reinit_valid && a.reinit_pose && a.reinit_valid[p] != 0) {   // 5. lost, a pose is offered
      const float* Tr = a.reinit_pose + 12L * p;
      for (int k = 0; k < 12; ++k) h1[k] = Tr[k];
      age = 1;
      for (int k = 0; k < 2 * Wn; ++k) ring[k] = 0.f;
      n = 0;
      pos = 0;
      reinit = true;
      status |= DIM_STATUS_TRACK_LOST | DIM_STATUS_TRACK_REINIT;
    } else {                                                  // 6. lost, nothing offered: the last accepted pose, no velocity
      age = min(age, 1);
      status |= DIM_STATUS_TRACK_LOST;
    }
    a.ring_n[p] = n;
    a.ring_pos[p] = pos;
  }
  a.age[p] = age;
  a.flags[p] = status;
  if (OCC) {
    a.occ_age[p] = occ_age;
    for (int k = 0; k < 12; ++k) a.pose_track[12L * p + k] = h1[k];
    a.occluder_ok[p] = (lost && !reinit) ? 0 : 1;
  }
}

// ---- occlusion: which drawn pixels of each track's render does another track, or the frame's own depth, hide
constexpr int kVisThreads = 256;
constexpr int kVisField = 10;   // a lane counts at most 4 pixels per class and a wave at most 256: three 10-bit fields in one word
constexpr unsigned kVisFieldMask = (1u << kVisField) - 1u;

__device__ __forceinline__ bool depth_drawn(float d) { return d > 0.f && d < INFINITY; }   // NaN, +inf, 0 and negatives are not drawn

// V pixels per lane: 4 (one 16-byte access per plane) or 1.  Pass 1 (only with DIM_TRACK_OCC_TRACKS): the smallest and the second
// smallest drawn depth of the eligible tracks at each pixel, with the track of the smallest -- x -> float32(d - x) is monotone, so
// "some eligible q != p with d_p - d_q > delta" is "d_p - m_p > delta", m_p the smallest eligible depth of a track other than p.
// Pass 2: classify and write.  Counts leave as one packed word per (wave, track) into `partial`; track_visibility_finish sums them.
// No lane returns early: every lane takes part in the butterfly.
template <int V>
__global__ __launch_bounds__(kVisThreads) void track_visibility_kernel(const float* __restrict__ depth_rendered,
                                                                       const float* __restrict__ depth_frame,
                                                                       const int* __restrict__ occluder_ok, int P, long plane, int mode,
                                                                       float delta, float* __restrict__ depth_visible,
                                                                       unsigned* __restrict__ partial) {
  const long pix = (long)V * ((long)blockIdx.x * kVisThreads + threadIdx.x);
  const bool live = pix < plane;   // V == 4: plane % 4 == 0, a live lane owns four whole pixels
  float d[V], m1[V], m2[V], o[V];
  int i1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    m1[j] = m2[j] = INFINITY;
    i1[j] = -1;
    o[j] = 0.f;
  }
  auto load = [&](const float* src, float* v) {
    if (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(src + pix);
      v[0] = q.x; v[1 % V] = q.y; v[2 % V] = q.z; v[3 % V] = q.w;
    } else {
      v[0] = src[pix];
    }
  };
  if (live && (mode & DIM_TRACK_OCC_TRACKS)) {
    for (int p = 0; p < P; ++p) {
      if (occluder_ok && occluder_ok[p] == 0) continue;
      load(depth_rendered + (long)p * plane, d);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (!depth_drawn(d[j])) continue;
        if (d[j] < m1[j]) {
          m2[j] = m1[j];
          m1[j] = d[j];
          i1[j] = p;
        } else if (d[j] < m2[j]) {
          m2[j] = d[j];
        }
      }
    }
  }
  if (live && (mode & DIM_TRACK_OCC_DEPTH)) {
    load(depth_frame, o);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (!depth_drawn(o[j])) o[j] = 0.f;   // no reading: hides nothing
  }
  const int wave = blockIdx.x * (kVisThreads / kWave) + threadIdx.x / kWave;
  for (int p = 0; p < P; ++p) {
    unsigned c = 0;
    if (live) {
      load(depth_rendered + (long)p * plane, d);
      float out[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        out[j] = 0.f;
        if (!depth_drawn(d[j])) continue;
        const float m = i1[j] == p ? m2[j] : m1[j];
        if (d[j] - m > delta) {
          c += 1u << kVisField;
        } else if (o[j] > 0.f && d[j] - o[j] > delta) {
          c += 1u << (2 * kVisField);
        } else {
          c += 1u;
          out[j] = d[j];
        }
      }
      float* dst = depth_visible + (long)p * plane + pix;
      if (V == 4)
        *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1 % V], out[2 % V], out[3 % V]);
      else
        *dst = out[0];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
    if (threadIdx.x % kWave == 0) partial[(long)wave * P + p] = c;
  }
}

// one wave per track: the packed words of all waves -> counts (P,4) = {drawn, visible, hidden by a track, hidden by the depth only}
__global__ __launch_bounds__(kWave) void track_visibility_finish(const unsigned* __restrict__ partial, int P, int waves,
                                                                 int* __restrict__ counts) {
  const int p = blockIdx.x;
  int vis = 0, trk = 0, dep = 0;
  for (int w = threadIdx.x; w < waves; w += kWave) {
    const unsigned c = partial[(long)w * P + p];
    vis += (int)(c & kVisFieldMask);
    trk += (int)((c >> kVisField) & kVisFieldMask);
    dep += (int)(c >> (2 * kVisField));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    vis += __shfl_xor(vis, s, 64);
    trk += __shfl_xor(trk, s, 64);
    dep += __shfl_xor(dep, s, 64);
  }
  if (threadIdx.x == 0) {
    int* c = counts + 4L * p;
    c[0] = vis + trk + dep;
    c[1] = vis;
    c[2] = trk;
    c[3] = dep;
  }
}

}  // namespace dim

using namespace dim;

extern "C" int dim_track_ingest(const unsigned char* frame_bgr, const unsigned short* depth_raw, int P, int H, int W, float depth_factor,
                                const float* pixel_means_bgr3, float* image_observed, float* depth_observed, void* stream) {
  DIM_REQUIRE(P > 0 && H > 0 && W > 0 && W % 4 == 0 && (long)H * W < (1L << 31), "track_ingest: P = %d, H = %d, W = %d (W must be a multiple of 4)",
              P, H, W);
  DIM_REQUIRE(depth_factor > 0.f, "track_ingest: depth_factor must be positive");
  DIM_REQUIRE(frame_bgr && pixel_means_bgr3 && image_observed, "track_ingest: null pointer");
  DIM_REQUIRE(!depth_observed || depth_raw, "track_ingest: depth_observed needs depth_raw");
  DIM_REQUIRE((reinterpret_cast<uintptr_t>(frame_bgr) & 3) == 0 && (reinterpret_cast<uintptr_t>(depth_raw) & 7) == 0 &&
                  ((reinterpret_cast<uintptr_t>(image_observed) | reinterpret_cast<uintptr_t>(depth_observed)) & 15) == 0,
              "track_ingest: pointer alignment: raw frame 4 bytes, raw depth 8 bytes, float planes 16 bytes");
  const int plane = H * W;
  hipLaunchKernelGGL(track_ingest_kernel, dim3(ceil_div(plane / 4, 256)), dim3(256), 0, as_stream(stream), frame_bgr, depth_raw, P, plane,
                     depth_factor, pixel_means_bgr3[0], pixel_means_bgr3[1], pixel_means_bgr3[2], image_observed, depth_observed);
  return check_launch("track_ingest");
}

extern "C" int dim_track_predict(const float* hist, const int* age, int P, int mode, float alpha, float* pose_out, void* stream) {
  DIM_REQUIRE(P > 0, "track_predict: P = %d", P);
  DIM_REQUIRE(mode == DIM_TRACK_MOTION_HOLD || mode == DIM_TRACK_MOTION_VELOCITY, "track_predict: mode = %d", mode);
  DIM_REQUIRE(alpha >= 0.f && alpha <= 1.f, "track_predict: alpha = %g outside [0, 1]", (double)alpha);
  DIM_REQUIRE(hist && age && pose_out, "track_predict: null pointer");
  hipLaunchKernelGGL(track_predict_kernel, dim3(ceil_div(P, 64)), dim3(64), 0, as_stream(stream), hist, age, P, mode, (double)alpha, pose_out);
  return check_launch("track_predict");
}

static TrackUpdateArgs track_update_args(const float* pose_before, const float* pose_new, const int* status_rows, int n_rows, int fatal_mask,
                                         const float* score, float min_score, const float* reinit_pose, const int* reinit_valid,
                                         float lost_rot_deg, float lost_trans_m, int Wn, float znear, float zfar, int P, float* hist,
                                         int* age, float* ring, int* ring_n, int* ring_pos, int* flags, float* step, float* mean) {
  return {pose_before, pose_new, status_rows, n_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid, lost_rot_deg, lost_trans_m,
          Wn, znear, zfar, P, hist, age, ring, ring_n, ring_pos, flags, step, mean,
          nullptr, 0.f, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
}

// the checks of dim_track_update (`name` "track_update") and dim_track_update_occ ("track_update_occ"), and the launch
template <bool OCC>
static int track_update_launch(const char* name, const TrackUpdateArgs& a, void* stream) {
  DIM_REQUIRE(a.P > 0 && a.n_rows >= 0, "%s: P = %d, n_rows = %d", name, a.P, a.n_rows);
  DIM_REQUIRE(a.Wn >= 1 && a.Wn <= DIM_TRACK_MAX_WINDOW, "%s: Wn = %d outside [1, %d]", name, a.Wn, DIM_TRACK_MAX_WINDOW);
  if (OCC) {
    DIM_REQUIRE(a.min_visible >= 0.f && a.min_visible <= 1.f, "%s: min_visible = %g outside [0, 1]", name, (double)a.min_visible);
    DIM_REQUIRE(a.max_occluded >= 0, "%s: max_occluded = %d", name, a.max_occluded);
  }
  DIM_REQUIRE(a.pose_before && a.pose_new && a.hist && a.age && a.ring && a.ring_n && a.ring_pos && a.flags && a.step && a.mean,
              "%s: null pointer", name);
  if (OCC)
    DIM_REQUIRE(a.counts && a.pose_pred && a.occ_age && a.visible && a.pose_track && a.occluder_ok, "%s: null pointer", name);
  DIM_REQUIRE(a.n_rows == 0 || a.status_rows, "%s: null pointer (status_rows)", name);
  DIM_REQUIRE((a.reinit_pose == nullptr) == (a.reinit_valid == nullptr), "%s: reinit_pose and reinit_valid go together", name);
  hipLaunchKernelGGL(track_update_kernel<OCC>, dim3(ceil_div(a.P, 64)), dim3(64), 0, as_stream(stream), a);
  return check_launch(name);
}

extern "C" int dim_track_update(const float* pose_before, const float* pose_new, const int* status_rows, int n_rows, int fatal_mask,
                                const float* score, float min_score, const float* reinit_pose, const int* reinit_valid,
                                float lost_rot_deg, float lost_trans_m, int Wn, float znear, float zfar, int P, float* hist, int* age,
                                float* ring, int* ring_n, int* ring_pos, int* flags, float* step, float* mean, void* stream) {
  return track_update_launch<false>("track_update",
                                    track_update_args(pose_before, pose_new, status_rows, n_rows, fatal_mask, score, min_score, reinit_pose,
                                                      reinit_valid, lost_rot_deg, lost_trans_m, Wn, znear, zfar, P, hist, age, ring, ring_n,
                                                      ring_pos, flags, step, mean),
                                    stream);
}

static long visibility_waves(long plane, int V) { return (long)ceil_div(plane, (long)kVisThreads * V) * (kVisThreads / kWave); }

extern "C" long dim_track_visibility_workspace_bytes(int P, int H, int W) {
  if (P <= 0 || H <= 0 || W <= 0) return 0;
  return visibility_waves((long)H * W, 1) * P * (long)sizeof(unsigned);   // the one-pixel-per-lane path has the most waves
}

extern "C" int dim_track_visibility(const float* depth_rendered, const float* depth_frame, const int* occluder_ok, int P, int H, int W,
                                    int mode, float delta, void* workspace, float* depth_visible, int* counts, void* stream) {
  DIM_REQUIRE(P > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31), "track_visibility: P = %d, H = %d, W = %d", P, H, W);
  DIM_REQUIRE(mode != 0 && (mode & ~(DIM_TRACK_OCC_TRACKS | DIM_TRACK_OCC_DEPTH)) == 0, "track_visibility: mode = %d", mode);
  DIM_REQUIRE(!(mode & DIM_TRACK_OCC_DEPTH) || depth_frame, "track_visibility: DIM_TRACK_OCC_DEPTH needs depth_frame");
  DIM_REQUIRE(delta >= 0.f && delta < INFINITY, "track_visibility: delta = %g must be finite and >= 0", (double)delta);
  DIM_REQUIRE(depth_rendered && workspace && depth_visible && counts, "track_visibility: null pointer");
  DIM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "track_visibility: the workspace must be 4-byte aligned");
  const long plane = (long)H * W;
  const float* frame = (mode & DIM_TRACK_OCC_DEPTH) ? depth_frame : nullptr;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = W % 4 == 0 && al(depth_rendered) && al(depth_visible) && (!frame || al(frame));
  const int V = vec ? 4 : 1;
  const int blocks = ceil_div(plane, (long)kVisThreads * V);
  unsigned* partial = reinterpret_cast<unsigned*>(workspace);
  if (vec)
    hipLaunchKernelGGL(track_visibility_kernel<4>, dim3(blocks), dim3(kVisThreads), 0, as_stream(stream), depth_rendered, frame, occluder_ok,
                       P, plane, mode, delta, depth_visible, partial);
  else
    hipLaunchKernelGGL(track_visibility_kernel<1>, dim3(blocks), dim3(kVisThreads), 0, as_stream(stream), depth_rendered, frame, occluder_ok,
                       P, plane, mode, delta, depth_visible, partial);
  hipLaunchKernelGGL(track_visibility_finish, dim3(P), dim3(kWave), 0, as_stream(stream), (const unsigned*)partial, P,
                     (int)visibility_waves(plane, V), counts);
  return check_launch("track_visibility");
}

extern "C" int dim_track_update_occ(const float* pose_before, const float* pose_new, const int* status_rows, int n_rows, int fatal_mask,
                                    const float* score, float min_score, const float* reinit_pose, const int* reinit_valid,
                                    float lost_rot_deg, float lost_trans_m, int Wn, float znear, float zfar, int P, const int* counts,
                                    float min_visible, int max_occluded, const float* pose_pred, float* hist, int* age, float* ring,
                                    int* ring_n, int* ring_pos, int* occ_age, int* flags, float* step, float* mean, float* visible,
                                    float* pose_track, int* occluder_ok, void* stream) {
  TrackUpdateArgs a = track_update_args(pose_before, pose_new, status_rows, n_rows, fatal_mask, score, min_score, reinit_pose, reinit_valid,
                                        lost_rot_deg, lost_trans_m, Wn, znear, zfar, P, hist, age, ring, ring_n, ring_pos, flags, step, mean);
  a.counts = counts;
  a.min_visible = min_visible;
  a.max_occluded = max_occluded;
  a.pose_pred = pose_pred;
  a.occ_age = occ_age;
  a.visible = visible;
  a.pose_track = pose_track;
  a.occluder_ok = occluder_ok;
  return track_update_launch<true>("track_update_occ", a, stream);
}
