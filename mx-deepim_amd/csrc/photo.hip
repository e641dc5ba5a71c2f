// Photometric pose polish after the refinement loop (RGB test time): a dense direct image alignment between the render at the loop's
// last pose and the observed image.  Restated in numpy by tests/photo_reference.py (planes in float32, the rest in float64); the
// arithmetic below follows it step by step.
//
// Per pair b: gray planes g = (c0 + c1) + c2 of the two mean-subtracted images; 2x2-mean pyramids of the observed gray, the rendered
// gray, the rendered depth and a template-valid flag (level 0: depth > 0 inside the render's bbox; level l: all four children); one
// gain a and bias b from the level-0 template pixels, t = a Ir + b; then from the coarsest level down `iters` Gauss-Newton iterations
// per level on r = I_obs(project(T_delta p0)) - t, bilinear with its analytic gradient, Huber under a hard gate, left twist (omega, v).
//   photo_level0_kernel      the four level-0 planes, four pixels per lane (16-byte loads where the rows allow them)
//   photo_down_kernel        level l from level l - 1, two output pixels per lane (one 16-byte load per input row and plane)
//   photo_stats_kernel       grid (kGnBlocks, B): float64 n, sum Ir, sum Ir^2, sum Io, sum Io^2 per workgroup (block_sum.h)
//   photo_gain_kernel        one workgroup per pair: the 16 partials in order -> the five sums, a, b and whether the pair may step
//   photo_accumulate_kernel  grid (kGnBlocks, B) over the box at the level: float64 per point and per lane, summed across lanes
//                            (block_sum.h) and, in the solve kernel, workgroups in a fixed order
//   gn_solve_kernel          (twist_solve.h) one workgroup per pair, driven with one iteration index over levels * iters
// No atomics, no memcpy / memset: a replay is bit-identical and the stage is graph-capturable.  Float64 per point, as flow_pnp.hip: the
// stage is bound by its dependent launches, and the gate and cell decisions then agree with the restatement's, so the counts are equal.
#include "common.h"
#include "twist_solve.h"

namespace dim {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kPhotoMaxLevels = 5;
constexpr int kPhotoPlanes = 4;    // observed gray, rendered gray, rendered depth, template-valid flag (0.f / 1.f)
constexpr int kPhotoGain = 8;      // doubles per pair: n, sum Ir, sum Ir^2, sum Io, sum Io^2, a, b, may step (1.0 / 0.0)

// workspace: [state B x kGnState][partial B x kGnBlocks x kGnSlot][gain B x kPhotoGain] doubles, then the float planes, kind-major
// then level: plane (kind, level) holds B x H_l x W_l floats and starts at a multiple of 16 bytes
struct PhotoLayout {
  int H[kPhotoMaxLevels], W[kPhotoMaxLevels];
  long off[kPhotoPlanes][kPhotoMaxLevels];   // bytes from the start of the workspace
  long gain, total;                          // bytes
};

static PhotoLayout photo_layout(int B, int H, int W, int levels) {
  PhotoLayout L = {};
  L.gain = gn_workspace_bytes(B);
  long at = L.gain + (long)B * kPhotoGain * (long)sizeof(double);
  for (int l = 0; l < levels; ++l) {
    L.H[l] = l ? L.H[l - 1] / 2 : H;
    L.W[l] = l ? L.W[l - 1] / 2 : W;
  }
  for (int k = 0; k < kPhotoPlanes; ++k)
    for (int l = 0; l < levels; ++l) {
      L.off[k][l] = at;
      at += (((long)B * L.H[l] * L.W[l] + 3) & ~3L) * (long)sizeof(float);
    }
  L.total = at;
  return L;
}

struct PhotoPlanes {
  float* p[kPhotoPlanes];
};

// VEC: W % 4 == 0 and 16-byte aligned planes, so the four pixels x4 .. x4 + 3 of a row are one 16-byte load per plane
template <bool VEC>
__global__ __launch_bounds__(256) void photo_level0_kernel(const float* __restrict__ image_o, const float* __restrict__ image_r,
                                                           const float* __restrict__ depth_r, const int* __restrict__ bbox, int B, int H,
                                                           int W, PhotoPlanes out) {
  const int nq = (W + 3) >> 2;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * nq) return;
  const int q = (int)(i % nq);
  const long by = i / nq;
  const int y = (int)(by % H), b = (int)(by / H);
  const int x4 = 4 * q;
  const PixelBox box = clamp_bbox(bbox, b, H, W);
  const long plane = (long)H * W;
  const long o = (long)b * plane + (long)y * W + x4;       // in the one-plane arrays
  const long o3 = (long)b * 3 * plane + (long)y * W + x4;  // channel 0 of the images
  const bool row_in = y >= box.y0 && y <= box.y1;
  if (VEC) {
    const v4f a0 = *reinterpret_cast<const v4f*>(image_o + o3), a1 = *reinterpret_cast<const v4f*>(image_o + o3 + plane),
              a2 = *reinterpret_cast<const v4f*>(image_o + o3 + 2 * plane);
    const v4f r0 = *reinterpret_cast<const v4f*>(image_r + o3), r1 = *reinterpret_cast<const v4f*>(image_r + o3 + plane),
              r2 = *reinterpret_cast<const v4f*>(image_r + o3 + 2 * plane);
    const v4f d = *reinterpret_cast<const v4f*>(depth_r + o);
    const v4f go = (a0 + a1) + a2, gr = (r0 + r1) + r2;
    v4f v;
    v.x = (row_in && x4 + 0 >= box.x0 && x4 + 0 <= box.x1 && d.x > 0.f) ? 1.f : 0.f;
    v.y = (row_in && x4 + 1 >= box.x0 && x4 + 1 <= box.x1 && d.y > 0.f) ? 1.f : 0.f;
    v.z = (row_in && x4 + 2 >= box.x0 && x4 + 2 <= box.x1 && d.z > 0.f) ? 1.f : 0.f;
    v.w = (row_in && x4 + 3 >= box.x0 && x4 + 3 <= box.x1 && d.w > 0.f) ? 1.f : 0.f;
    *reinterpret_cast<v4f*>(out.p[0] + o) = go;
    *reinterpret_cast<v4f*>(out.p[1] + o) = gr;
    *reinterpret_cast<v4f*>(out.p[2] + o) = d;
    *reinterpret_cast<v4f*>(out.p[3] + o) = v;
  } else {
    for (int k = 0; k < 4 && x4 + k < W; ++k) {
      const float d = depth_r[o + k];
      out.p[0][o + k] = (image_o[o3 + k] + image_o[o3 + plane + k]) + image_o[o3 + 2 * plane + k];
      out.p[1][o + k] = (image_r[o3 + k] + image_r[o3 + plane + k]) + image_r[o3 + 2 * plane + k];
      out.p[2][o + k] = d;
      out.p[3][o + k] = (row_in && x4 + k >= box.x0 && x4 + k <= box.x1 && d > 0.f) ? 1.f : 0.f;
    }
  }
}

// level l (Hl x Wl) from level l - 1 (Hp x Wp), Hl = Hp / 2, Wl = Wp / 2: ((a + b) + (c + d)) * 0.25f with a, b on the upper row; the
// flag is set only where all four children are.  VEC: Wp % 4 == 0 and 16-byte aligned planes (then Wl is even).
template <bool VEC>
__global__ __launch_bounds__(256) void photo_down_kernel(PhotoPlanes src, PhotoPlanes dst, int B, int Hp, int Wp, int Hl, int Wl) {
  const int nq = (Wl + 1) >> 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * Hl * nq) return;
  const int q = (int)(i % nq);
  const long by = i / nq;
  const int Y = (int)(by % Hl), b = (int)(by / Hl);
  const long up = ((long)b * Hp + 2 * Y) * Wp + 4 * q, lo = up + Wp;
  const long o = ((long)b * Hl + Y) * Wl + 2 * q;
  const bool two = 2 * q + 1 < Wl;
#pragma unroll
  for (int k = 0; k < kPhotoPlanes; ++k) {
    float u[4], w[4];
    if (VEC) {
      const v4f u4 = *reinterpret_cast<const v4f*>(src.p[k] + up), w4 = *reinterpret_cast<const v4f*>(src.p[k] + lo);
      u[0] = u4.x; u[1] = u4.y; u[2] = u4.z; u[3] = u4.w;
      w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = e < 2 || two;   // the second output's children: columns 4q + 2, 4q + 3 < 2 Wl <= Wp
        u[e] = in ? src.p[k][up + e] : 0.f;
        w[e] = in ? src.p[k][lo + e] : 0.f;
      }
    }
    float r0, r1;
    if (k == 3) {
      r0 = (u[0] > 0.5f && u[1] > 0.5f && w[0] > 0.5f && w[1] > 0.5f) ? 1.f : 0.f;
      r1 = (u[2] > 0.5f && u[3] > 0.5f && w[2] > 0.5f && w[3] > 0.5f) ? 1.f : 0.f;
    } else {
      r0 = ((u[0] + u[1]) + (w[0] + w[1])) * 0.25f;
      r1 = ((u[2] + u[3]) + (w[2] + w[3])) * 0.25f;
    }
    if (VEC) {
      v2f r;
      r.x = r0; r.y = r1;
      *reinterpret_cast<v2f*>(dst.p[k] + o) = r;
    } else {
      dst.p[k][o] = r0;
      if (two) dst.p[k][o + 1] = r1;
    }
  }
}

__global__ __launch_bounds__(256) void photo_stats_kernel(const float* __restrict__ gray_o, const float* __restrict__ gray_r,
                                                          const float* __restrict__ valid, const int* __restrict__ bbox, int H, int W,
                                                          double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const PixelBox box = clamp_bbox(bbox, b, H, W);
  const int bw = box.x1 - box.x0 + 1;
  const int n = (box.x1 >= box.x0 && box.y1 >= box.y0) ? bw * (box.y1 - box.y0 + 1) : 0;
  const long base = (long)b * H * W;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kGnBlocks * blockDim.x) {
    const int yy = i / bw;
    const long o = base + (long)(box.y0 + yy) * W + box.x0 + (i - yy * bw);
    if (!(valid[o] > 0.5f)) continue;
    const double ir = gray_r[o], io = gray_o[o];
    acc[0] += 1.0;
    acc[1] += ir;
    acc[2] += ir * ir;
    acc[3] += io;
    acc[4] += io * io;
  }
  const double total = block_sum(acc);
  if (tid < 5) partial[((long)b * kGnBlocks + blockIdx.x) * kGnSlot + tid] = total;
}

__global__ __launch_bounds__(64) void photo_gain_kernel(const double* __restrict__ partial, int gain, double* __restrict__ out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double s[5];
  if (tid < 5) {
    double v = 0.0;
    for (int k = 0; k < kGnBlocks; ++k) v += partial[((long)b * kGnBlocks + k) * kGnSlot + tid];
    s[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  double* g = out + (long)b * kPhotoGain;
  for (int k = 0; k < 5; ++k) g[k] = s[k];
  double a = 1.0, bias = 0.0, ok = 0.0;
  const double n = s[0];
  if (n >= (double)kGnMinPoints) {
    const double mr = s[1] / n, mo = s[3] / n;
    const double vr = s[2] / n - mr * mr, vo = s[4] / n - mo * mo;
    if (vr > 0.0 && vo > 0.0 && isfinite(vr) && isfinite(vo)) {
      ok = 1.0;
      if (gain) {
        a = sqrt(vo / vr);
        bias = mo - a * mr;
      }
    }
  }
  g[5] = a;
  g[6] = bias;
  g[7] = ok;
}

// one linearisation at pyramid level lvl (planes Hl x Wl, s = 2^lvl); bbox is the level-0 box of the H0 x W0 frame
__global__ __launch_bounds__(256) void photo_accumulate_kernel(const float* __restrict__ gray_o, const float* __restrict__ gray_r,
                                                               const float* __restrict__ depth, const float* __restrict__ valid,
                                                               const int* __restrict__ bbox, PinholeCam k9,
                                                               const float* __restrict__ K_per_sample, int H0, int W0, int Hl, int Wl,
                                                               int lvl, float huber, float gate, const double* __restrict__ gain, int it,
                                                               const double* __restrict__ state, double* __restrict__ partial) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const PinholeCam c = cam_pick(K_per_sample, k9, b);
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  double R[9], t[3];
  gn_load_pose(state, b, it, R, t);
  const double* g = gain + (long)b * kPhotoGain;
  const double ga = g[5], gb = g[6];
  const bool may_step = g[7] > 0.5 && cam_ok(c);
  const PixelBox box = clamp_bbox(bbox, b, H0, W0);
  // a valid pixel of this level has all its 4^lvl children inside the box, so its column lies in [x0 >> lvl, x1 >> lvl]
  const int x0 = box.x0 >> lvl, x1 = min(box.x1 >> lvl, Wl - 1), y0 = box.y0 >> lvl, y1 = min(box.y1 >> lvl, Hl - 1);
  const int bw = x1 - x0 + 1;
  const int n = (may_step && box.x1 >= box.x0 && box.y1 >= box.y0 && x1 >= x0 && y1 >= y0) ? bw * (y1 - y0 + 1) : 0;
  const long base = (long)b * Hl * Wl;
  const double s = (double)(1 << lvl), half = (s - 1.0) / 2.0;
  const double hub = huber, gt = gate;
  double acc[kGnTerms];
#pragma unroll
  for (int k = 0; k < kGnTerms; ++k) acc[k] = 0.0;
  for (int i = blockIdx.x * blockDim.x + tid; i < n; i += kGnBlocks * blockDim.x) {
    const int yy = i / bw;
    const int X = x0 + (i - yy * bw), Y = y0 + yy;
    const long o = base + (long)Y * Wl + X;
    if (!(valid[o] > 0.5f)) continue;
    const double d = depth[o];
    const double tv = ga * (double)gray_r[o] + gb;
    const double xc = (double)X * s + half, yc = (double)Y * s + half;
    const double sx = d * (xc - cx) / fx, sy = d * (yc - cy) / fy;
    const double px = R[0] * sx + R[1] * sy + R[2] * d + t[0];
    const double py = R[3] * sx + R[4] * sy + R[5] * d + t[1];
    const double pz = R[6] * sx + R[7] * sy + R[8] * d + t[2];
    if (!(pz > 0.0)) continue;
    const double U = ((fx * px / pz + cx) - half) / s, V = ((fy * py / pz + cy) - half) / s;
    const double xf = floor(U), yf = floor(V);
    if (!(xf >= 0.0 && xf < (double)(Wl - 1) && yf >= 0.0 && yf < (double)(Hl - 1))) continue;   // NaN fails too
    const long q = base + (long)yf * Wl + (long)xf;   // the cell: q, q + 1, q + Wl, q + Wl + 1 lie inside the plane
    const double ax = U - xf, ay = V - yf;
    const double i00 = gray_o[q], i01 = gray_o[q + 1], i10 = gray_o[q + Wl], i11 = gray_o[q + Wl + 1];
    const double val = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11);
    const double gx = ((1.0 - ay) * (i01 - i00) + ay * (i11 - i10)) / s;
    const double gy = ((1.0 - ax) * (i10 - i00) + ax * (i11 - i01)) / s;
    const double r = val - tv, e = fabs(r);
    if (!(e <= gt)) continue;   // w = 0 (and a NaN residual)
    const double w = e <= hub ? 1.0 : hub / e;
    // gp = gx du/dp + gy dv/dp, J = (p x gp, gp)
    const double gpx = gx * (fx / pz), gpy = gy * (fy / pz), gpz = -(gx * fx * px + gy * fy * py) / (pz * pz);
    const double J[6] = {py * gpz - pz * gpy, pz * gpx - px * gpz, px * gpy - py * gpx, gpx, gpy, gpz};
    gn_add_row(acc, J, r, w);
    acc[27] += 1.0;
    acc[28] += w * r * r;
  }
  gn_store_partial(acc, partial, b);
}

}  // namespace dim

using namespace dim;

static bool photo_shape_ok(int B, int H, int W, int levels) {
  return B > 0 && levels >= 1 && levels <= kPhotoMaxLevels && H > 0 && W > 0 && (H >> (levels - 1)) >= 3 && (W >> (levels - 1)) >= 3;
}

extern "C" long dim_photo_workspace_bytes(int B, int H, int W, int levels) {
  return photo_shape_ok(B, H, W, levels) ? photo_layout(B, H, W, levels).total : 0;
}

extern "C" long dim_photo_workspace_offset(int B, int H, int W, int levels, int plane, int level) {
  if (!photo_shape_ok(B, H, W, levels)) return -1;
  const PhotoLayout L = photo_layout(B, H, W, levels);
  if (plane == kPhotoPlanes) return L.gain;
  if (plane < 0 || plane > kPhotoPlanes || level < 0 || level >= levels) return -1;
  return L.off[plane][level];
}

// both entries: views == nullptr is dim_photo_refine
static int photo_run(const float* image_observed, const float* image_rendered, const float* depth_rendered, const int* bbox,
                     const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int levels, int iters,
                     float huber, float gate, int gain, void* workspace, float* pose_out, float* stats, int* status, const GnViews* views,
                     void* stream) {
  DIM_REQUIRE(B > 0, "photo_refine: B = %d", B);
  DIM_REQUIRE(levels >= 1 && levels <= kPhotoMaxLevels, "photo_refine: levels = %d (1 .. %d)", levels, kPhotoMaxLevels);
  DIM_REQUIRE(iters >= 0, "photo_refine: iters = %d", iters);
  DIM_REQUIRE(huber > 0.f, "photo_refine: huber must be > 0");
  DIM_REQUIRE(gate >= huber, "photo_refine: gate must be >= huber");
  DIM_REQUIRE(photo_shape_ok(B, H, W, levels), "photo_refine: image %d x %d is smaller than 3 x 3 at the coarsest of %d levels", H, W,
              levels);
  DIM_REQUIRE(image_observed && image_rendered && depth_rendered && pose_in && K9 && workspace && pose_out, "photo_refine: null pointer");
  DIM_REQUIRE(!views || gn_views_ok(*views, B), "photo_refine_views: V in 1 .. %d dividing B = %d, cam_T_rig, pose_rig_in and pose_rig_out required",
              kGnMaxViews, B);
  if (iters == 0) {
    const int rc = dim_copy_words(pose_out, pose_in, 12L * B, stream);
    return (rc != DIM_OK || !views) ? rc : dim_copy_words(views->pose_rig_out, views->pose_rig_in, 12L * (B / views->V), stream);
  }
  const hipStream_t st = as_stream(stream);
  const PinholeCam k9 = cam_of_k9(K9);
  const PhotoLayout L = photo_layout(B, H, W, levels);
  char* ws = (char*)workspace;
  const GnWorkspace gn(workspace, B);
  double* gains = (double*)(ws + L.gain);
  PhotoPlanes lv[kPhotoMaxLevels];
  for (int l = 0; l < levels; ++l)
    for (int k = 0; k < kPhotoPlanes; ++k) lv[l].p[k] = (float*)(ws + L.off[k][l]);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool ws16 = al16(workspace);
  const bool vec0 = W % 4 == 0 && ws16 && al16(image_observed) && al16(image_rendered) && al16(depth_rendered);
  hipLaunchKernelGGL(vec0 ? photo_level0_kernel<true> : photo_level0_kernel<false>, dim3(ceil_div((long)B * H * ((W + 3) >> 2), 256)),
                     dim3(256), 0, st, image_observed, image_rendered, depth_rendered, bbox, B, H, W, lv[0]);
  for (int l = 1; l < levels; ++l) {
    const bool vec = L.W[l - 1] % 4 == 0 && ws16;
    hipLaunchKernelGGL(vec ? photo_down_kernel<true> : photo_down_kernel<false>,
                       dim3(ceil_div((long)B * L.H[l] * ((L.W[l] + 1) >> 1), 256)), dim3(256), 0, st, lv[l - 1], lv[l], B, L.H[l - 1],
                       L.W[l - 1], L.H[l], L.W[l]);
  }
  hipLaunchKernelGGL(photo_stats_kernel, dim3(kGnBlocks, B), dim3(256), 0, st, (const float*)lv[0].p[0], (const float*)lv[0].p[1],
                     (const float*)lv[0].p[3], bbox, H, W, gn.partial);
  hipLaunchKernelGGL(photo_gain_kernel, dim3(B), dim3(64), 0, st, (const double*)gn.partial, gain, gains);
  // one iteration index over levels * iters, from the coarsest level down
  gn_iterate_either<DIM_STATUS_PHOTO_FEW_POINTS>(gn, (double*)(ws + L.total), B, views, levels * iters, pose_in, pose_out, stats, status, st,
                                                 [&](int it) {
    const int l = levels - 1 - it / iters;
    hipLaunchKernelGGL(photo_accumulate_kernel, dim3(kGnBlocks, B), dim3(256), 0, st, (const float*)lv[l].p[0], (const float*)lv[l].p[1],
                       (const float*)lv[l].p[2], (const float*)lv[l].p[3], bbox, k9, K_per_sample, H, W, L.H[l], L.W[l], l, huber, gate,
                       (const double*)gains, it, (const double*)gn.state, gn.partial);
  });
  return check_launch(views ? "photo_refine_views" : "photo_refine");
}

extern "C" int dim_photo_refine(const float* image_observed, const float* image_rendered, const float* depth_rendered, const int* bbox,
                                const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int levels,
                                int iters, float huber, float gate, int gain, void* workspace, float* pose_out, float* stats,
                                int* status, void* stream) {
  return photo_run(image_observed, image_rendered, depth_rendered, bbox, pose_in, K9, K_per_sample, B, H, W, levels, iters, huber, gate, gain,
                   workspace, pose_out, stats, status, nullptr, stream);
}

// the single-view layout unchanged (every plane offset keeps its meaning), the group state rows behind it
extern "C" long dim_photo_views_workspace_bytes(int B, int H, int W, int levels, int V) {
  return (photo_shape_ok(B, H, W, levels) && V > 0) ? photo_layout(B, H, W, levels).total + gn_views_state_bytes(B, V) : 0;
}

extern "C" int dim_photo_refine_views(const float* image_observed, const float* image_rendered, const float* depth_rendered, const int* bbox,
                                      const float* pose_in, const float* K9, const float* K_per_sample, int B, int H, int W, int levels,
                                      int iters, float huber, float gate, int gain, void* workspace, float* pose_out, float* stats,
                                      int* status, const float* cam_T_rig, int V, const float* pose_rig_in, float* pose_rig_out,
                                      float* stats_group, void* stream) {
  const GnViews views{cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group};
  return photo_run(image_observed, image_rendered, depth_rendered, bbox, pose_in, K9, K_per_sample, B, H, W, levels, iters, huber, gate, gain,
                   workspace, pose_out, stats, status, &views, stream);
}
