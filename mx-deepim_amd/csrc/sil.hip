// Silhouette pose polish after the refinement loop: the contour of the render at a pose is pulled onto the edge of a segmentation
// mask (a RAPID-style contour alignment for textureless objects).  Restated in float64 numpy by tests/sil_reference.py; the
// arithmetic below follows it step by step.
//
// dim_sil_edge_field: the exact nearest-edge field of a mask within `radius` (a windowed Euclidean feature transform), in integers.
//   sil_column_kernel  grid (ceil(W/64), ceil(H/32), B), 64 lanes across x (coalesced rows) x 4 row groups: the edge flags of the
//                      tile's 32 rows and `radius` rows above and below it go to LDS (one byte each, <= 160 x 64), then every pixel
//                      finds the nearest edge row of its own column, the smaller row on a tie, and writes it (-1: none) into field
//   sil_row_kernel     grid (H, B), one workgroup per row: the whole pass-1 row is staged in LDS as 16-bit rows (W <= 32767: < 64 KB),
//                      then every pixel scans x' in [x - radius, x + radius] upwards and keeps the first least dx^2 + dy^2 <= radius^2.
//                      The row is rewritten in place only after the barrier behind the staging, and no other workgroup reads it.
//   Column first, then row, both ties to the smaller coordinate: the minimum of the key (d^2, ex, ey).  O(radius) work per pixel.
// dim_sil_refine: Gauss-Newton on T = [R | t] from the identity, as flow_pnp.hip, with the field's edge pixel as the target.
//   sil_accumulate_kernel  grid (kGnBlocks, B): the box is scanned in chunks of 256 pixels per workgroup; the contour pixels of a
//                          chunk (a handful per wave) are compacted through ballots into an LDS queue in pixel order and worked off
//                          256 at a time, so the float64 work runs on full waves.  Float64 per point and per lane, summed across
//                          lanes (block_sum.h) and, in the solve kernel, workgroups in a fixed order: no atomics, the queue order
//                          is positional, a replay is bit-identical
//   gn_solve_kernel        (twist_solve.h) as the other Gauss-Newton stages; gn_solve_views_kernel for dim_sil_refine_views
// Two launches per iteration; nothing allocates or synchronises, so the stage is graph-capturable.
#include "common.h"
#include "twist_solve.h"

namespace dim {

constexpr int kSilMaxRadius = 64;
constexpr int kSilMaxSide = 32767;   // a coordinate takes 16 bits of a field word and of a queue entry
constexpr int kSilTileY = 32;        // rows per pass-1 tile

struct SilMaskFg {   // a NaN is background
  __device__ __forceinline__ bool operator()(float m) const { return m >= 0.5f; }
};
struct SilDepthFg {
  __device__ __forceinline__ bool operator()(float d) const { return d > 0.f; }
};

// foreground with a background 4-neighbour inside the frame (a neighbour outside the frame counts as foreground)
template <class FG>
__device__ __forceinline__ bool sil_is_edge(const float* __restrict__ p, int x, int y, int H, int W, FG fg) {
  const long o = (long)y * W + x;
  if (!fg(p[o])) return false;
  return (x > 0 && !fg(p[o - 1])) || (x + 1 < W && !fg(p[o + 1])) || (y > 0 && !fg(p[o - W])) || (y + 1 < H && !fg(p[o + W]));
}

__global__ __launch_bounds__(256) void sil_column_kernel(const float* __restrict__ mask, int H, int W, int radius, int* __restrict__ field) {
  __shared__ unsigned char flag[(kSilTileY + 2 * kSilMaxRadius) * 64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + tx, y0 = blockIdx.y * kSilTileY, b = blockIdx.z;
  const float* m = mask + (long)b * H * W;
  const int rows = kSilTileY + 2 * radius;   // LDS row j is image row y0 - radius + j
  for (int j = ty; j < rows; j += 4) {
    const int y = y0 - radius + j;
    flag[j * 64 + tx] = (x < W && y >= 0 && y < H && sil_is_edge(m, x, y, H, W, SilMaskFg())) ? 1 : 0;
  }
  __syncthreads();
  if (x >= W) return;
  for (int k = ty; k < kSilTileY; k += 4) {
    const int y = y0 + k;
    if (y >= H) break;
    const int j = k + radius;
    int ey = -1;
    for (int dy = 0; dy <= radius; ++dy) {   // the row above first: the smaller row wins a tie
      if (flag[(j - dy) * 64 + tx]) {
        ey = y - dy;
        break;
      }
      if (flag[(j + dy) * 64 + tx]) {
        ey = y + dy;
        break;
      }
    }
    field[((long)b * H + y) * W + x] = ey;
  }
}

__global__ __launch_bounds__(256) void sil_row_kernel(int H, int W, int radius, int* __restrict__ field) {
  extern __shared__ short sil_row[];   // W entries: the nearest edge row of every column of this row, -1 = none
  const int y = blockIdx.x, b = blockIdx.y;
  int* f = field + ((long)b * H + y) * W;
  for (int x = threadIdx.x; x < W; x += 256) sil_row[x] = (short)f[x];
  __syncthreads();
  const int r2 = radius * radius;
  for (int x = threadIdx.x; x < W; x += 256) {
    const int lo = max(x - radius, 0), hi = min(x + radius, W - 1);
    int best = r2 + 1, out = -1;
    for (int xe = lo; xe <= hi; ++xe) {   // upwards: the smaller column wins a tie
      const int ey = sil_row[xe];
      if (ey < 0) continue;
      const int dx = xe - x, dy = ey - y;
      const int d2 = dx * dx + dy * dy;
      if (d2 < best) {
        best = d2;
        out = (ey << 16) | xe;
      }
    }
    f[x] = out;
  }
}

__global__ __launch_bounds__(256) void sil_accumulate_kernel(const float* __restrict__ depth_r, const int* __restrict__ field,
                                                             const int* __restrict__ bbox, PinholeCam k9,
                                                             const float* __restrict__ K_per_sample, int H, int W, int it, float huber_px,
                                                             float max_px, const double* __restrict__ state, double* __restrict__ partial) {
  __shared__ int queue[512];   // contour pixels (y << 16 | x) waiting for a full pass: fewer than 256 left over plus one chunk
  __shared__ int wave_n[4];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
  const PinholeCam c = cam_pick(K_per_sample, k9, b);
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy;
  double R[9], t[3];
  gn_load_pose(state, b, it, R, t);
  const PixelBox box = clamp_bbox(bbox, b, H, W);
  const int bw = box.x1 - box.x0 + 1, bh = box.y1 - box.y0 + 1;
  const long n = (cam_ok(c) && bw > 0 && bh > 0) ? (long)bw * bh : 0;
  const long plane = (long)H * W;
  const float* dr = depth_r + (long)b * plane;
  const int* fl = field + (long)b * plane;
  const double hub = huber_px, gate = max_px;
  double acc[kGnTerms];
#pragma unroll
  for (int k = 0; k < kGnTerms; ++k) acc[k] = 0.0;

  auto point = [&](int packed) {
    const int x = packed & 0xFFFF, y = packed >> 16;
    const double z = dr[(long)y * W + x];
    const double sx = z * ((double)x - cx) / fx, sy = z * ((double)y - cy) / fy;
    const double mx = R[0] * sx + R[1] * sy + R[2] * z + t[0];
    const double my = R[3] * sx + R[4] * sy + R[5] * z + t[1];
    const double mz = R[6] * sx + R[7] * sy + R[8] * z + t[2];
    if (!(mz > 0.0)) return;
    const double u = fx * mx / mz + cx, v = fy * my / mz + cy;
    const double uf = floor(u + 0.5), vf = floor(v + 0.5);
    if (!(uf >= 0.0 && uf <= (double)(W - 1) && vf >= 0.0 && vf <= (double)(H - 1))) return;   // (a NaN fails too)
    const int f = fl[(long)(int)vf * W + (int)uf];
    if (f < 0) return;
    const double rx = u - (double)(f & 0xFFFF), ry = v - (double)(f >> 16);
    const double e2 = rx * rx + ry * ry;
    const double e = sqrt(e2);
    if (!(e <= gate)) return;   // w = 0
    double w = 1.0;
    if (!(e <= hub)) w = hub / e;
    gn_add_pixel(acc, fx, fy, mx, my, mz, rx, ry, w, e2);
  };

  int count = 0;   // queue length: the same in every lane
  for (long base = (long)blockIdx.x * 256; base < n; base += (long)kGnBlocks * 256) {   // the same trip count in every lane
    const long i = base + tid;
    bool on = false;
    int packed = 0;
    if (i < n) {
      const int qy = (int)(i / bw);
      const int y = box.y0 + qy, x = box.x0 + (int)(i - (long)qy * bw);
      on = sil_is_edge(dr, x, y, H, W, SilDepthFg());
      packed = (y << 16) | x;
    }
    const unsigned long long m = __ballot(on);
    const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if ((tid & 63) == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int off = count, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int nw = wave_n[w];
      if (w < wave) off += nw;
      total += nw;
    }
    if (on) queue[off + before] = packed;   // off + before < count + total <= 255 + 256
    count += total;
    __syncthreads();
    if (count >= 256) {
      point(queue[tid]);
      const int rest = count - 256;
      const int keep = tid < rest ? queue[256 + tid] : 0;
      __syncthreads();
      if (tid < rest) queue[tid] = keep;
      count = rest;
      __syncthreads();
    }
  }
  if (tid < count) point(queue[tid]);
  gn_store_partial(acc, partial, b);
}

}  // namespace dim

using namespace dim;

extern "C" int dim_sil_edge_field(const float* mask, int B, int H, int W, int radius, int* field, void* stream) {
  DIM_REQUIRE(B > 0, "sil_edge_field: B = %d", B);
  DIM_REQUIRE(radius >= 1 && radius <= kSilMaxRadius, "sil_edge_field: radius = %d (1 .. %d)", radius, kSilMaxRadius);
  DIM_REQUIRE(H >= 3 && W >= 3 && H <= kSilMaxSide && W <= kSilMaxSide, "sil_edge_field: image %d x %d (3 .. %d)", H, W, kSilMaxSide);
  DIM_REQUIRE(B <= 65535 && ceil_div(H, kSilTileY) <= 65535, "sil_edge_field: B = %d", B);
  DIM_REQUIRE(mask && field, "sil_edge_field: null pointer");
  hipLaunchKernelGGL(sil_column_kernel, dim3(ceil_div(W, 64), ceil_div(H, kSilTileY), B), dim3(256), 0, as_stream(stream), mask, H, W, radius,
                     field);
  hipLaunchKernelGGL(sil_row_kernel, dim3(H, B), dim3(256), (size_t)((W + 1) & ~1) * sizeof(short), as_stream(stream), H, W, radius, field);
  return check_launch("sil_edge_field");
}

extern "C" long dim_sil_workspace_bytes(int B, int H, int W) {
  (void)H;
  (void)W;
  return gn_workspace_bytes(B);
}

// both entries: views == nullptr is dim_sil_refine
static int sil_run(const float* depth_rendered, const int* field, const int* bbox, const float* pose_in, const float* K9,
                   const float* K_per_sample, int B, int H, int W, int iters, float huber_px, float max_px, void* workspace,
                   float* pose_out, float* stats, int* status, const GnViews* views, void* stream) {
  DIM_REQUIRE(B > 0 && B <= 65535, "sil_refine: B = %d", B);
  DIM_REQUIRE(iters >= 0, "sil_refine: iters = %d", iters);
  DIM_REQUIRE(huber_px > 0.f, "sil_refine: huber_px must be > 0");
  DIM_REQUIRE(max_px >= huber_px, "sil_refine: max_px must be >= huber_px");
  DIM_REQUIRE(H >= 3 && W >= 3 && H <= kSilMaxSide && W <= kSilMaxSide, "sil_refine: image %d x %d (3 .. %d)", H, W, kSilMaxSide);
  DIM_REQUIRE(depth_rendered && field && pose_in && K9 && workspace && pose_out, "sil_refine: null pointer");
  DIM_REQUIRE(!views || gn_views_ok(*views, B), "sil_refine_views: V in 1 .. %d dividing B = %d, cam_T_rig, pose_rig_in and pose_rig_out required",
              kGnMaxViews, B);
  if (iters == 0) {
    const int rc = dim_copy_words(pose_out, pose_in, 12L * B, stream);
    return (rc != DIM_OK || !views) ? rc : dim_copy_words(views->pose_rig_out, views->pose_rig_in, 12L * (B / views->V), stream);
  }
  const PinholeCam k9 = cam_of_k9(K9);
  const GnWorkspace ws(workspace, B);
  gn_iterate_either<DIM_STATUS_SIL_FEW_POINTS>(ws, (double*)((char*)workspace + gn_workspace_bytes(B)), B, views, iters, pose_in, pose_out,
                                               stats, status, as_stream(stream), [&](int it) {
    hipLaunchKernelGGL(sil_accumulate_kernel, dim3(kGnBlocks, B), dim3(256), 0, as_stream(stream), depth_rendered, field, bbox, k9,
                       K_per_sample, H, W, it, huber_px, max_px, (const double*)ws.state, ws.partial);
  });
  return check_launch(views ? "sil_refine_views" : "sil_refine");
}

extern "C" int dim_sil_refine(const float* depth_rendered, const int* field, const int* bbox, const float* pose_in, const float* K9,
                              const float* K_per_sample, int B, int H, int W, int iters, float huber_px, float max_px, void* workspace,
                              float* pose_out, float* stats, int* status, void* stream) {
  return sil_run(depth_rendered, field, bbox, pose_in, K9, K_per_sample, B, H, W, iters, huber_px, max_px, workspace, pose_out, stats, status,
                 nullptr, stream);
}

extern "C" long dim_sil_views_workspace_bytes(int B, int H, int W, int V) {
  (void)H;
  (void)W;
  return (B <= 0 || V <= 0) ? 0 : gn_workspace_bytes(B) + gn_views_state_bytes(B, V);
}

extern "C" int dim_sil_refine_views(const float* depth_rendered, const int* field, const int* bbox, const float* pose_in, const float* K9,
                                    const float* K_per_sample, int B, int H, int W, int iters, float huber_px, float max_px,
                                    void* workspace, float* pose_out, float* stats, int* status, const float* cam_T_rig, int V,
                                    const float* pose_rig_in, float* pose_rig_out, float* stats_group, void* stream) {
  const GnViews views{cam_T_rig, V, pose_rig_in, pose_rig_out, stats_group};
  return sil_run(depth_rendered, field, bbox, pose_in, K9, K_per_sample, B, H, W, iters, huber_px, max_px, workspace, pose_out, stats, status,
                 &views, stream);
}
