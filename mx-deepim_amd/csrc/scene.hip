// Multi-object scene composition on the device: S single-object renders (the layers the rasteriser returns) -> one occluded scene
// with labels, per-layer visibility masks, pixel counts and boxes.  Stands in for the offline scene generation of
// toolkit/LM6d_occ_dsm_1_gen_observed_light.py:164-238 (render every object alone, paste them together, label) and the
// visibility count of toolkit/LM6d_occ_dsm_3_remove_low_visible.py.
//
// Per-pixel rule: the winner is the used layer (label > 0) with the smallest depth that is finite and > 0; equal depths go to the lower
// slot; no candidate = background (colour 0, depth 0, label 0).
//
// Deviation from the reference: it paints WHOLE objects one over the other in order of their mean depth (:219-236) -- and that order
// is scrambled there by indexing a reversed array with the argsort of its reverse.  The per-pixel depth test here is what that code
// approximates; the two agree whenever the objects do not interpenetrate and the order is the intended far-to-near one.
//
// Streaming kernel, one thread per four consecutive pixels (one pixel when W % 4 != 0 or a plane is not 16-byte aligned): all S depth
// loads are issued before the first is used (the loop is unrolled to a compile-time bound, a layer's load is skipped by a
// wave-uniform test), then only the winner's colour is fetched.  Counts and boxes: ballots / LDS integer min-max inside the
// workgroup, one row of plain stores per workgroup into the workspace, and a second small kernel that folds the rows -- integer
// sums and extrema, so the result does not depend on any order, and nothing is read that this call did not write.
#include "common.h"

namespace dim {

constexpr int kSceneMaxLayers = 16;
constexpr int kScenePart = 6;   // ints per (workgroup, layer) row: full, visible, min x, max x, min y, max y

template <int SMAX, bool VEC>
__global__ __launch_bounds__(256) void scene_compose_kernel(const float* __restrict__ layer_bgr, const float* __restrict__ layer_depth,
                                                            const int* __restrict__ layer_label, int S, int H, int W,
                                                            float* __restrict__ scene_bgr, float* __restrict__ scene_depth,
                                                            float* __restrict__ scene_label, float* __restrict__ vis_mask,
                                                            int* __restrict__ part) {
  constexpr int PX = VEC ? 4 : 1;
  typedef float v4f __attribute__((ext_vector_type(4)));
  const int n = blockIdx.y;
  const long plane = (long)H * W;
  const long pix = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PX;   // first pixel of this thread inside the scene
  const bool live = pix < plane;                                         // (VEC: plane % 4 == 0, so a live quad is whole)
  __shared__ int s_cnt[4][kSceneMaxLayers][2];
  __shared__ int s_box[kSceneMaxLayers][4];
  if (part && threadIdx.x < kSceneMaxLayers) {
    s_box[threadIdx.x][0] = 0x7FFFFFFF; s_box[threadIdx.x][1] = -1; s_box[threadIdx.x][2] = 0x7FFFFFFF; s_box[threadIdx.x][3] = -1;
  }
  // ---- all depth loads first (labels are wave-uniform: scalar loads, and an unused layer costs no vector load)
  int lab[SMAX];
  float d[SMAX][PX];
#pragma unroll
  for (int s = 0; s < SMAX; ++s) {
    lab[s] = s < S ? layer_label[n * S + s] : 0;
#pragma unroll
    for (int k = 0; k < PX; ++k) d[s][k] = 0.f;
    if (lab[s] > 0 && live) {
      const float* p = layer_depth + ((long)n * S + s) * plane + pix;
      if (VEC) {
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
        d[s][0] = v.x; d[s][1 % PX] = v.y; d[s][2 % PX] = v.z; d[s][3 % PX] = v.w;
      } else {
        d[s][0] = __builtin_nontemporal_load(p);
      }
    }
  }
  // ---- depth test: ascending slots, strict <, so a tie stays with the lower slot; NaN, inf, 0 and negatives never qualify
  float best[PX];
  int win[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) { best[k] = __builtin_inff(); win[k] = -1; }
#pragma unroll
  for (int s = 0; s < SMAX; ++s)
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const float v = d[s][k];
      if (v > 0.f && v < best[k]) { best[k] = v; win[k] = s; }   // (v < inf on the first hit: finite)
    }
  if (live) {
    // ---- the winner's colour only
    if (scene_bgr) {
      float c[PX * 3];
      bool same = VEC && win[0] >= 0;
#pragma unroll
      for (int k = 1; k < PX; ++k) same = same && win[k] == win[0];
      if (same) {   // one layer owns the quad (the common case inside an object): three 16-byte loads
        const v4f* p = reinterpret_cast<const v4f*>(layer_bgr + (((long)n * S + win[0]) * plane + pix) * 3);
        const v4f a = p[0], b = p[1], e = p[2];
        const float t[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, e.x, e.y, e.z, e.w};
#pragma unroll
        for (int k = 0; k < PX * 3; ++k) c[k] = t[k % 12];
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          c[3 * k] = c[3 * k + 1] = c[3 * k + 2] = 0.f;
          if (win[k] >= 0) {
            const float* p = layer_bgr + (((long)n * S + win[k]) * plane + pix + k) * 3;
            c[3 * k] = p[0]; c[3 * k + 1] = p[1]; c[3 * k + 2] = p[2];
          }
        }
      }
      float* o = scene_bgr + ((long)n * plane + pix) * 3;
      if (VEC) {
        v4f* o4 = reinterpret_cast<v4f*>(o);
        __builtin_nontemporal_store((v4f){c[0], c[1 % (PX * 3)], c[2 % (PX * 3)], c[3 % (PX * 3)]}, o4);
        __builtin_nontemporal_store((v4f){c[4 % (PX * 3)], c[5 % (PX * 3)], c[6 % (PX * 3)], c[7 % (PX * 3)]}, o4 + 1);
        __builtin_nontemporal_store((v4f){c[8 % (PX * 3)], c[9 % (PX * 3)], c[10 % (PX * 3)], c[11 % (PX * 3)]}, o4 + 2);
      } else {
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
      }
    }
    float zd[PX], zl[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      zd[k] = win[k] >= 0 ? best[k] : 0.f;
      int l = 0;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) l = win[k] == s ? lab[s] : l;
      zl[k] = (float)l;
    }
    const long o = (long)n * plane + pix;
    if (VEC) {
      if (scene_depth) __builtin_nontemporal_store((v4f){zd[0], zd[1 % PX], zd[2 % PX], zd[3 % PX]}, reinterpret_cast<v4f*>(scene_depth + o));
      if (scene_label) __builtin_nontemporal_store((v4f){zl[0], zl[1 % PX], zl[2 % PX], zl[3 % PX]}, reinterpret_cast<v4f*>(scene_label + o));
    } else {
      if (scene_depth) scene_depth[o] = zd[0];
      if (scene_label) scene_label[o] = zl[0];
    }
    if (vis_mask) {   // every slot is written, the unused ones with zeros
#pragma unroll
      for (int s = 0; s < SMAX; ++s)
        if (s < S) {
          float* m = vis_mask + ((long)n * S + s) * plane + pix;
          if (VEC)
            __builtin_nontemporal_store((v4f){win[0] == s ? 1.f : 0.f, win[1 % PX] == s ? 1.f : 0.f, win[2 % PX] == s ? 1.f : 0.f,
                                              win[3 % PX] == s ? 1.f : 0.f}, reinterpret_cast<v4f*>(m));
          else
            m[0] = win[0] == s ? 1.f : 0.f;
        }
    }
  }
  if (!part) return;   // (kernel-uniform) no counts, boxes or status asked for
  // ---- counts: one ballot per layer and pixel of the quad, summed on the scalar side
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < SMAX; ++s)
    if (s < S) {
      int full = 0, vis = 0;
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        full += __popcll(__ballot(d[s][k] > 0.f));
        vis += __popcll(__ballot(win[k] == s));
      }
      if (lane == 0) { s_cnt[wave][s][0] = full; s_cnt[wave][s][1] = vis; }
    }
  __syncthreads();   // s_box initialised, s_cnt written
  // ---- boxes: a layer's visible pixels inside the quad are runs; a run's first pixel bounds min x, its last max x (a quad never
  // crosses a row: W % 4 == 0 on this path)
  if (live) {
    const int y = (int)(pix / W), x0 = (int)(pix - (long)y * W);
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (win[k] < 0) continue;
      if (k == 0 || win[k] != win[k > 0 ? k - 1 : 0]) {
        atomicMin(&s_box[win[k]][0], x0 + k);
        atomicMin(&s_box[win[k]][2], y);
        atomicMax(&s_box[win[k]][3], y);
      }
      if (k == PX - 1 || win[k] != win[k < PX - 1 ? k + 1 : k]) atomicMax(&s_box[win[k]][1], x0 + k);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < S) {
    const int s = threadIdx.x;
    int* r = part + (((long)n * gridDim.x + blockIdx.x) * S + s) * kScenePart;
    r[0] = s_cnt[0][s][0] + s_cnt[1][s][0] + s_cnt[2][s][0] + s_cnt[3][s][0];
    r[1] = s_cnt[0][s][1] + s_cnt[1][s][1] + s_cnt[2][s][1] + s_cnt[3][s][1];
    r[2] = s_box[s][0]; r[3] = s_box[s][1]; r[4] = s_box[s][2]; r[5] = s_box[s][3];
  }
}

// one wave per (scene, layer): folds the workgroup rows.  Box in dim_mask_bbox's convention, empty = {W, -1, H, -1}.
__global__ __launch_bounds__(64) void scene_fold_kernel(const int* __restrict__ part, const int* __restrict__ layer_label, int nblk, int S,
                                                        int H, int W, int* __restrict__ counts, int* __restrict__ vis_bbox,
                                                        int* __restrict__ status) {
  const int ns = blockIdx.x, n = ns / S, s = ns - n * S;
  int full = 0, vis = 0, lo = 0x7FFFFFFF, hi = -1, ylo = 0x7FFFFFFF, yhi = -1;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    const int* r = part + (((long)n * nblk + i) * S + s) * kScenePart;
    full += r[0]; vis += r[1];
    lo = min(lo, r[2]); hi = max(hi, r[3]); ylo = min(ylo, r[4]); yhi = max(yhi, r[5]);
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    full += __shfl_xor(full, dlt);
    vis += __shfl_xor(vis, dlt);
    lo = min(lo, __shfl_xor(lo, dlt));
    hi = max(hi, __shfl_xor(hi, dlt));
    ylo = min(ylo, __shfl_xor(ylo, dlt));
    yhi = max(yhi, __shfl_xor(yhi, dlt));
  }
  if (threadIdx.x == 0) {
    if (counts) { counts[2 * ns] = full; counts[2 * ns + 1] = vis; }
    if (vis_bbox) { vis_bbox[4 * ns] = min(lo, W); vis_bbox[4 * ns + 1] = hi; vis_bbox[4 * ns + 2] = min(ylo, H); vis_bbox[4 * ns + 3] = yhi; }
    if (status && layer_label[ns] > 0 && vis == 0) atomicOr(status + ns, DIM_STATUS_LAYER_HIDDEN);
  }
}

}  // namespace dim

using namespace dim;

extern "C" {

// rows of the larger (one pixel per thread) launch
long dim_scene_compose_workspace_bytes(int N, int S, int H, int W) {
  if (N <= 0 || S <= 0 || H <= 0 || W <= 0) return 0;
  return (long)N * ceil_div((long)H * W, 256) * S * kScenePart * (long)sizeof(int);
}

int dim_scene_compose(const float* layer_bgr, const float* layer_depth, const int* layer_label, int N, int S, int H, int W,
                      void* workspace, float* scene_bgr, float* scene_depth, float* scene_label, float* vis_mask, int* counts,
                      int* vis_bbox, int* status, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(S >= 1 && S <= kSceneMaxLayers, "scene_compose: S must be in [1, %d], got %d", kSceneMaxLayers, S);
  DIM_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "scene_compose: bad sizes");
  DIM_REQUIRE(layer_depth && layer_label, "scene_compose: null pointer (layer_depth, layer_label)");
  DIM_REQUIRE(!scene_bgr || layer_bgr, "scene_compose: scene_bgr needs layer_bgr");
  const bool fold = counts || vis_bbox || status;
  DIM_REQUIRE(!fold || workspace, "scene_compose: counts / vis_bbox / status need the workspace");
  DIM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "scene_compose: workspace must be 4-byte aligned");
  hipStream_t st = as_stream(stream);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = W % 4 == 0 && al16(layer_bgr) && al16(layer_depth) && al16(scene_bgr) && al16(scene_depth) && al16(scene_label) &&
                   al16(vis_mask);
  int* part = fold ? reinterpret_cast<int*>(workspace) : nullptr;
  const long plane = (long)H * W;
  const int nblk = ceil_div(vec ? plane / 4 : plane, 256);
#define DIM_SCENE_LAUNCH(SMAX, VEC)                                                                                              \
  hipLaunchKernelGGL((scene_compose_kernel<SMAX, VEC>), dim3(nblk, N), dim3(256), 0, st, layer_bgr, layer_depth, layer_label, S, H, W, \
                     scene_bgr, scene_depth, scene_label, vis_mask, part)
  if (!vec) DIM_SCENE_LAUNCH(16, false);
  else if (S <= 2) DIM_SCENE_LAUNCH(2, true);
  else if (S <= 4) DIM_SCENE_LAUNCH(4, true);
  else if (S <= 8) DIM_SCENE_LAUNCH(8, true);
  else DIM_SCENE_LAUNCH(16, true);
#undef DIM_SCENE_LAUNCH
  if (fold)
    hipLaunchKernelGGL(scene_fold_kernel, dim3(N * S), dim3(64), 0, st, part, layer_label, nblk, S, H, W, counts, vis_bbox, status);
  return check_launch("scene_compose");
}

}  // extern "C"
