// Colour-histogram segmentation of the tracks: a mask per track and frame from per-track foreground / background colour histograms
// that are carried from frame to frame.  The rule stands in deepim_hip.h; tests/track_seg_reference.py restates it in numpy.
//   dim_track_seg_mask   seg_lut_kernel        per track: one bit per colour bin, "foreground histogram > background histogram", and the
//                                              track's header words (region, has-model, counts[0], counts[1] = 0, the status bit)
//                        seg_mask_kernel       one block per 64 x 16 pixel tile and track: the raw bits of the tile and its halo into
//                                              LDS (a frame pixel -> its bin -> its bit), the integer majority filter, one 16-byte
//                                              store per lane; a tile outside the region stores zeros and reads nothing
//                        (counts[1] is summed with one integer atomicAdd per wave)
//   dim_track_seg_learn  seg_clear_kernel      zeroes the bin counters and {n_f, n_b}
//                        seg_count_kernel      kSegBands blocks per track over the rows of its region: 4 pixels per lane (two 16-byte
//                                              depth loads, 12 bytes of colour), one counter increment per classified pixel
//                        seg_blend_kernel      one lane per bin: count / n, first update or blend
//                        seg_finish_kernel     one lane per track: counts out, seg_age
// Where the counters live.  Both histograms at bits = 5 are 2 x 32768 words = 256 KiB per track: more than the 160 KiB of LDS, and one
// of them alone (128 KiB) would leave one block per CU that clears and flushes 32768 words for a band of a few hundred pixels.  So the
// split is by the number of bins, not by class: up to bits = 3 (2 x 512 words = 4 KiB) a block counts into an LDS sub-histogram and
// flushes its non-zero words with global atomics -- few bins, so global atomics alone would pile onto a handful of addresses --; from
// bits = 4 on (2 x 4096 words and more) the lanes add to the global counters directly, after the lanes of a wave that hold the bin of
// its first live lane have been merged into one add (a textureless object puts most of a wave into one bin; a textured one spreads
// over many addresses by itself).  Integer adds: the sums do not depend on the order, and a replay gives the same bits.
// Nothing allocates or synchronises: every entry is graph-capturable, and no memset node is used.
#include "common.h"

namespace dim {

constexpr int kSegThreads = 256;
constexpr int kSegTileW = 64, kSegTileH = 16;   // 256 lanes x 4 pixels
constexpr int kSegMaxRadius = 4;
constexpr int kSegLdsW = kSegTileW + 2 * kSegMaxRadius, kSegLdsH = kSegTileH + 2 * kSegMaxRadius;
constexpr int kSegBands = 64;            // blocks per track of the counting kernel
constexpr int kSegLdsBits = 3;           // up to here the counters of a block live in LDS
constexpr int kSegHeadWords = 8;         // per track: {x0, x1, y0, y1, has model, -, -, -}

struct SegRegion {
  int x0, x1, y0, y1;   // inclusive; x1 < x0: none
};

__device__ __forceinline__ SegRegion seg_region(const int* bbox, int margin, int H, int W) {
  SegRegion r = {0, -1, 0, -1};
  const long bx0 = bbox[0], bx1 = bbox[1], by0 = bbox[2], by1 = bbox[3];
  if (bx1 < bx0 || by1 < by0) return r;
  const long x0 = max(bx0 - margin, 0L), x1 = min(bx1 + margin, (long)W - 1);
  const long y0 = max(by0 - margin, 0L), y1 = min(by1 + margin, (long)H - 1);
  if (x1 < x0 || y1 < y0) return r;
  r.x0 = (int)x0; r.x1 = (int)x1; r.y0 = (int)y0; r.y1 = (int)y1;
  return r;
}

__device__ __forceinline__ int seg_bin(unsigned b, unsigned g, unsigned r, int bits) {
  const int s = 8 - bits;
  return (int)(((b >> s) << (2 * bits)) | ((g >> s) << bits) | (r >> s));
}

__device__ __forceinline__ bool seg_drawn(float d) { return d > 0.f && d < INFINITY; }

// ---------------------------------------------------------------------------------------------------- the mask
// grid (ceil(NB / 256), P): lane -> one bin; a wave's 64 comparisons leave as two words of the track's bit table
__global__ __launch_bounds__(kSegThreads) void seg_lut_kernel(const float* __restrict__ seg_hist, const int* __restrict__ seg_age,
                                                              const int* __restrict__ bbox, int H, int W, int NB, int lut_words,
                                                              int margin, unsigned* __restrict__ lut, int* __restrict__ head,
                                                              int* __restrict__ counts, int* __restrict__ status) {
  const int p = blockIdx.y;
  const int c = blockIdx.x * kSegThreads + threadIdx.x;
  bool fg = false;
  if (c < NB) fg = seg_hist[((long)p * 2) * NB + c] > seg_hist[((long)p * 2 + 1) * NB + c];
  const unsigned long long bits = __ballot(fg);
  const int lane = threadIdx.x % kWave;
  const int word = (c - lane) / 32;   // the wave's first word; NB < 64 (bits = 1): only word 0 exists
  if (lane == 0 && word < lut_words) lut[(long)p * lut_words + word] = (unsigned)bits;
  if (lane == 32 && word + 1 < lut_words) lut[(long)p * lut_words + word + 1] = (unsigned)(bits >> 32);
  if (c == 0) {
    const SegRegion r = seg_region(bbox + 4L * p, margin, H, W);
    const bool region = r.x1 >= r.x0, model = region && seg_age[p] > 0;
    int* h = head + (long)kSegHeadWords * p;
    h[0] = r.x0; h[1] = r.x1; h[2] = r.y0; h[3] = r.y1;
    h[4] = model ? 1 : 0;
    counts[2 * p] = region ? (r.x1 - r.x0 + 1) * (r.y1 - r.y0 + 1) : 0;
    counts[2 * p + 1] = 0;
    if (status && !model) status[p] |= DIM_STATUS_TRACK_SEG_NO_MODEL;
  }
}

// grid (ceil(W / 64), ceil(H / 16), P).  VEC: W % 4 == 0 and mask 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kSegThreads) void seg_mask_kernel(const unsigned char* __restrict__ frame_bgr, const unsigned* __restrict__ lut,
                                                               const int* __restrict__ head, int H, int W, int bits, int lut_words,
                                                               int radius, float* __restrict__ mask, int* __restrict__ counts) {
  __shared__ unsigned char raw[kSegLdsH * kSegLdsW];
  const int p = blockIdx.z;
  const int* h = head + (long)kSegHeadWords * p;
  const int rx0 = h[0], rx1 = h[1], ry0 = h[2], ry1 = h[3];
  const int tx0 = blockIdx.x * kSegTileW, ty0 = blockIdx.y * kSegTileH;
  const int lx = 4 * (threadIdx.x % (kSegTileW / 4)), ly = threadIdx.x / (kSegTileW / 4);
  const int x = tx0 + lx, y = ty0 + ly;
  float* dst = mask + ((long)p * H + y) * W + x;
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  // block-uniform: the tile meets the region of a track with a model
  const bool live = h[4] != 0 && tx0 <= rx1 && tx0 + kSegTileW - 1 >= rx0 && ty0 <= ry1 && ty0 + kSegTileH - 1 >= ry0;
  int n = 0;
  if (live) {
    const int tw = kSegTileW + 2 * radius, th = kSegTileH + 2 * radius;
    const unsigned* bit = lut + (long)p * lut_words;
    for (int i = threadIdx.x; i < tw * th; i += kSegThreads) {
      const int hy = i / tw, hx = i - hy * tw;
      const int gx = tx0 - radius + hx, gy = ty0 - radius + hy;
      unsigned char v = 0;
      if (gx >= rx0 && gx <= rx1 && gy >= ry0 && gy <= ry1) {   // inside the region: inside the frame
        const unsigned char* px = frame_bgr + ((long)gy * W + gx) * 3;
        const int c = seg_bin(px[0], px[1], px[2], bits);
        v = (unsigned char)((bit[c >> 5] >> (c & 31)) & 1u);
      }
      raw[hy * kSegLdsW + hx] = v;
    }
    __syncthreads();
    const int need = (2 * radius + 1) * (2 * radius + 1);
    if (y >= ry0 && y <= ry1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x + j < rx0 || x + j > rx1) continue;
        int sum = 0;
        for (int dy = 0; dy <= 2 * radius; ++dy)
          for (int dx = 0; dx <= 2 * radius; ++dx) sum += raw[(ly + dy) * kSegLdsW + lx + j + dx];
        if (2 * sum > need) {
          out[j] = 1.f;
          ++n;
        }
      }
    }
  }
  if (y < H) {
    if (VEC) {
      if (x < W) *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1], out[2], out[3]);   // W % 4 == 0: four whole pixels
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < W) dst[j] = out[j];
    }
  }
  if (live) {   // block-uniform: every lane of the wave takes part
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s, 64);
    if (threadIdx.x % kWave == 0 && n > 0) atomicAdd(counts + 2 * p + 1, n);
  }
}

// ---------------------------------------------------------------------------------------------------- the histograms
__global__ __launch_bounds__(kSegThreads) void seg_clear_kernel(unsigned* __restrict__ words, long n) {
  const long i = 4 * ((long)blockIdx.x * kSegThreads + threadIdx.x);
  if (i < n) *reinterpret_cast<uint4*>(words + i) = make_uint4(0u, 0u, 0u, 0u);   // n % 4 == 0, 16-byte aligned
}

// one add of `one` into dst[key] per lane with key >= 0; the lanes that hold the key of the wave's first live lane become one add.
// Every lane of the wave must call it.
__device__ __forceinline__ void seg_add_merged(unsigned* dst, int key) {
  const unsigned long long live = __ballot(key >= 0);
  if (live == 0) return;   // wave-uniform
  const int src = __ffsll((long long)live) - 1;
  const int lead = __shfl(key, src, 64);
  const unsigned long long same = __ballot(key == lead);
  if ((int)(threadIdx.x % kWave) == src) atomicAdd(dst + lead, (unsigned)__popcll(same));
  else if (key >= 0 && key != lead) atomicAdd(dst + key, 1u);
}

// grid (kSegBands, P).  V pixels per lane: 4 (W % 4 == 0, depth planes 16-byte and the frame 4-byte aligned) or 1.  LDS: the block's
// own counters (bits <= kSegLdsBits).  bins (P,2,NB) and nfb (P,2) are the zeroed global counters
template <int V, bool LDS>
__global__ __launch_bounds__(kSegThreads) void seg_count_kernel(const unsigned char* __restrict__ frame_bgr,
                                                                const float* __restrict__ depth_drawn, const float* __restrict__ depth_fg,
                                                                const int* __restrict__ bbox, int H, int W, int bits, int NB, int margin,
                                                                unsigned* __restrict__ bins, unsigned* __restrict__ nfb) {
  __shared__ unsigned sub[LDS ? 2 << (3 * kSegLdsBits) : 1];
  const int p = blockIdx.y;
  const SegRegion r = seg_region(bbox + 4L * p, margin, H, W);
  if (r.x1 < r.x0) return;   // block-uniform
  const int rows = r.y1 - r.y0 + 1, per = (rows + kSegBands - 1) / kSegBands;
  const int yb0 = r.y0 + (int)blockIdx.x * per, yb1 = min(yb0 + per - 1, r.y1);
  if (yb0 > yb1) return;     // block-uniform
  if (LDS) {
    for (int i = threadIdx.x; i < 2 * NB; i += kSegThreads) sub[i] = 0u;
    __syncthreads();
  }
  const int xa = V == 4 ? (r.x0 & ~3) : r.x0;
  const int units = (r.x1 - xa) / V + 1;
  const int total = units * (yb1 - yb0 + 1);
  const long plane = (long)H * W;
  const float* drawn_p = depth_drawn + (long)p * plane;
  const float* fg_p = depth_fg ? depth_fg + (long)p * plane : nullptr;
  unsigned* dst = LDS ? sub : bins + (long)p * 2 * NB;
  unsigned nf = 0, nb = 0;
  for (int i0 = 0; i0 < total; i0 += kSegThreads) {   // the trip count is block-uniform: every lane reaches the ballots
    const int i = i0 + threadIdx.x;
    int key[V];
#pragma unroll
    for (int j = 0; j < V; ++j) key[j] = -1;
    if (i < total) {
      const int row = i / units, x = xa + (i - row * units) * V, y = yb0 + row;
      const long pix = (long)y * W + x;
      float dd[V], df[V];
      unsigned char col[V][3];
      if (V == 4) {   // x % 4 == 0 and W % 4 == 0: four whole pixels of the frame
        const float4 q = *reinterpret_cast<const float4*>(drawn_p + pix);
        dd[0] = q.x; dd[1 % V] = q.y; dd[2 % V] = q.z; dd[3 % V] = q.w;
        if (fg_p) {
          const float4 f = *reinterpret_cast<const float4*>(fg_p + pix);
          df[0] = f.x; df[1 % V] = f.y; df[2 % V] = f.z; df[3 % V] = f.w;
        }
        const uint3 c3 = *reinterpret_cast<const uint3*>(frame_bgr + pix * 3);   // 12 bytes = 4 pixels x (B, G, R)
        const unsigned w[3] = {c3.x, c3.y, c3.z};
#pragma unroll
        for (int k = 0; k < 12; ++k) col[(k / 3) % V][k % 3] = (unsigned char)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
      } else {
        dd[0] = drawn_p[pix];
        if (fg_p) df[0] = fg_p[pix];
        for (int k = 0; k < 3; ++k) col[0][k] = frame_bgr[pix * 3 + k];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (x + j < r.x0 || x + j > r.x1) continue;
        const bool fore = seg_drawn(fg_p ? df[j] : dd[j]);
        const bool back = !fore && !seg_drawn(dd[j]);
        if (!fore && !back) continue;   // drawn but hidden
        key[j] = (fore ? 0 : NB) + seg_bin(col[j][0], col[j][1], col[j][2], bits);
        nf += fore ? 1u : 0u;
        nb += back ? 1u : 0u;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (LDS) {
        if (key[j] >= 0) atomicAdd(dst + key[j], 1u);
      } else {
        seg_add_merged(dst, key[j]);
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    nf += __shfl_xor(nf, s, 64);
    nb += __shfl_xor(nb, s, 64);
  }
  if (threadIdx.x % kWave == 0) {
    if (nf) atomicAdd(nfb + 2 * p, nf);
    if (nb) atomicAdd(nfb + 2 * p + 1, nb);
  }
  if (LDS) {
    __syncthreads();
    unsigned* g = bins + (long)p * 2 * NB;
    for (int i = threadIdx.x; i < 2 * NB; i += kSegThreads)
      if (sub[i]) atomicAdd(g + i, sub[i]);
  }
}

__device__ __forceinline__ bool seg_skipped(const unsigned* nfb, const int* flags, int skip_mask, int min_pixels, int p) {
  if (flags && (flags[p] & skip_mask) != 0) return true;
  return nfb[2 * p] < (unsigned)min_pixels || nfb[2 * p + 1] < (unsigned)min_pixels;
}

// grid (ceil(2 NB / 256), P): lane -> one word of the track's two histograms.  Reads seg_age, which seg_finish_kernel writes afterwards
__global__ __launch_bounds__(kSegThreads) void seg_blend_kernel(const unsigned* __restrict__ bins, const unsigned* __restrict__ nfb,
                                                                const int* __restrict__ flags, int skip_mask, int min_pixels, int NB,
                                                                float rate, const int* __restrict__ seg_age, float* __restrict__ seg_hist) {
  const int p = blockIdx.y;
  const int i = blockIdx.x * kSegThreads + threadIdx.x;
  if (i >= 2 * NB || seg_skipped(nfb, flags, skip_mask, min_pixels, p)) return;
  const float n = (float)nfb[2 * p + (i >= NB ? 1 : 0)];
  const float h = __fdiv_rn((float)bins[(long)p * 2 * NB + i], n);
  float* dst = seg_hist + (long)p * 2 * NB + i;
  if (seg_age[p] <= 0) {
    *dst = h;
  } else {
    const float old = *dst;
    *dst = __fadd_rn(old, __fmul_rn(rate, __fsub_rn(h, old)));
  }
}

__global__ __launch_bounds__(64) void seg_finish_kernel(const unsigned* __restrict__ nfb, const int* __restrict__ flags, int skip_mask,
                                                        int min_pixels, int P, int* __restrict__ seg_age, int* __restrict__ counts) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  counts[2 * p] = (int)nfb[2 * p];
  counts[2 * p + 1] = (int)nfb[2 * p + 1];
  if (!seg_skipped(nfb, flags, skip_mask, min_pixels, p)) seg_age[p] = min(max(seg_age[p], 0) + 1, 1 << 30);
}

// the workspace: [mask: head (P,8) int32 | bit table (P,lut_words)] [learn: {n_f, n_b} (P,2) | bin counters (P,2,NB)], each part
// rounded up to 16 bytes
struct SegLayout {
  long lut_words, head_off, lut_off, nfb_off, bins_off, learn_words, total_words;
};

static long round4(long words) { return (words + 3) & ~3L; }

static SegLayout seg_layout(int P, int bits) {
  SegLayout s;
  const long NB = 1L << (3 * bits);
  s.lut_words = NB < 32 ? 1 : NB / 32;
  s.head_off = 0;
  s.lut_off = round4((long)P * kSegHeadWords);
  s.nfb_off = s.lut_off + round4((long)P * s.lut_words);
  s.bins_off = s.nfb_off + round4(2L * P);
  s.learn_words = round4(2L * P) + round4(2L * P * NB);
  s.total_words = s.nfb_off + s.learn_words;
  return s;
}

}  // namespace dim

using namespace dim;

static bool seg_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

#define SEG_REQUIRE_SHAPE(name)                                                                                                        \
  DIM_REQUIRE(P > 0 && P <= 65535 && H > 0 && W > 0 && (long)H * W <= (1L << 24), "%s: P = %d, H = %d, W = %d (H*W at most 1 << 24)", name, P, H, W); \
  DIM_REQUIRE(bits >= 1 && bits <= 5, "%s: bits = %d outside 1..5", name, bits);                                                       \
  DIM_REQUIRE(margin >= 0, "%s: margin = %d", name, margin)

extern "C" long dim_track_seg_workspace_bytes(int P, int H, int W, int bits) {
  if (P <= 0 || H <= 0 || W <= 0 || bits < 1 || bits > 5) return 0;
  return seg_layout(P, bits).total_words * (long)sizeof(unsigned);
}

extern "C" int dim_track_seg_mask(const unsigned char* frame_bgr, const int* bbox, const float* seg_hist, const int* seg_age, int P, int H,
                                  int W, int bits, int margin, int radius, void* workspace, float* mask, int* counts, int* status,
                                  void* stream) {
  SEG_REQUIRE_SHAPE("track_seg_mask");
  DIM_REQUIRE(radius >= 0 && radius <= kSegMaxRadius, "track_seg_mask: radius = %d outside 0..%d", radius, kSegMaxRadius);
  DIM_REQUIRE(frame_bgr && bbox && seg_hist && seg_age && workspace && mask && counts, "track_seg_mask: null pointer");
  DIM_REQUIRE(seg_aligned(bbox, 4) && seg_aligned(seg_hist, 4) && seg_aligned(seg_age, 4) && seg_aligned(mask, 4) && seg_aligned(counts, 4) &&
                  seg_aligned(status, 4) && seg_aligned(workspace, 16),
              "track_seg_mask: pointer alignment: float and int arrays 4 bytes, the workspace 16 bytes");
  const SegLayout s = seg_layout(P, bits);
  const int NB = 1 << (3 * bits);
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  int* head = reinterpret_cast<int*>(ws + s.head_off);
  unsigned* lut = ws + s.lut_off;
  hipLaunchKernelGGL(seg_lut_kernel, dim3(ceil_div(NB, kSegThreads), P), dim3(kSegThreads), 0, as_stream(stream), seg_hist, seg_age, bbox, H, W,
                     NB, (int)s.lut_words, margin, lut, head, counts, status);
  const dim3 grid(ceil_div(W, kSegTileW), ceil_div(H, kSegTileH), P);
  if (W % 4 == 0 && seg_aligned(mask, 16))
    hipLaunchKernelGGL(seg_mask_kernel<true>, grid, dim3(kSegThreads), 0, as_stream(stream), frame_bgr, (const unsigned*)lut,
                       (const int*)head, H, W, bits, (int)s.lut_words, radius, mask, counts);
  else
    hipLaunchKernelGGL(seg_mask_kernel<false>, grid, dim3(kSegThreads), 0, as_stream(stream), frame_bgr, (const unsigned*)lut,
                       (const int*)head, H, W, bits, (int)s.lut_words, radius, mask, counts);
  return check_launch("track_seg_mask");
}

extern "C" int dim_track_seg_learn(const unsigned char* frame_bgr, const float* depth_drawn, const float* depth_fg, const int* bbox,
                                   const int* flags, int skip_mask, int P, int H, int W, int bits, int margin, float rate, int min_pixels,
                                   void* workspace, float* seg_hist, int* seg_age, int* counts, void* stream) {
  SEG_REQUIRE_SHAPE("track_seg_learn");
  DIM_REQUIRE(rate >= 0.f && rate <= 1.f, "track_seg_learn: rate = %g outside [0, 1]", (double)rate);
  DIM_REQUIRE(min_pixels >= 1, "track_seg_learn: min_pixels = %d", min_pixels);
  DIM_REQUIRE(frame_bgr && depth_drawn && bbox && workspace && seg_hist && seg_age && counts, "track_seg_learn: null pointer");
  DIM_REQUIRE(seg_aligned(depth_drawn, 4) && seg_aligned(depth_fg, 4) && seg_aligned(bbox, 4) && seg_aligned(flags, 4) &&
                  seg_aligned(seg_hist, 4) && seg_aligned(seg_age, 4) && seg_aligned(counts, 4) && seg_aligned(workspace, 16),
              "track_seg_learn: pointer alignment: float and int arrays 4 bytes, the workspace 16 bytes");
  const SegLayout s = seg_layout(P, bits);
  const int NB = 1 << (3 * bits);
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  unsigned* nfb = ws + s.nfb_off;
  unsigned* bins = ws + s.bins_off;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(seg_clear_kernel, dim3(ceil_div(s.learn_words / 4, kSegThreads)), dim3(kSegThreads), 0, st, nfb, s.learn_words);
  const bool vec = W % 4 == 0 && seg_aligned(depth_drawn, 16) && seg_aligned(depth_fg, 16) && seg_aligned(frame_bgr, 4);
  const bool lds = bits <= kSegLdsBits;
  const dim3 grid(kSegBands, P);
#define SEG_COUNT(V, L)                                                                                                                  \
  hipLaunchKernelGGL((seg_count_kernel<V, L>), grid, dim3(kSegThreads), 0, st, frame_bgr, depth_drawn, depth_fg, bbox, H, W, bits, NB, margin, \
                     bins, nfb)
  if (vec && lds) SEG_COUNT(4, true);
  else if (vec) SEG_COUNT(4, false);
  else if (lds) SEG_COUNT(1, true);
  else SEG_COUNT(1, false);
#undef SEG_COUNT
  hipLaunchKernelGGL(seg_blend_kernel, dim3(ceil_div(2 * NB, kSegThreads), P), dim3(kSegThreads), 0, st, (const unsigned*)bins,
                     (const unsigned*)nfb, flags, skip_mask, min_pixels, NB, rate, (const int*)seg_age, seg_hist);
  hipLaunchKernelGGL(seg_finish_kernel, dim3(ceil_div(P, 64)), dim3(64), 0, st, (const unsigned*)nfb, flags, skip_mask, min_pixels, P, seg_age,
                     counts);
  return check_launch("track_seg_learn");
}
