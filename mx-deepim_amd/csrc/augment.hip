// Photometric augmentation of the observed training image, one fused pass over the blob: blur, saturation, contrast / brightness,
// white balance, sensor noise, clamp, 8-bit rounding.  The draws are made by the caller (lib/utils/augment.py), the kernel is
// deterministic; include/deepim_hip.h (dim_augment_observed) lists the rules in their order, tests/augment_reference.py restates them in
// numpy and the kernel gives the same bits.  The library is built with -ffp-contract=off: every a + w * v below is a rounded product
// and a rounded sum, as numpy computes it.
//
// Shape: a workgroup of 256 threads owns a tile of 64 x 32 pixels of one pair.  Plane after plane it loads the tile plus the halo of
// the PAIR's radius (16-byte loads, coordinates clamped to the image = replicate border) into LDS as grey levels, blurs the rows LDS to
// LDS, blurs the columns into registers (a thread keeps 4 consecutive pixels of 2 rows of all three planes: 24 floats), and then runs
// the colour chain and the noise in registers and stores 16 bytes per plane and row.  The radius is a kernel argument per pair
// (blockIdx.z), so no wave diverges on it; every radius is its own instantiation with the taps and the window offsets as constants.
// LDS: (32 + 14) x (64 + 16) + (32 + 14) x 64 floats = 26,496 bytes at radius 7 (one plane at a time), room for six workgroups per
// CU; the kernel's 112 vector registers allow four (16 waves per CU).  DESIGN.md has the reasons and the timings.
#include "common.h"

namespace dim {

constexpr int AUG_TW = 64, AUG_TH = 32, AUG_THREADS = 256, AUG_MAX_R = 7, AUG_TAPS = 2 * AUG_MAX_R + 1;
constexpr int AUG_QW = AUG_TW / 4;                                // float4 columns of a tile
constexpr int AUG_NR = AUG_TH / (AUG_THREADS / AUG_QW);           // rows per thread in the column pass and the colour chain
constexpr int AUG_MAX_HX = (AUG_MAX_R + 3) / 4 * 4;               // the halo in x is a whole number of float4
constexpr int AUG_IN_FLOATS = (AUG_TH + 2 * AUG_MAX_R) * (AUG_TW + 2 * AUG_MAX_HX);
constexpr int AUG_ROW_FLOATS = (AUG_TH + 2 * AUG_MAX_R) * AUG_TW;
constexpr int AUG_CHUNK = 256;                                    // pairs per launch: their radii travel as 4-bit fields
static_assert(AUG_NR * (AUG_THREADS / AUG_QW) == AUG_TH && AUG_TW % 4 == 0, "tile / thread mapping");

struct AugRadii {
  unsigned w[AUG_CHUNK / 8];
};

__device__ __forceinline__ unsigned aug_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// unit-variance noise from integers alone: the sum of four 16-bit uniforms of two hashes of (seed, counter)
__device__ __forceinline__ float aug_noise(unsigned seed, unsigned n) {
  const unsigned h0 = aug_mix(seed + n * 0x9E3779B9u);
  const unsigned h1 = aug_mix(h0 ^ 0x85EBCA6Bu);
  const int s = (int)((h0 & 0xFFFFu) + (h0 >> 16) + (h1 & 0xFFFFu) + (h1 >> 16));
  return (float)(s - 131070) * 2.6428997e-05f;
}

// acc + w * v per component, written on pairs so that the compiler takes the packed float32 multiply and add (the same roundings)
typedef float aug_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 aug_axpy(float4 acc, float w, float4 v) {
  const aug_f2 w2 = {w, w};
  const aug_f2 lo = aug_f2{acc.x, acc.y} + w2 * aug_f2{v.x, v.y}, hi = aug_f2{acc.z, acc.w} + w2 * aug_f2{v.z, v.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// One plane of the tile at (x0, y0): grey levels src + mean, blurred with radius R -> v[j] = pixels 4 q .. 4 q + 3 of tile row
// (tid / 16) * AUG_NR + j.  Two barriers; the caller may call it again at once (the next load writes s_in, which nobody reads after
// the second barrier, and s_row is written again only behind the next call's first barrier).
template <int R>
__device__ __forceinline__ void aug_blur_plane(const float* __restrict__ src, int H, int W, int x0, int y0, float mean,
                                               const float* __restrict__ taps, float* s_in, float* s_row, float4 (&v)[AUG_NR]) {
  constexpr int HX = (R + 3) / 4 * 4, PIN = AUG_TW + 2 * HX, QIN = PIN / 4, ROWS = AUG_TH + 2 * R;
  const int tid = threadIdx.x;
  float w[2 * R + 1];
#pragma unroll
  for (int t = 0; t <= 2 * R; ++t) w[t] = taps[t];
#pragma unroll 1
  for (int i = tid; i < ROWS * QIN; i += AUG_THREADS) {
    const int row = i / QIN, q = i - row * QIN;
    const int y = min(max(y0 - R + row, 0), H - 1);
    const int x = x0 - HX + 4 * q;                       // a multiple of 4, like W: the float4 is inside the row or outside it
    float4 p = *reinterpret_cast<const float4*>(src + (long)y * W + min(max(x, 0), W - 4));
    if (x < 0) p = make_float4(p.x, p.x, p.x, p.x);
    if (x >= W) p = make_float4(p.w, p.w, p.w, p.w);
    *reinterpret_cast<float4*>(s_in + row * PIN + 4 * q) = make_float4(p.x + mean, p.y + mean, p.z + mean, p.w + mean);
  }
  __syncthreads();
#pragma unroll 1
  for (int i = tid; i < ROWS * AUG_QW; i += AUG_THREADS) {
    const int row = i / AUG_QW, q = i - row * AUG_QW;
    float win[4 + 2 * HX];
#pragma unroll
    for (int j = 0; j < 1 + HX / 2; ++j) {
      float4 p = *reinterpret_cast<const float4*>(s_in + row * PIN + 4 * (q + j));
      // keep the 16-byte read whole: left alone the compiler drops the unused ends of the window and re-cuts the rest into 4- and
      // 8-byte reads, which at 16 bytes between lanes hit the same banks four at a time
      asm volatile("" : "+v"(p.x), "+v"(p.y), "+v"(p.z), "+v"(p.w));
      win[4 * j] = p.x; win[4 * j + 1] = p.y; win[4 * j + 2] = p.z; win[4 * j + 3] = p.w;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t <= 2 * R; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = acc[k] + w[t] * win[HX - R + t + k];
    *reinterpret_cast<float4*>(s_row + row * AUG_TW + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
  __syncthreads();
  const int q = tid % AUG_QW, r0 = (tid / AUG_QW) * AUG_NR;
#pragma unroll
  for (int j = 0; j < AUG_NR; ++j) v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < 2 * R + AUG_NR; ++t) {
    const float4 p = *reinterpret_cast<const float4*>(s_row + (r0 + t) * AUG_TW + 4 * q);
#pragma unroll
    for (int j = 0; j < AUG_NR; ++j)
      if (t - j >= 0 && t - j <= 2 * R) v[j] = aug_axpy(v[j], w[t - j], p);
  }
  // The sums are finished HERE: without this the compiler sinks them into the bounds-guarded colour chain and keeps the 2 R + 2
  // float4 reads of all three planes alive until then (211 registers at radius 7, two waves per SIMD).
#pragma unroll
  for (int j = 0; j < AUG_NR; ++j) asm volatile("" : "+v"(v[j].x), "+v"(v[j].y), "+v"(v[j].z), "+v"(v[j].w));
}

struct AugArgs {
  const float* in;
  float* out;
  int H, W;
  float mean[3];          // of blob plane c (BGR channel 2 - c)
  const int* on;
  const float* taps;      // (B, 15)
  const float* chain;     // (B, 7): saturation, contrast, brightness, gain of plane 0, 1, 2, noise sigma
  const unsigned* seed;
  int quantize;
};

template <int R>
__device__ __forceinline__ void aug_tile(const AugArgs& a, int b, float* s_in, float* s_row) {
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;
  const int x = x0 + 4 * (tid % AUG_QW), yt = y0 + (tid / AUG_QW) * AUG_NR;
  const long plane = (long)a.H * a.W;
  const float* src = a.in + (long)b * 3 * plane;
  float* dst = a.out + (long)b * 3 * plane;
  float4 v[3][AUG_NR];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (R == 0) {
#pragma unroll
      for (int j = 0; j < AUG_NR; ++j) {
        v[c][j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x < a.W && yt + j < a.H) {
          const float4 p = *reinterpret_cast<const float4*>(src + c * plane + (long)(yt + j) * a.W + x);
          v[c][j] = make_float4(p.x + a.mean[c], p.y + a.mean[c], p.z + a.mean[c], p.w + a.mean[c]);
        }
      }
    } else {
      aug_blur_plane<R>(src + c * plane, a.H, a.W, x0, y0, a.mean[c], a.taps + b * AUG_TAPS, s_in, s_row, v[c]);
    }
  }
  if (x >= a.W) return;
  const float* ch = a.chain + b * 7;
  const float sat = ch[0], con = ch[1], bri = ch[2], sigma = ch[6];
  const float gain[3] = {ch[3], ch[4], ch[5]};
  const unsigned seed = a.seed[b];
#pragma unroll
  for (int j = 0; j < AUG_NR; ++j) {
    const int y = yt + j;
    if (y >= a.H) break;
    float px[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      px[c][0] = v[c][j].x; px[c][1] = v[c][j].y; px[c][2] = v[c][j].z; px[c][3] = v[c][j].w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gray = 0.299f * px[0][k] + 0.587f * px[1][k] + 0.114f * px[2][k];   // plane 0 is red
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t = gray + sat * (px[c][k] - gray);
        t = (t - 128.f) * con + 128.f + bri;
        t = t * gain[c];
        if (sigma != 0.f) t = t + sigma * aug_noise(seed, ((unsigned)c * (unsigned)a.H + (unsigned)y) * (unsigned)a.W + (unsigned)(x + k));
        t = fminf(fmaxf(t, 0.f), 255.f);
        if (a.quantize) t = rintf(t);
        px[c][k] = t - a.mean[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(dst + c * plane + (long)y * a.W + x) = make_float4(px[c][0], px[c][1], px[c][2], px[c][3]);
  }
}

__global__ __launch_bounds__(AUG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void augment_observed_kernel(AugArgs a, AugRadii radii, int b0) {
  __shared__ __attribute__((aligned(16))) float s_in[AUG_IN_FLOATS];
  __shared__ __attribute__((aligned(16))) float s_row[AUG_ROW_FLOATS];
  const int b = b0 + blockIdx.z;
  if (a.on[b] == 0) {   // the pair is left alone: its bits are copied
    const int x = blockIdx.x * AUG_TW + 4 * (threadIdx.x % AUG_QW), yt = blockIdx.y * AUG_TH + (threadIdx.x / AUG_QW) * AUG_NR;
    if (x >= a.W) return;
    const long plane = (long)a.H * a.W;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < AUG_NR; ++j)
        if (yt + j < a.H) {
          const long o = ((long)b * 3 + c) * plane + (long)(yt + j) * a.W + x;
          *reinterpret_cast<float4*>(a.out + o) = *reinterpret_cast<const float4*>(a.in + o);
        }
    return;
  }
  switch ((radii.w[blockIdx.z >> 3] >> (4 * (blockIdx.z & 7))) & 15u) {   // uniform over the workgroup
    case 0: aug_tile<0>(a, b, s_in, s_row); break;
    case 1: aug_tile<1>(a, b, s_in, s_row); break;
    case 2: aug_tile<2>(a, b, s_in, s_row); break;
    case 3: aug_tile<3>(a, b, s_in, s_row); break;
    case 4: aug_tile<4>(a, b, s_in, s_row); break;
    case 5: aug_tile<5>(a, b, s_in, s_row); break;
    case 6: aug_tile<6>(a, b, s_in, s_row); break;
    case 7: aug_tile<7>(a, b, s_in, s_row); break;
    default: break;   // the host refuses any other radius before it launches
  }
}

}  // namespace dim

using namespace dim;

extern "C" {

int dim_augment_observed(const float* in, float* out, int B, int H, int W, const float* pixel_means_bgr3, const int* on,
                         const int* radius_host, const float* taps, const float* chain, const unsigned* seed, int quantize, void* stream) {
  DIM_REQUIRE(in && out && pixel_means_bgr3 && on && radius_host && taps && chain && seed, "augment_observed: null pointer");
  DIM_REQUIRE(B > 0 && H > 0 && W > 0, "augment_observed: B, H and W must be positive, got %d %d %d", B, H, W);
  DIM_REQUIRE(W % 4 == 0, "augment_observed: W must be a multiple of 4 (16-byte accesses), got %d", W);
  DIM_REQUIRE(ceil_div(H, AUG_TH) <= 65535, "augment_observed: H above %d", 65535 * AUG_TH);
  DIM_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "augment_observed: in and out must be 16-byte aligned");
  const uintptr_t lo_in = reinterpret_cast<uintptr_t>(in), lo_out = reinterpret_cast<uintptr_t>(out);
  const uintptr_t bytes = (uintptr_t)B * 3 * (uintptr_t)H * (uintptr_t)W * sizeof(float);
  DIM_REQUIRE(lo_in + bytes <= lo_out || lo_out + bytes <= lo_in,
              "augment_observed: in and out alias (the halo of one tile is the output of another)");
  for (int b = 0; b < B; ++b)
    DIM_REQUIRE(radius_host[b] >= 0 && radius_host[b] <= AUG_MAX_R, "augment_observed: radius %d of pair %d outside 0..%d", radius_host[b], b,
                AUG_MAX_R);
  AugArgs a;
  a.in = in; a.out = out; a.H = H; a.W = W;
  for (int c = 0; c < 3; ++c) a.mean[c] = pixel_means_bgr3[2 - c];
  a.on = on; a.taps = taps; a.chain = chain; a.seed = seed; a.quantize = quantize != 0;
  hipStream_t st = as_stream(stream);
  for (int b0 = 0; b0 < B; b0 += AUG_CHUNK) {
    const int n = B - b0 < AUG_CHUNK ? B - b0 : AUG_CHUNK;
    AugRadii radii = {};
    for (int i = 0; i < n; ++i) radii.w[i >> 3] |= (unsigned)radius_host[b0 + i] << (4 * (i & 7));
    hipLaunchKernelGGL(augment_observed_kernel, dim3(ceil_div(W, AUG_TW), ceil_div(H, AUG_TH), n), dim3(AUG_THREADS), 0, st, a, radii, b0);
  }
  return check_launch("augment_observed");
}

}  // extern "C"
