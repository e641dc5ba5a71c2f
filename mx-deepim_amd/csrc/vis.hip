// Contour overlays for test --vis: the outlines of up to 8 rendered layers (depth planes or 0/1 masks) blended over an observed frame,
// one pass from the float blobs to a finished 8-bit B,G,R frame.  include/deepim_hip.h (dim_vis_overlay) states the rules,
// tests/vis_reference.py restates them in numpy; everything behind the base colour is integer arithmetic, so the bytes are the same.
//
// Shape: a workgroup of 256 threads owns a tile of 64 x 32 pixels of one pair.  The L inside-bits of a pixel are one byte (bit l =
// layer l); four pixels are one 32-bit word and every step below works on whole words, the byte lanes in parallel:
//   1. s_in   the tile plus a halo of radius + 1 rows and 4 columns (one word), coordinates clamped to the frame, so that a neighbour
//             outside the frame repeats the pixel itself and cannot make it an edge
//   2. s_edge inside & ~(up & down & left & right), zeroed outside the frame (a clamped copy is no pixel, it must not be dilated)
//   3. s_row  the OR of the edge bytes over x - radius .. x + radius
//   4. the OR of s_row over y - radius .. y + radius into registers = the marked bits; a thread holds one word of two rows
//   5. the base colour from the three planes, the layers painted in order, 12 bytes stored per word
// LDS: 2 x 40 rows x 72 bytes + 40 x 64 + the counts = 8,384 bytes.  A row is 18 words: the 32 lanes of an access group read two
// rows, 36 distinct banks.
// With W % 4 == 0 and aligned pointers every global access is a whole word of pixels (16-byte loads, 12-byte stores); any other width
// takes the same kernel with one pixel per access.
#include "common.h"

namespace dim {

constexpr int VIS_TW = 64, VIS_TH = 32, VIS_THREADS = 256, VIS_MAX_L = 8, VIS_MAX_R = 3;
constexpr int VIS_QW = VIS_TW / 4;                       // words of a tile row
constexpr int VIS_PW = VIS_QW + 2;                       // ... plus one halo word on either side
constexpr int VIS_NR = VIS_TH / (VIS_THREADS / VIS_QW);  // rows per thread when painting
constexpr int VIS_MAX_ROWS = VIS_TH + 2 * (VIS_MAX_R + 1);
static_assert(VIS_NR * (VIS_THREADS / VIS_QW) == VIS_TH && VIS_MAX_R + 1 <= 4, "tile / thread mapping, halo within one word");

struct VisStyle {
  unsigned colour[VIS_MAX_L];   // B | G << 8 | R << 16
  unsigned alpha[VIS_MAX_L];    // edge_alpha | fill_alpha << 16
};

struct VisArgs {
  const float* image;    // (B,3,H,W)
  const float* layers;   // (L,B,H,W)
  unsigned char* out;    // (B,H,W,3)
  int* counts;           // (B,L,2) or NULL
  int B, H, W, radius;
  float mean[3];         // of blob plane c (BGR channel 2 - c)
  VisStyle style;
};

__device__ __forceinline__ unsigned vis_blend(unsigned c, unsigned colour, unsigned a) { return (c * (256u - a) + colour * a + 128u) >> 8; }

// v = plane value + mean as a grey level: rintf, clamp to [0, 255], NaN -> 0 (fmaxf drops the NaN)
__device__ __forceinline__ unsigned vis_base(float v, float mean) { return (unsigned)fminf(fmaxf(rintf(v + mean), 0.f), 255.f); }

// bytes of `c` moved towards higher x by n pixels, filled from the word on the left (n in 1..3) -- and the other way
__device__ __forceinline__ unsigned vis_from_left(unsigned left, unsigned c, int n) { return (c << (8 * n)) | (left >> (32 - 8 * n)); }
__device__ __forceinline__ unsigned vis_from_right(unsigned c, unsigned right, int n) { return (c >> (8 * n)) | (right << (32 - 8 * n)); }

// 0xFF in the bytes of the word at x .. x + 3 of row y that are pixels of the frame
__device__ __forceinline__ unsigned vis_frame_mask(int x, int y, int H, int W) {
  if (y < 0 || y >= H) return 0u;
  unsigned m = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) m |= (x + k >= 0 && x + k < W) ? 0xFFu << (8 * k) : 0u;
  return m;
}

template <int L, bool VEC>
__global__ __launch_bounds__(VIS_THREADS) void vis_overlay_kernel(VisArgs a) {
  __shared__ unsigned s_in[VIS_MAX_ROWS * VIS_PW], s_edge[VIS_MAX_ROWS * VIS_PW], s_row[VIS_MAX_ROWS * VIS_QW];
  __shared__ int s_cnt[2 * VIS_MAX_L];
  const int tid = threadIdx.x, b = blockIdx.z, H = a.H, W = a.W, R = a.radius;
  const int x0 = blockIdx.x * VIS_TW, y0 = blockIdx.y * VIS_TH;
  const int halo = R + 1, rows = VIS_TH + 2 * halo;
  const size_t plane = (size_t)H * (size_t)W;
  if (tid < 2 * VIS_MAX_L) s_cnt[tid] = 0;
  // 1. inside bits: row i of s_in is frame row y0 - halo + i, word q frame columns x0 - 4 + 4 q .. + 3, all clamped
  for (int i = tid; i < rows * VIS_PW; i += VIS_THREADS) {
    const int row = i / VIS_PW, q = i - row * VIS_PW;
    const int y = min(max(y0 - halo + row, 0), H - 1), x = x0 - 4 + 4 * q;
    unsigned bits = 0u;
    if (VEC) {   // x and W are multiples of 4: the word lies inside the row or outside it
      const int xc = min(max(x, 0), W - 4);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        float4 p = *reinterpret_cast<const float4*>(a.layers + ((size_t)l * a.B + b) * plane + (size_t)y * W + xc);
        if (x < 0) p = make_float4(p.x, p.x, p.x, p.x);
        if (x >= W) p = make_float4(p.w, p.w, p.w, p.w);
        bits |= ((p.x > 0.f ? 1u : 0u) | (p.y > 0.f ? 0x100u : 0u) | (p.z > 0.f ? 0x10000u : 0u) | (p.w > 0.f ? 0x1000000u : 0u)) << l;
      }
    } else {
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const float* src = a.layers + ((size_t)l * a.B + b) * plane + (size_t)y * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) bits |= (src[min(max(x + k, 0), W - 1)] > 0.f ? 1u : 0u) << (8 * k + l);
      }
    }
    s_in[i] = bits;
  }
  __syncthreads();
  // 2. edge bits of rows 1 .. rows - 2 (the rows whose vertical neighbours are there).  The outermost bytes of the two halo words take
  // the word itself as the missing neighbour: they lie 4 pixels outside the tile, where no radius <= 3 reaches.
  for (int i = tid; i < (rows - 2) * VIS_PW; i += VIS_THREADS) {
    const int row = 1 + i / VIS_PW, q = i % VIS_PW, at = row * VIS_PW + q;
    const unsigned c = s_in[at], up = s_in[at - VIS_PW], down = s_in[at + VIS_PW];
    const unsigned left = s_in[q > 0 ? at - 1 : at], right = s_in[q < VIS_PW - 1 ? at + 1 : at];
    const unsigned all = up & down & vis_from_left(left, c, 1) & vis_from_right(c, right, 1);
    s_edge[at] = c & ~all & vis_frame_mask(x0 - 4 + 4 * q, y0 - halo + row, H, W);
  }
  __syncthreads();
  // 3. rows 1 .. rows - 2 again, the tile's own words: OR over x - R .. x + R
  for (int i = tid; i < (rows - 2) * VIS_QW; i += VIS_THREADS) {
    const int row = 1 + i / VIS_QW, q = i % VIS_QW, at = row * VIS_PW + 1 + q;
    const unsigned c = s_edge[at], left = s_edge[at - 1], right = s_edge[at + 1];
    unsigned m = c;
    for (int n = 1; n <= R; ++n) m |= vis_from_left(left, c, n) | vis_from_right(c, right, n);
    s_row[row * VIS_QW + q] = m;
  }
  __syncthreads();
  // 4. + 5. a thread paints word q of tile rows r0 .. r0 + VIS_NR - 1
  const int q = tid % VIS_QW, r0 = (tid / VIS_QW) * VIS_NR, x = x0 + 4 * q;
  int n_mark[L], n_in[L];
#pragma unroll
  for (int l = 0; l < L; ++l) n_mark[l] = n_in[l] = 0;
  if (x < W) {
#pragma unroll
    for (int j = 0; j < VIS_NR; ++j) {
      const int y = y0 + r0 + j, row = halo + r0 + j;
      if (y >= H) break;
      unsigned mark = 0u;
      for (int dy = -R; dy <= R; ++dy) mark |= s_row[(row + dy) * VIS_QW + q];
      const unsigned frame = vis_frame_mask(x, y, H, W);
      const unsigned in = s_in[row * VIS_PW + 1 + q] & frame;
      mark &= frame;
      float px[3][4];
      const float* src = a.image + (size_t)b * 3 * plane + (size_t)y * W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (VEC) {
          const float4 p = *reinterpret_cast<const float4*>(src + c * plane);
          px[c][0] = p.x; px[c][1] = p.y; px[c][2] = p.z; px[c][3] = p.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) px[c][k] = x + k < W ? src[c * plane + k] : 0.f;
        }
      }
      unsigned bgr[4][3];   // plane 0 is red
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) bgr[k][2 - c] = vis_base(px[c][k], a.mean[c]);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const unsigned colour = a.style.colour[l], edge_alpha = a.style.alpha[l] & 0xFFFFu, fill_alpha = a.style.alpha[l] >> 16;
        n_mark[l] += __popc((mark >> l) & 0x01010101u);
        n_in[l] += __popc((in >> l) & 0x01010101u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool marked = (mark >> (8 * k + l)) & 1u, inside = (in >> (8 * k + l)) & 1u;
          const unsigned alpha = marked ? edge_alpha : (inside ? fill_alpha : 0u);
          if (alpha != 0u) {
#pragma unroll
            for (int c = 0; c < 3; ++c) bgr[k][c] = vis_blend(bgr[k][c], (colour >> (8 * c)) & 0xFFu, alpha);
          }
        }
      }
      unsigned char* dst = a.out + (((size_t)b * H + y) * W + x) * 3;
      if (VEC) {   // 12 bytes at a 4-byte aligned address
        unsigned* d = reinterpret_cast<unsigned*>(dst);
        d[0] = bgr[0][0] | bgr[0][1] << 8 | bgr[0][2] << 16 | bgr[1][0] << 24;
        d[1] = bgr[1][1] | bgr[1][2] << 8 | bgr[2][0] << 16 | bgr[2][1] << 24;
        d[2] = bgr[2][2] | bgr[3][0] << 8 | bgr[3][1] << 16 | bgr[3][2] << 24;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x + k < W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[3 * k + c] = (unsigned char)bgr[k][c];
          }
      }
    }
  }
  if (a.counts == nullptr) return;   // uniform over the grid
  // a thread counts at most 8 pixels and a wave 512: both numbers of a layer ride in one word through the wave's sum, and one lane
  // per wave adds to LDS (every thread adding to LDS on its own: 40.2 us instead of 35.0 at 16 x 480 x 640, L = 3)
#pragma unroll
  for (int l = 0; l < L; ++l) {
    int v = n_mark[l] | n_in[l] << 16;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & (kWave - 1)) == 0 && v) {
      atomicAdd(&s_cnt[2 * l], v & 0xFFFF);
      atomicAdd(&s_cnt[2 * l + 1], v >> 16);
    }
  }
  __syncthreads();
  if (tid < 2 * L && s_cnt[tid]) atomicAdd(a.counts + (size_t)b * 2 * L + tid, s_cnt[tid]);
}

__global__ void vis_zero_counts_kernel(int* counts, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) counts[i] = 0;
}

template <int L>
static void vis_launch(const VisArgs& a, bool vec, hipStream_t st) {
  const dim3 grid(ceil_div(a.W, VIS_TW), ceil_div(a.H, VIS_TH), a.B);
  if (vec)
    hipLaunchKernelGGL((vis_overlay_kernel<L, true>), grid, dim3(VIS_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((vis_overlay_kernel<L, false>), grid, dim3(VIS_THREADS), 0, st, a);
}

static bool vis_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + nq && b < a + np;
}

}  // namespace dim

using namespace dim;

extern "C" {

int dim_vis_overlay(const float* image, const float* pixel_means_bgr3, const float* layers, int L, const int* style, int radius, int B,
                    int H, int W, unsigned char* out_bgr, int* counts, void* stream) {
  DIM_REQUIRE(image && pixel_means_bgr3 && layers && style && out_bgr, "vis_overlay: null pointer");
  DIM_REQUIRE(L >= 1 && L <= VIS_MAX_L, "vis_overlay: L must be in 1..%d, got %d", VIS_MAX_L, L);
  DIM_REQUIRE(radius >= 0 && radius <= VIS_MAX_R, "vis_overlay: radius must be in 0..%d, got %d", VIS_MAX_R, radius);
  DIM_REQUIRE(B >= 1 && B <= 65535, "vis_overlay: B must be in 1..65535, got %d", B);
  DIM_REQUIRE(H >= 1 && H <= 32767 && W >= 1 && W <= 32767, "vis_overlay: H and W must be in 1..32767, got %d %d", H, W);
  VisArgs a;
  for (int l = 0; l < L; ++l) {
    const int* s = style + 5 * l;
    DIM_REQUIRE(s[0] >= 0 && s[0] <= 255 && s[1] >= 0 && s[1] <= 255 && s[2] >= 0 && s[2] <= 255,
                "vis_overlay: colour of layer %d outside 0..255: %d %d %d", l, s[0], s[1], s[2]);
    DIM_REQUIRE(s[3] >= 0 && s[3] <= 256 && s[4] >= 0 && s[4] <= 256, "vis_overlay: alpha of layer %d outside 0..256: %d %d", l, s[3], s[4]);
    a.style.colour[l] = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16;
    a.style.alpha[l] = (unsigned)s[3] | (unsigned)s[4] << 16;
  }
  for (int l = L; l < VIS_MAX_L; ++l) a.style.colour[l] = a.style.alpha[l] = 0u;
  const size_t pixels = (size_t)B * (size_t)H * (size_t)W;
  DIM_REQUIRE(!vis_overlap(out_bgr, pixels * 3, image, pixels * 3 * sizeof(float)) &&
                  !vis_overlap(out_bgr, pixels * 3, layers, pixels * (size_t)L * sizeof(float)),
              "vis_overlay: out_bgr overlaps an input (the halo of one tile is the output of another)");
  DIM_REQUIRE((reinterpret_cast<uintptr_t>(image) & 3) == 0 && (reinterpret_cast<uintptr_t>(layers) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(counts) & 3) == 0, "vis_overlay: image, layers and counts must be 4-byte aligned");
  a.image = image; a.layers = layers; a.out = out_bgr; a.counts = counts;
  a.B = B; a.H = H; a.W = W; a.radius = radius;
  for (int c = 0; c < 3; ++c) a.mean[c] = pixel_means_bgr3[2 - c];
  const bool vec = W % 4 == 0 && ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(layers)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_bgr) & 3) == 0;
  hipStream_t st = as_stream(stream);
  if (counts) hipLaunchKernelGGL(vis_zero_counts_kernel, dim3(ceil_div((long)B * L * 2, 256)), dim3(256), 0, st, counts, B * L * 2);
  switch (L) {
    case 1: vis_launch<1>(a, vec, st); break;
    case 2: vis_launch<2>(a, vec, st); break;
    case 3: vis_launch<3>(a, vec, st); break;
    case 4: vis_launch<4>(a, vec, st); break;
    case 5: vis_launch<5>(a, vec, st); break;
    case 6: vis_launch<6>(a, vec, st); break;
    case 7: vis_launch<7>(a, vec, st); break;
    default: vis_launch<8>(a, vec, st); break;
  }
  return check_launch("vis_overlay");
}

}  // extern "C"
