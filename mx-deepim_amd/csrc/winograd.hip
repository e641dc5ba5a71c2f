// ------------------------------------------------------------------------------------------------ Winograd F(2x2, 3x3)
// 3x3 / stride 1 / pad 1 layers (conv3_1, conv4_1, conv5_1, conv6_1 of deepIM_flownet.py:103-191) as
//   V = B^T d B  (input tiles 4x4, stride 2)  ->  16 independent GEMMs  M_k = V_k (T x Cin) * U_k (Cin x Cout)  ->  Y = A^T M A
// 2.25x fewer multiply-adds than the direct form; the GEMMs run as ONE persistent stream-K launch (wino_gemm.hip).  Transforms are exact in the sense of using only +,- on the data (B, A have entries
// 0, +-1); the weight transform G (entries 1, 1/2) is applied once at pack time.  f32 throughout.
#include "wino_driver.h"

namespace dim {

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// V[t][k][c]: thread = (tile t, channel quad)
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, float* __restrict__ V, int N, int H, int W, int C,
                                                         int in_cstride, int th, int tw, FastDiv div_cq, FastDiv div_tw, FastDiv div_th) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned CQ = C >> 2;
  const unsigned T = (unsigned)N * th * tw;
  const unsigned t = fastdiv(idx, div_cq);
  if (t >= T) return;
  const unsigned cq = idx - t * CQ;
  const unsigned r = fastdiv(t, div_tw);
  const unsigned tx = t - r * tw;
  const unsigned n = fastdiv(r, div_th);
  const unsigned ty = r - n * th;
  const int y0 = 2 * (int)ty - 1, x0 = 2 * (int)tx - 1;
  const float* base = x + (long)n * H * W * in_cstride + cq * 4;
  float4 d[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int yy = y0 + a, xx = x0 + b;
      d[a][b] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                    ? *reinterpret_cast<const float4*>(base + ((long)yy * W + xx) * in_cstride)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  float4 tmp[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {  // B^T d
    tmp[0][b] = f4sub(d[0][b], d[2][b]);
    tmp[1][b] = f4add(d[1][b], d[2][b]);
    tmp[2][b] = f4sub(d[2][b], d[1][b]);
    tmp[3][b] = f4sub(d[1][b], d[3][b]);
  }
  const long plane = C;  // V [t][k][c]: the 16 planes of a tile are consecutive K columns of its row (wino_gemm.hip)
  float* out = V + (long)t * 16 * C + cq * 4;
#pragma unroll
  for (int a = 0; a < 4; ++a) {  // (.) B
    *reinterpret_cast<float4*>(out + (a * 4 + 0) * plane) = f4sub(tmp[a][0], tmp[a][2]);
    *reinterpret_cast<float4*>(out + (a * 4 + 1) * plane) = f4add(tmp[a][1], tmp[a][2]);
    *reinterpret_cast<float4*>(out + (a * 4 + 2) * plane) = f4sub(tmp[a][2], tmp[a][1]);
    *reinterpret_cast<float4*>(out + (a * 4 + 3) * plane) = f4sub(tmp[a][1], tmp[a][3]);
  }
}

// Y = A^T M A + bias, LeakyReLU; thread = (tile t, output-channel quad); writes the 2x2 outputs that fall inside H x W
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ y,
                                                          int N, int H, int W, int C, int out_cstride, int out_coff, int th, int tw,
                                                          float slope, FastDiv div_cq, FastDiv div_tw, FastDiv div_th) {
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned CQ = C >> 2;
  const unsigned T = (unsigned)N * th * tw;
  const unsigned t = fastdiv(idx, div_cq);
  if (t >= T) return;
  const unsigned cq = idx - t * CQ;
  const unsigned r = fastdiv(t, div_tw);
  const unsigned tx = t - r * tw;
  const unsigned n = fastdiv(r, div_th);
  const unsigned ty = r - n * th;
  const long plane = C;  // M [t][k][c]
  const float* in = M + (long)t * 16 * C + cq * 4;
  float4 m[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const float4*>(in + (a * 4 + b) * plane);
  float4 r0[4], r1[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {  // A^T m
    r0[b] = f4add(f4add(m[0][b], m[1][b]), m[2][b]);
    r1[b] = f4sub(f4sub(m[1][b], m[2][b]), m[3][b]);
  }
  float4 o[2][2];
  o[0][0] = f4add(f4add(r0[0], r0[1]), r0[2]);
  o[0][1] = f4sub(f4sub(r0[1], r0[2]), r0[3]);
  o[1][0] = f4add(f4add(r1[0], r1[1]), r1[2]);
  o[1][1] = f4sub(f4sub(r1[1], r1[2]), r1[3]);
  const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int oy = 2 * (int)ty + a, ox = 2 * (int)tx + b;
      if (oy < H && ox < W) {
        float4 v = f4add(o[a][b], bv);
        v.x = v.x > 0.f ? v.x : v.x * slope;
        v.y = v.y > 0.f ? v.y : v.y * slope;
        v.z = v.z > 0.f ? v.z : v.z * slope;
        v.w = v.w > 0.f ? v.w : v.w * slope;
        *reinterpret_cast<float4*>(y + (((long)n * H + oy) * W + ox) * out_cstride + out_coff + cq * 4) = v;
      }
    }
}

// U_k = G g G^T per (co, ci), written in the 1x1 packed layout of each of the 16 GEMMs: [k][ci/32][co][ci%32]
// DGRAD: the kernel of the input gradient, g'[ci -> co][kh][kw] = w[ci][co][2 - kh][2 - kw] read from the forward's (O, I, 3, 3) array
// (Cout / Cin are the GEMM's: dX channels / dY channels), instead of a flipped + transposed copy made by the caller
template <bool DGRAD>
__global__ void wino_pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cout * Cin) return;
  const int ci = (int)(idx % Cin), co = (int)(idx / Cin);
  float g[9];
  {
    const float* gp = w + (DGRAD ? (long)ci * Cout + co : (long)co * Cin + ci) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = gp[DGRAD ? 8 - i : i];
  }
  float Gg[4][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    Gg[0][j] = g[j];
    Gg[1][j] = 0.5f * (g[j] + g[3 + j] + g[6 + j]);
    Gg[2][j] = 0.5f * (g[j] - g[3 + j] + g[6 + j]);
    Gg[3][j] = g[6 + j];
  }
  const long per_k = (long)Cin * Cout;
  float* o = wp + ((long)(ci >> 5) * Cout + co) * 32 + (ci & 31);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[(i * 4 + 0) * per_k] = Gg[i][0];
    o[(i * 4 + 1) * per_k] = 0.5f * (Gg[i][0] + Gg[i][1] + Gg[i][2]);
    o[(i * 4 + 2) * per_k] = 0.5f * (Gg[i][0] - Gg[i][1] + Gg[i][2]);
    o[(i * 4 + 3) * per_k] = Gg[i][2];
  }
}

// ------------------------------------------------------------------------------------------------ Winograd F(4x4, 3x3)
// Same scheme with 6x6 input tiles at stride 4 and 36 GEMMs: 4x fewer multiply-adds than the direct form (F(2x2): 2.25x) and
// 2.25 T-tile planes per input pixel instead of 4, i.e. less transform traffic as well.  Cook-Toom points {0, 1, -1, 2, -1/2, inf}:
// mixing a large and a small point keeps the f32 error at ~2e-6 rms / 2e-5 max of the output scale (the usual {0,+-1,+-2}: 4e-5 max).
//   B^T = [1 3/2 -2 -3/2 1 0; 0 -1 -5/2 -1/2 1 0; 0 1 1/2 -5/2 1 0; 0 -1/2 -1 1/2 1 0; 0 2 -1 -2 1 0; 0 1 3/2 -2 -3/2 1]
//   G   = [1 0 0; -1/3 -1/3 -1/3; 1/3 -1/3 1/3; 1/15 2/15 4/15; -16/15 8/15 -4/15; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -1/2 0; 0 1 1 4 1/4 0; 0 1 -1 8 -1/8 1]
constexpr int kWino4Vec = 2;  // channels per thread of the F(4x4) transforms

template <int VEC>
struct WinoVec {
  typedef float type __attribute__((ext_vector_type(VEC)));
};

#define DIM_WINO4_BT(O, D, S)                                                          \
  {                                                                                    \
    O[0 * S] = D[0] + 1.5f * D[1] - 2.f * D[2] - 1.5f * D[3] + D[4];                    \
    O[1 * S] = D[4] - D[1] - 2.5f * D[2] - 0.5f * D[3];                                 \
    O[2 * S] = D[4] + D[1] + 0.5f * D[2] - 2.5f * D[3];                                 \
    O[3 * S] = D[4] - 0.5f * D[1] - D[2] + 0.5f * D[3];                                 \
    O[4 * S] = D[4] + 2.f * D[1] - D[2] - 2.f * D[3];                                   \
    O[5 * S] = D[1] + 1.5f * D[2] - 2.f * D[3] - 1.5f * D[4] + D[5];                    \
  }

// ---- forward 5x5 / stride-2 layers: the zero blocks of the transformed weights are neither stored in V nor multiplied.
// For an odd phase (py = 1) the third row of the sub-kernel g is zero, and the last row of G is [0 0 1]: every plane (a, b) with a = 5 of
// U = G g G^T is exactly zero for that phase; likewise px = 1 and b = 5.  That is 6 + 6 + 11 = 23 of the 144 (phase, plane) blocks:
//   planes (a, b < 5)   phases 0 1 2 3        planes (5, b < 5)   phases (0,0) (0,1)
//   planes (a < 5, 5)   phases (0,0) (1,0)    plane  (5, 5)       phase  (0,0)
// (wino5_phase_mask, common.h).  Layouts and sizes of V, U, U3 and M are unchanged: wino4_input_kernel<VEC, 2, true> leaves the 23 blocks
// of a tile row unwritten (holes), the plane GEMMs step over their chunks (WGemmArgs::skip5) and U keeps the zeros it always held.
// The GEMM's ranges are still cut in the flat chunk list of the full K, so every item is split between two workgroups exactly where it
// was when the zeros were multiplied, and adding or leaving out exact zeros does not change a float sum: results keep their bits.
// The backward paths (weight gradient: all of V; input gradient: zero structure on the GEMM's N side) do not skip.

// V[t][k][c], k = 6a + b: thread = (tile t, VEC channels).
// S = 1: a 3x3 / stride-1 / pad-1 layer.  S = 2: a 5x5 / stride-2 / pad-2 layer as the sum of four 3x3 / stride-1 / pad-1
// convolutions of its phase images X^(py,px)[r][q] = x[2r + py][2q + px] (sub-kernels g[u][v] = w[2u + py][2v + px], zero beyond
// the 5 taps): the four transformed phase tiles are concatenated along the channels, V has 4C of them (phase-major), so that ONE
// GEMM per Winograd plane contracts over phases and channels and the output transform is that of the stride-1 layer.
// FWD5 (S = 2, the forward layer): the blocks that meet zero weights are not stored (predicated stores; the loads are unconditional).
template <int VEC, int S, bool FWD5 = false>
__global__ __launch_bounds__(256) void wino4_input_kernel(const float* __restrict__ x, float* __restrict__ V, int N, int H, int W, int C,
                                                          int in_cstride, int th, int tw, FastDiv div_cq, FastDiv div_tw, FastDiv div_th,
                                                          unsigned nblk, WGemmArgs plan) {
#pragma clang fp contract(fast)
  typedef typename WinoVec<VEC>::type vf;
  if (blockIdx.x >= nblk) {  // spare blocks: zero the M tiles that two workgroups of the following stream-K GEMM share
    wino_gemm_zero_tile(plan, (int)(blockIdx.x - nblk) + 1);
    return;
  }
  // XCD-contiguous numbering: neighbouring tiles share two of their six input rows / columns, and block ids go round-robin to the 8
  // XCDs -- in launch order every overlap is fetched into a second L2 (PMC: 1.4x the algorithmic bytes on the fabric)
  const unsigned idx = (unsigned)wg_xcd_contiguous((int)blockIdx.x, (int)nblk) * 256u + threadIdx.x;
  const unsigned CT = C * S * S;  // channels of V
  const unsigned CQ = CT / VEC;
  const unsigned T = (unsigned)N * th * tw;
  const unsigned t = fastdiv(idx, div_cq);
  if (t >= T) return;
  const unsigned cq = idx - t * CQ;
  const unsigned r = fastdiv(t, div_tw);
  const unsigned tx = t - r * tw;
  const unsigned n = fastdiv(r, div_th);
  const unsigned ty = r - n * th;
  const int y0 = 4 * (int)ty - 1, x0 = 4 * (int)tx - 1;  // tile origin in the (phase) image
  const unsigned cc = cq * VEC;
  const unsigned ph = S == 1 ? 0u : (unsigned)(cc >= (unsigned)C) + (unsigned)(cc >= 2u * C) + (unsigned)(cc >= 3u * C);
  const int py = ph >> 1, px = ph & 1;
  const float* base = x + (long)n * H * W * in_cstride + (cc - ph * C);
  vf tmp[36];
#pragma unroll
  for (int b = 0; b < 6; ++b) {  // B^T d, one tile column at a time
    const int xx = S * (x0 + b) + px;
    const bool okx = (unsigned)xx < (unsigned)W;
    const int xc = okx ? xx : 0;
    vf d[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      // load from a clamped address, then select: a conditional load would compile to a branch with a wait per load
      const int yy = S * (y0 + a) + py;
      const bool ok = okx && (unsigned)yy < (unsigned)H;
      const int yc = (unsigned)yy < (unsigned)H ? yy : 0;
      vf v = *reinterpret_cast<const vf*>(base + ((long)yc * W + xc) * in_cstride);
      d[a] = ok ? v : (vf)(0.f);
    }
    vf* o = tmp + b;
    DIM_WINO4_BT(o, d, 6)
  }
  const long plane = CT;  // V [t][k][c]
  float* out = V + (long)t * 36 * CT + cc;
#pragma unroll
  for (int a = 0; a < 6; ++a) {  // (.) B
    vf o[6];
    const vf* d = tmp + 6 * a;
    DIM_WINO4_BT(o, d, 1)
#pragma unroll
    for (int b = 0; b < 6; ++b)
      if (!FWD5 || ((a < 5 || py == 0) && (b < 5 || px == 0)))
        __builtin_nontemporal_store(o[b], reinterpret_cast<vf*>(out + (a * 6 + b) * plane));
  }
}

#define DIM_WINO4_AT(O, M, S)                                       \
  {                                                                 \
    const vf s1 = M[1] + M[2], d1 = M[1] - M[2];                    \
    O[0 * S] = M[0] + s1 + M[3] + M[4];                             \
    O[1 * S] = d1 + 2.f * M[3] - 0.5f * M[4];                       \
    O[2 * S] = s1 + 4.f * M[3] + 0.25f * M[4];                      \
    O[3 * S] = d1 + 8.f * M[3] - 0.125f * M[4] + M[5];              \
  }

// Y = A^T M A + bias, LeakyReLU; thread = (tile t, VEC output channels); writes the 4x4 outputs that fall inside H x W.
// S = 2 (input gradient of a 5x5 / stride-2 layer): M carries 4 C channels, phase-major; the 4x4 block of phase (py,px) is one
// of the four stride-2 phase images of the H x W output: pixel (2 (4 ty + a) + py, 2 (4 tx + b) + px), channel c.
template <int VEC, int S>
__global__ __launch_bounds__(256) void wino4_output_kernel(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ y,
                                                           int N, int H, int W, int C, int out_cstride, int out_coff, int th, int tw,
                                                           float slope, FastDiv div_cq, FastDiv div_tw, FastDiv div_th) {
#pragma clang fp contract(fast)
  typedef typename WinoVec<VEC>::type vf;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned CT = C * S * S;  // channels of M
  const unsigned CQ = CT / VEC;
  const unsigned T = (unsigned)N * th * tw;
  const unsigned t = fastdiv(idx, div_cq);
  if (t >= T) return;
  const unsigned cq = idx - t * CQ;
  const unsigned r = fastdiv(t, div_tw);
  const unsigned tx = t - r * tw;
  const unsigned n = fastdiv(r, div_th);
  const unsigned ty = r - n * th;
  const long plane = CT;  // M [t][k][c]
  const unsigned cc = cq * VEC;
  const unsigned ph = S == 1 ? 0u : (unsigned)(cc >= (unsigned)C) + (unsigned)(cc >= 2u * C) + (unsigned)(cc >= 3u * C);
  const int py = ph >> 1, px = ph & 1;
  const unsigned co = cc - ph * C;  // output channel
  const float* in = M + (long)t * 36 * CT + cc;
  vf rr[24];  // A^T m: rr[4 rows][6 columns]
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    vf m[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) m[a] = __builtin_nontemporal_load(reinterpret_cast<const vf*>(in + (a * 6 + b) * plane));
    vf* o = rr + b;
    DIM_WINO4_AT(o, m, 6)
  }
  vf bv = (vf)(0.f);
  if (bias) bv = *reinterpret_cast<const vf*>(bias + co);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    vf o[4];
    const vf* m = rr + 6 * a;
    DIM_WINO4_AT(o, m, 1)
    const int oy = S * (4 * (int)ty + a) + py;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int ox = S * (4 * (int)tx + b) + px;
      if (oy < H && ox < W) {
        vf v = o[b] + bv;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope;
        *reinterpret_cast<vf*>(y + (((long)n * H + oy) * W + ox) * out_cstride + out_coff + co) = v;
      }
    }
  }
}

// U_k = G g G^T for one 3x3 kernel g, scattered with stride per_k over the 36 planes; f64 inside (runs once per weight update)
__device__ __forceinline__ void wino4_transform_weight(const float g[9], float* __restrict__ o, long per_k) {
  const double G[6][3] = {{1., 0., 0.},
                          {-1. / 3, -1. / 3, -1. / 3},
                          {1. / 3, -1. / 3, 1. / 3},
                          {1. / 15, 2. / 15, 4. / 15},
                          {-16. / 15, 8. / 15, -4. / 15},
                          {0., 0., 1.}};
  double Gg[6][3];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Gg[i][j] = G[i][0] * g[j] + G[i][1] * g[3 + j] + G[i][2] * g[6 + j];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) o[(i * 6 + j) * per_k] = (float)(Gg[i][0] * G[j][0] + Gg[i][1] * G[j][1] + Gg[i][2] * G[j][2]);
}

// (Cout,Cin,3,3) -> the 1x1 packed layout of each of the 36 GEMMs: [k][ci/32][co][ci%32]
template <bool DGRAD>
__global__ void wino4_pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cout * Cin) return;
  const int ci = (int)(idx % Cin), co = (int)(idx / Cin);
  const float* gp = w + (DGRAD ? (long)ci * Cout + co : (long)co * Cin + ci) * 9;
  float g[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) g[i] = gp[DGRAD ? 8 - i : i];
  wino4_transform_weight(g, wp + ((long)(ci >> 5) * Cout + co) * 32 + (ci & 31), (long)Cin * Cout);
}

// (Cout,Cin,5,5) of a stride-2 layer -> 36 GEMMs over K = 4 Cin (phase-major: kk = (2 py + px) Cin + ci), sub-kernel of phase
// (py,px): g[u][v] = w[2u + py][2v + px], zero where 2u + py or 2v + px > 4
__global__ void wino4_pack_weight_5x5s2_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cout * Cin * 4) return;
  const int kk = (int)(idx % (4 * Cin)), co = (int)(idx / (4 * Cin));
  const int ph = kk / Cin, ci = kk - ph * Cin;
  const int py = ph >> 1, px = ph & 1;
  const float* gp = w + ((long)co * Cin + ci) * 25;
  float g[9];
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int i = 2 * u + py, j = 2 * v + px;
      g[u * 3 + v] = (i < 5 && j < 5) ? gp[i * 5 + j] : 0.f;
    }
  wino4_transform_weight(g, wp + ((long)(kk >> 5) * Cout + co) * 32 + (kk & 31), 4L * Cin * Cout);
}

// Input gradient of the 5x5 / stride-2 layer: dX^(py,px)[r][q] = sum_{u,v} g_ph[2-u][2-v] dY[r+u-1][q+v-1]  (the forward's sub-kernels,
// flipped), contracted over the OUTPUT channels: one F(4x4,3x3) transform of dY, 36 GEMMs with K = Cout and N = 4 Cin (phase-major
// n = (2 py + px) Cin + ci), phase-scattering output transform.  Packed [k][co/32][4 Cin][co%32].
__global__ void wino4_pack_weight_5x5s2_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Cout * Cin * 4) return;
  const int co = (int)(idx % Cout), nn = (int)(idx / Cout);
  const int ph = nn / Cin, ci = nn - ph * Cin;
  const int py = ph >> 1, px = ph & 1;
  const float* gp = w + ((long)co * Cin + ci) * 25;
  float g[9];
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const int i = 2 * (2 - u) + py, j = 2 * (2 - v) + px;
      g[u * 3 + v] = (i < 5 && j < 5) ? gp[i * 5 + j] : 0.f;
    }
  wino4_transform_weight(g, wp + ((long)(co >> 5) * (4 * Cin) + nn) * 32 + (co & 31), 4L * Cin * Cout);
}

// ------------------------------------------------------------------------------------------------ Winograd weight gradient
// dW[u][v] = sum_{n,y,x} X[y+u-1][x+v-1] dY[y][x] per 4x4 tile of dY is the correlation F(3x3, 4x4): input = the 6x6 tile of X (the
// forward's V = B^T d B, same tiles, same kernel), "filter" = the 4x4 tile of dY (D = G4 g G4^T), three outputs per axis:
//   dW = A3^T [ sum_tiles V (.) D ] A3      -- the sum over tiles and batch is a GEMM per plane (contraction over T), 36 instead of 144
// multiply-adds per tile and (ci, co).  Same six points {0, 1, -1, 2, -1/2, inf}:
//   G4  = [1 0 0 0; -1/3 -1/3 -1/3 -1/3; 1/3 -1/3 1/3 -1/3; 1/15 2/15 4/15 8/15; -16/15 8/15 -4/15 2/15; 0 0 0 1]
//   A3^T = [1 1 1 1 1 0; 0 1 -1 2 -1/2 0; 0 1 1 4 1/4 1]
#define DIM_WINO4_G4(O, D, S)                                                                        \
  {                                                                                                  \
    const vf ev_ = D[0] + D[2], od_ = D[1] + D[3];                                                   \
    O[0 * S] = D[0];                                                                                 \
    O[1 * S] = (-1.f / 3) * (ev_ + od_);                                                             \
    O[2 * S] = (1.f / 3) * (ev_ - od_);                                                              \
    O[3 * S] = (1.f / 15) * D[0] + (2.f / 15) * D[1] + (4.f / 15) * D[2] + (8.f / 15) * D[3];        \
    O[4 * S] = (-16.f / 15) * D[0] + (8.f / 15) * D[1] - (4.f / 15) * D[2] + (2.f / 15) * D[3];      \
    O[5 * S] = D[3];                                                                                 \
  }

// D[t][k][c] = (G4 g G4^T)[k] for the 4x4 tile g of dY at (4 ty, 4 tx); thread = (tile, VEC channels)
template <int VEC>
__global__ __launch_bounds__(256) void wino4_dy_kernel(const float* __restrict__ dy, float* __restrict__ D, int N, int H, int W, int C,
                                                       int cstride, int th, int tw, FastDiv div_cq, FastDiv div_tw, FastDiv div_th) {
#pragma clang fp contract(fast)
  typedef typename WinoVec<VEC>::type vf;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned CQ = C / VEC;
  const unsigned T = (unsigned)N * th * tw;
  const unsigned t = fastdiv(idx, div_cq);
  if (t >= T) return;
  const unsigned cq = idx - t * CQ;
  const unsigned r = fastdiv(t, div_tw);
  const unsigned tx = t - r * tw;
  const unsigned n = fastdiv(r, div_th);
  const unsigned ty = r - n * th;
  const float* base = dy + (long)n * H * W * cstride + cq * VEC;
  vf tmp[24];  // G4 g: [6][4]
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int xx = 4 * (int)tx + b;
    const bool okx = xx < W;
    const int xc = okx ? xx : 0;
    vf g[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int yy = 4 * (int)ty + a;
      const bool ok = okx && yy < H;
      vf v = *reinterpret_cast<const vf*>(base + ((long)(yy < H ? yy : 0) * W + xc) * cstride);
      g[a] = ok ? v : (vf)(0.f);
    }
    vf* o = tmp + b;
    DIM_WINO4_G4(o, g, 4)
  }
  float* out = D + (long)t * 36 * C + cq * VEC;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    vf o[6];
    const vf* g = tmp + 4 * a;
    DIM_WINO4_G4(o, g, 1)
#pragma unroll
    for (int b = 0; b < 6; ++b) *reinterpret_cast<vf*>(out + (a * 6 + b) * (long)C) = o[b];
  }
}

// dW = A3^T dM A3 per (co, kk): dM packed [p * K/32 + kk/32][Cout][kk%32] -> MXNet layout.  S = 1: 3x3 / stride-1 layer, K = Cin, dW is
// the (Cout,Cin,3,3) gradient.  S = 2: 5x5 / stride-2 layer, kk = (2 py + px) Cin + ci, and the 3x3 result of phase (py,px) holds the
// taps w[2u + py][2v + px] of the (Cout,Cin,5,5) gradient (u or v = 2 does not exist for an odd phase: dropped).
template <int S>
__global__ __launch_bounds__(256) void wino4_wgrad_output_kernel(const float* __restrict__ dM, float* __restrict__ dw, int Cout, int Cin,
                                                                 float scale, int accumulate) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int K = Cin * S * S;
  if (idx >= (long)Cout * K) return;
  const int kk = (int)(idx % K), co = (int)(idx / K);  // kk fastest: the 32 k of a packed row are contiguous
  const long per_k = (long)K * Cout;
  const float* in = dM + ((long)(kk >> 5) * Cout + co) * 32 + (kk & 31);
  const float AT[3][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f}, {0.f, 1.f, -1.f, 2.f, -0.5f, 0.f}, {0.f, 1.f, 1.f, 4.f, 0.25f, 1.f}};
  float r[3][6];  // A3^T dM
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    float m[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) m[a] = in[(a * 6 + b) * per_k];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 6; ++a) acc += AT[u][a] * m[a];
      r[u][b] = acc;
    }
  }
  const int ph = S == 1 ? 0 : kk / Cin, ci = kk - ph * Cin;
  const int py = ph >> 1, px = ph & 1;
  constexpr int KS = S == 1 ? 3 : 5;
  float* o = dw + ((long)co * Cin + ci) * (KS * KS);
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      float acc = 0.f;
#pragma unroll
      for (int b = 0; b < 6; ++b) acc += r[u][b] * AT[v][b];
      const int i = S == 1 ? u : 2 * u + py, j = S == 1 ? v : 2 * v + px;
      if (i < KS && j < KS) {
        const float val = acc * scale;
        o[i * KS + j] = accumulate ? o[i * KS + j] + val : val;
      }
    }
}

}  // namespace dim

using namespace dim;

extern "C" {

long dim_winograd_packed_weight_floats(int Cout, int Cin, int m) { return wino_packed_with_split((long)(m + 2) * (m + 2) * Cout * Cin); }

long dim_winograd_workspace_floats(int N, int H, int W, int Cin, int Cout, int m) {
  return m == 2 || m == 4 ? wino_geom(N, H, W, (m + 2) * (m + 2), m, Cin, Cout).workspace_floats() : 0;
}

int dim_winograd_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int m, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(m == 2 || m == 4, "output tile m must be 2 or 4");
  DIM_REQUIRE(Cin % 32 == 0 && Cout % 64 == 0, "Cin %% 32 == 0 and Cout %% 64 == 0 required");
  long total = (long)Cout * Cin;
  if (m == 2)
    hipLaunchKernelGGL(wino_pack_weight_kernel<false>, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, Cout, Cin);
  else
    hipLaunchKernelGGL(wino4_pack_weight_kernel<false>, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, Cout, Cin);
  int rc = check_launch("winograd_pack_weight");
  return rc != DIM_OK ? rc : wino_split_weights(w_packed, (long)(m + 2) * (m + 2) * (Cin / 32), Cout, as_stream(stream));
}

// transformed weights of the INPUT gradient of a 3x3 / stride-1 / pad-1 layer, straight from its forward (Cout, Cin, 3, 3) array:
// == dim_winograd_pack_weight of w.flip(2, 3).transpose(0, 1), i.e. a Winograd layer with Cin output and Cout input channels
int dim_winograd_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int m, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(m == 2 || m == 4, "output tile m must be 2 or 4");
  DIM_REQUIRE(Cout % 32 == 0 && Cin % 64 == 0, "Cout %% 32 == 0 and Cin %% 64 == 0 required");
  long total = (long)Cout * Cin;
  if (m == 2)
    hipLaunchKernelGGL(wino_pack_weight_kernel<true>, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, Cin, Cout);
  else
    hipLaunchKernelGGL(wino4_pack_weight_kernel<true>, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, Cin, Cout);
  int rc = check_launch("winograd_dgrad_pack_weight");
  return rc != DIM_OK ? rc : wino_split_weights(w_packed, (long)(m + 2) * (m + 2) * (Cout / 32), Cin, as_stream(stream));
}

// S = 1: 3x3 / stride 1 / pad 1 with output tile m; S = 2: 5x5 / stride 2 / pad 2 through its four phase images (m = 4).
static int winograd_fwd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W, int Cin,
                        int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, int m, int S, void** events4,
                        void* stream, const WinoItemMap* map = nullptr) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(x && w_packed && y && workspace, "null pointer");
  DIM_REQUIRE(m == 2 || m == 4, "output tile m must be 2 or 4");
  DIM_REQUIRE(Cin % 32 == 0 && Cout % 64 == 0, "Cin %% 32 == 0 and Cout %% 64 == 0 required");
  if (in_cstride == 0) in_cstride = Cin;
  if (out_cstride == 0) out_cstride = Cout;
  DIM_REQUIRE(in_cstride >= Cin && in_cstride % 4 == 0 && out_cstride >= out_coff + Cout && out_cstride % 4 == 0 && out_coff % 4 == 0,
              "channel strides / offsets must be multiples of 4 and cover the channels");
  const int Ho = S == 1 ? H : (H + 1) / 2, Wo = S == 1 ? W : (W + 1) / 2;  // 5x5 / s2 / p2: floor((H - 1) / 2) + 1
  const WinoGeom g = wino_geom(N, Ho, Wo, (m + 2) * (m + 2), m, Cin * S * S, Cout);
  const int th = g.th, tw = g.tw, CT = g.K;
  hipStream_t st = as_stream(stream);
  const FastDiv dtw = make_fastdiv((unsigned)tw), dth = make_fastdiv((unsigned)th);
  auto gemm_tile = [&](long T) { return tile ? tile : (Cout % 128 == 0 && T >= 1024) ? 4 : 3; };
  auto input = [&](int n0, int n, long T, const WGemmArgs& plan, float* V) {
    const float* xs = x + (long)n0 * H * W * in_cstride;
    const unsigned nblk = (unsigned)ceil_div(T * (CT / kWino4Vec), 256);
    if (m == 2)
      hipLaunchKernelGGL(wino_input_kernel, dim3(ceil_div(T * (Cin / 4), 256)), dim3(256), 0, st, xs, V, n, H, W, Cin, in_cstride, th, tw,
                         make_fastdiv((unsigned)(Cin / 4)), dtw, dth);
    else if (S == 1)  // + G - 1 spare blocks that zero the M tiles shared by two GEMM workgroups
      hipLaunchKernelGGL((wino4_input_kernel<kWino4Vec, 1>), dim3(nblk + plan.G - 1), dim3(256), 0, st, xs, V, n, H, W, Cin, in_cstride, th,
                         tw, make_fastdiv((unsigned)(CT / kWino4Vec)), dtw, dth, nblk, plan);
    else
      hipLaunchKernelGGL((wino4_input_kernel<kWino4Vec, 2, true>), dim3(nblk + plan.G - 1), dim3(256), 0, st, xs, V, n, H, W, Cin, in_cstride,
                         th, tw, make_fastdiv((unsigned)(CT / kWino4Vec)), dtw, dth, nblk, plan);
    return check_launch("winograd_input");
  };
  auto output = [&](int n0, int n, long T, const float* M) {
    float* ys = y + (long)n0 * Ho * Wo * out_cstride;
    if (m == 2)
      hipLaunchKernelGGL(wino_output_kernel, dim3(ceil_div(T * (Cout / 4), 256)), dim3(256), 0, st, M, bias, ys, n, Ho, Wo, Cout, out_cstride,
                         out_coff, th, tw, slope, make_fastdiv((unsigned)(Cout / 4)), dtw, dth);
    else
      hipLaunchKernelGGL((wino4_output_kernel<kWino4Vec, 1>), dim3(ceil_div(T * (Cout / kWino4Vec), 256)), dim3(256), 0, st, M, bias, ys, n, Ho,
                         Wo, Cout, out_cstride, out_coff, th, tw, slope, make_fastdiv((unsigned)(Cout / kWino4Vec)), dtw, dth);
    return check_launch("winograd_output");
  };
  return wino_run_slices(g, w_packed, workspace, gemm_tile, /*skip5=*/S == 2, /*zeroed=*/m == 4, events4, st, input, output, map);
}

int dim_conv2d_fwd_winograd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                            int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, int m,
                            void** events4, void* stream) {
  return winograd_fwd(x, w_packed, bias, y, workspace, N, H, W, Cin, in_cstride, Cout, out_cstride, out_coff, slope, tile, m, 1, events4,
                       stream);
}

long dim_winograd5x5s2_packed_weight_floats(int Cout, int Cin) { return wino_packed_with_split(36L * Cout * 4 * Cin); }

long dim_winograd5x5s2_workspace_floats(int N, int H, int W, int Cin, int Cout) {
  return wino_geom(N, (H + 1) / 2, (W + 1) / 2, 36, 4, 4 * Cin, Cout).workspace_floats();
}

int dim_winograd5x5s2_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(Cin % 32 == 0 && Cout % 64 == 0, "Cin %% 32 == 0 and Cout %% 64 == 0 required");
  long total = 4L * Cout * Cin;
  hipLaunchKernelGGL(wino4_pack_weight_5x5s2_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, Cout,
                     Cin);
  int rc = check_launch("winograd5x5s2_pack_weight");
  return rc != DIM_OK ? rc : wino_split_weights(w_packed, 36L * (4 * Cin / 32), Cout, as_stream(stream));
}

int dim_winograd5x5s2_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(Cout % 32 == 0 && (4 * Cin) % 64 == 0, "Cout %% 32 == 0 and Cin %% 16 == 0 required");
  long total = 4L * Cout * Cin;
  hipLaunchKernelGGL(wino4_pack_weight_5x5s2_dgrad_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed,
                     Cout, Cin);
  int rc = check_launch("winograd5x5s2_dgrad_pack_weight");
  return rc != DIM_OK ? rc : wino_split_weights(w_packed, 36L * (Cout / 32), 4 * Cin, as_stream(stream));
}

int dim_conv2d_dgrad_winograd5x5s2(const float* dy, const float* w_packed, float* dx, float* workspace, int N, int H, int W, int Cin,
                                   int dx_cstride, int Cout, int dy_cstride, int tile, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(dy && w_packed && dx && workspace, "null pointer");
  DIM_REQUIRE(Cout % 32 == 0 && (4 * Cin) % 64 == 0 && Cin % 2 == 0, "Cout %% 32 == 0 and Cin %% 16 == 0 required");
  if (dx_cstride == 0) dx_cstride = Cin;
  if (dy_cstride == 0) dy_cstride = Cout;
  DIM_REQUIRE(dx_cstride >= Cin && dx_cstride % 2 == 0 && dy_cstride >= Cout && dy_cstride % 2 == 0, "channel strides must cover the channels");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const WinoGeom g = wino_geom(N, Ho, Wo, 36, 4, Cout, 4 * Cin);  // the forward's workspace: K and the output width change places
  const int th = g.th, tw = g.tw, CT = g.Nout;
  hipStream_t st = as_stream(stream);
  const FastDiv dtw = make_fastdiv((unsigned)tw), dth = make_fastdiv((unsigned)th);
  auto gemm_tile = [&](long T) { return tile ? tile : (CT % 128 == 0 && T >= 1024) ? 4 : 3; };
  auto input = [&](int n0, int n, long T, const WGemmArgs& plan, float* V) {
    const unsigned nblk = (unsigned)ceil_div(T * (Cout / kWino4Vec), 256);
    hipLaunchKernelGGL((wino4_input_kernel<kWino4Vec, 1>), dim3(nblk + plan.G - 1), dim3(256), 0, st, dy + (long)n0 * Ho * Wo * dy_cstride, V, n,
                       Ho, Wo, Cout, dy_cstride, th, tw, make_fastdiv((unsigned)(Cout / kWino4Vec)), dtw, dth, nblk, plan);
    return check_launch("winograd_dgrad_input");
  };
  auto output = [&](int n0, int n, long T, const float* M) {
    hipLaunchKernelGGL((wino4_output_kernel<kWino4Vec, 2>), dim3(ceil_div(T * (CT / kWino4Vec), 256)), dim3(256), 0, st, M, nullptr,
                       dx + (long)n0 * H * W * dx_cstride, n, H, W, Cin, dx_cstride, 0, th, tw, 1.0f, make_fastdiv((unsigned)(CT / kWino4Vec)),
                       dtw, dth);
    return check_launch("winograd_dgrad_output");
  };
  return wino_run_slices(g, w_packed, workspace, gemm_tile, /*skip5=*/0, /*zeroed=*/true, nullptr, st, input, output);
}

// Weight gradient through Winograd.  S = 1: 3x3 / stride 1 / pad 1; S = 2: 5x5 / stride 2 / pad 2 (phase images of x).
long dim_conv2d_wgrad_winograd_workspace_floats(int N, int H, int W, int Cin, int Cout, int S, int splits) {
  const int Ho = S == 1 ? H : (H + 1) / 2, Wo = S == 1 ? W : (W + 1) / 2;
  const long T = (long)N * ((Ho + 3) / 4) * ((Wo + 3) / 4);
  const long K = (long)Cin * S * S;
  if (splits < 1) splits = 1;
  return 36 * T * (K + Cout) + 36 * K * Cout * (long)(splits + 1);
}

int dim_conv2d_wgrad_winograd(const float* x, const float* dy, float* dw_oihw, float* workspace, int N, int H, int W, int Cin, int in_cstride,
                              int Cout, int dy_cstride, int S, int splits, float scale, int accumulate, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(x && dy && dw_oihw && workspace, "null pointer");
  DIM_REQUIRE(S == 1 || S == 2, "S must be 1 (3x3 / stride 1) or 2 (5x5 / stride 2)");
  DIM_REQUIRE(Cin % 32 == 0 && Cout % 64 == 0 && (Cin * S * S) % 64 == 0, "Cin %% 32 == 0 (%% 64 for S = 1) and Cout %% 64 == 0 required");
  if (in_cstride == 0) in_cstride = Cin;
  if (dy_cstride == 0) dy_cstride = Cout;
  DIM_REQUIRE(in_cstride >= Cin && in_cstride % 2 == 0 && dy_cstride >= Cout && dy_cstride % 2 == 0, "channel strides must cover the channels");
  const int Ho = S == 1 ? H : (H + 1) / 2, Wo = S == 1 ? W : (W + 1) / 2;
  const int th = (Ho + 3) / 4, tw = (Wo + 3) / 4;
  const long T = (long)N * th * tw;
  const int K = Cin * S * S;
  DIM_REQUIRE(T * 36 * (K > Cout ? K : Cout) < (1L << 29), "winograd wgrad: batch too large for 32-bit byte offsets");
  if (splits < 1) splits = 1;
  float* V = workspace;
  float* D = V + 36 * T * K;
  float* dM = D + 36 * T * Cout;
  float* slabs = dM + 36L * K * Cout;
  hipStream_t st = as_stream(stream);
  const FastDiv dtw = make_fastdiv((unsigned)tw), dth = make_fastdiv((unsigned)th);
  const unsigned nblk = (unsigned)ceil_div(T * (K / kWino4Vec), 256);  // no stream-K GEMM follows: no spare blocks
  const WGemmArgs none = {};
  if (S == 1)
    hipLaunchKernelGGL((wino4_input_kernel<kWino4Vec, 1>), dim3(nblk), dim3(256), 0, st, x, V, N, H, W, Cin, in_cstride, th, tw,
                       make_fastdiv((unsigned)(K / kWino4Vec)), dtw, dth, nblk, none);
  else
    hipLaunchKernelGGL((wino4_input_kernel<kWino4Vec, 2>), dim3(nblk), dim3(256), 0, st, x, V, N, H, W, Cin, in_cstride, th, tw,
                       make_fastdiv((unsigned)(K / kWino4Vec)), dtw, dth, nblk, none);
  hipLaunchKernelGGL(wino4_dy_kernel<kWino4Vec>, dim3(ceil_div(T * (Cout / kWino4Vec), 256)), dim3(256), 0, st, dy, D, N, Ho, Wo, Cout,
                     dy_cstride, th, tw, make_fastdiv((unsigned)(Cout / kWino4Vec)), dtw, dth);
  int rc = check_launch("winograd_wgrad_transforms");
  if (rc != DIM_OK) return rc;
  rc = launch_wgrad_planes(V, D, dM, slabs, (int)T, K, Cout, 36, splits, st);
  if (rc != DIM_OK) return rc;
  if (S == 1)
    hipLaunchKernelGGL(wino4_wgrad_output_kernel<1>, dim3(ceil_div((long)Cout * K, 256)), dim3(256), 0, st, dM, dw_oihw, Cout, Cin, scale,
                       accumulate);
  else
    hipLaunchKernelGGL(wino4_wgrad_output_kernel<2>, dim3(ceil_div((long)Cout * K, 256)), dim3(256), 0, st, dM, dw_oihw, Cout, Cin, scale,
                       accumulate);
  return check_launch("winograd_wgrad_output");
}

int dim_conv2d_fwd_winograd5x5s2(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                                 int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile, void** events4,
                                 void* stream) {
  return winograd_fwd(x, w_packed, bias, y, workspace, N, H, W, Cin, in_cstride, Cout, out_cstride, out_coff, slope, tile, 4, 2, events4,
                       stream);
}

int dim_conv2d_fwd_winograd5x5s2_map(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H,
                                     int W, int Cin, int in_cstride, int Cout, int out_cstride, int out_coff, float slope, int tile,
                                     const void* item_map, void** events4, void* stream) {
  return winograd_fwd(x, w_packed, bias, y, workspace, N, H, W, Cin, in_cstride, Cout, out_cstride, out_coff, slope, tile, 4, 2, events4,
                       stream, static_cast<const WinoItemMap*>(item_map));
}

}  // extern "C"
