// Internal header of the direct-convolution files: what more than one of them needs.  Nothing here is part of include/deepim_hip.h.
//
// Source map (`tile` = the argument of dim_conv2d_fwd* / ConvEx users that selects the kernel):
//   conv.hip             conv2d_fwd_impl (validation, ConvArgs set-up, the "auto" tail split, dispatch by tile), the launch plans
//                        (dim_conv_auto_plan, dim_conv2d_tail_plan, dim_winograd_gemm_tile*), split-K reduce, the input gradient and the
//                        deconvolution wrappers, the dim_conv2d_fwd* entry points
//   conv_gather.hip      gathered-tap MFMA kernels conv_fwd_kernel / conv_bf16_kernel: tiles 1, 2, 3, 4 (f32 and bf16) and 8 (bf16)
//   conv_first.hip       flow_conv1 from an LDS halo: tile 6 (f32 pipe, bf16 pipe, three-term f32 on the bf16 pipe) + its weight split
//   conv_bf16_tiles.hip  bf16 LDS-halo kernel (tile 7) and bf16 patch kernel (tile 9)
//   conv_pack.hip        every weight packer of the direct / dgrad / deconvolution / small-Cout / fc layers, f32 <-> bf16 converters
//   heads.hip            small-Cout convolution, tiny deconvolution, 16x upsampling, pose head (own arguments, no ConvArgs, no tile)
//   winograd.hip         Winograd transforms, weight packers and entry points (GEMMs in wino_gemm*.hip); wino_s2.hip: 3x3 / stride 2
//   wino_driver.h        their shared host side: slice geometry (workspace sizes, the 2^32 rule) and the loop over the slices of a batch
#pragma once
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace dim {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;        // final output (splits == 1) or slab base (splits > 1)
  int N, H, W, Cin;
  int Ho, Wo, Cout;
  int KH, KW, stride, pad_h, pad_w;
  int M;           // N*Ho*Wo
  int nchunks;     // total K chunks of 32
  int chunks_per_split;
  float slope;     // LeakyReLU slope (1 = linear)
  int has_bias;
  // generalised addressing (decoder): input pixel stride, output row stride / channel offset (write into a concat buffer),
  // and an output scatter (oy,ox) = (ho*osy + ooy, wo*osx + oox) clipped to OH x OW (sub-pixel phases of a deconvolution + Crop)
  int in_cstride, out_cstride, out_coff;
  int dense_out, OH, OW, osy, osx, ooy, oox;
  int accumulate;  // out += v (final pass only)
  unsigned x_bytes, w_bytes;  // extents of x / w for the buffer descriptors (loads past them return 0)
  unsigned y_bytes;           // extent of one output problem (kernels that store through a descriptor: tile 9)
  int xcd_chunk;   // > 0: workgroup id -> tile remap that keeps consecutive tiles on one XCD (see conv_fwd_kernel)
  FastDiv div_kw;  // 8-channel layer: flat tap index -> (kh, kw)
  int boy, box;    // batched launch with scattered output: problem b lands at (ooy + (b >> 1) boy, oox + (b & 1) box) (deconv phases)
  long bx, bw, by; // batched launch (gridDim.y > 1): element strides of x / w / y between the problems (Winograd: 16 GEMMs)
  int tile_off;    // first tile of this launch (tail launch of an "auto" workload)
  int slab_row0;   // split-K slabs hold rows [slab_row0, M)
  long slab_stride;  // elements between the slabs of consecutive splits
  int bf16;          // weights are packed bf16, products on v_mfma_f32_32x32x16_bf16 (conv_bf16_kernel)
  int slab_full;     // split-K slabs are whole copies of the OUTPUT tensor (its channel stride, offset and scatter): the partial
                     // results of a strided / scattered launch (input-gradient phases) land where the final values go, slab by slab
  // tile 9 as the input gradient of a layer whose INPUT went through LeakyReLU: out = v * (mask > 0 ? 1 : mask_slope) with `mask` laid
  // out like the output (the stored activation), and every wave's column sums over its pixels -> colsum[(colsum_row0 + 2 block + wm)]
  // [Cout] (the bias gradient of that layer after one small reduce): the separate LeakyReLU' + bias-gradient pass folded in
  const float* mask;
  float mask_slope;
  float* colsum;
  int colsum_row0;
};

// Epilogue of the gathered-tap kernels (f32 and bf16): bias + LeakyReLU (+ accumulate) and the store of a wave's TM x TN accumulator
// tiles.  D layout: col = lane & 31 -> output channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> GEMM row of the tile.
// Every store goes through a buffer descriptor and a row outside the output gets byte offset 0xFFFFFFFF, which the range check drops:
// no branches.  With a per-row `if` hipcc opens each block with `s_waitcnt vmcnt(0)` (the bias load is still "pending" across the
// block boundary), and on gfx950 vmcnt also counts the stores -- the wave's 32 .. 128 stores then leave one round trip (~0.2 us) at a
// time.  Round 1 gave the f32 full-tile path its own branch-free loop for that reason; the partial tiles, the scattered output of the
// deconvolution / strided-gradient phases, the accumulate path and the whole bf16 twin still paid it (6 us per workgroup of a bf16
// layer whose main loop is 7 us).
template <int TM, int TN>
__device__ __forceinline__ void conv_store_tiles(const ConvArgs& a, const f32x16 (&acc)[TM][TN], float* yb, int mrow, int ncol, int split) {
  const bool final = gridDim.z == 1;
  const bool shaped = final || a.slab_full;   // addressed like the output tensor itself
  const int ldc = shaped ? a.out_cstride : a.Cout;
  float* base = final ? yb : yb + (long)split * a.slab_stride;
  const unsigned extent = shaped ? a.y_bytes : (unsigned)((long)(a.M - a.slab_row0) * a.Cout * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(base, 0, extent, 0x00020000);
  float bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) bv[j] = (final && a.has_bias) ? a.bias[ncol + 32 * j] : 0.f;
  const float slope = final ? a.slope : 1.0f;
  int voff[TM][16];   // byte offset of the row's channel ncol (tile j: + 128 j bytes), -1 = not stored
  if (!shaped || a.dense_out) {
    const int col_b = ((shaped ? a.out_coff : 0) + ncol) * 4, row0 = shaped ? 0 : a.slab_row0;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mrow + 32 * i + (r & 3) + 8 * (r >> 2);
        voff[i][r] = m < a.M ? (m - row0) * (ldc * 4) + col_b : -1;
      }
  } else {
    // scattered output (deconvolution phase + Crop, strided-gradient phase): row m = (n, ho, wo) lands at (n, ho*osy+ooy, wo*osx+oox)
    // if that is inside OH x OW
    const int oyb = a.ooy + (int)(blockIdx.y >> 1) * a.boy, oxb = a.oox + (int)(blockIdx.y & 1) * a.box;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mrow + 32 * i + (r & 3) + 8 * (r >> 2);
        const int mm = m < a.M ? m : 0;
        const int wo = mm % a.Wo, t = mm / a.Wo;
        const int ho = t % a.Ho, n = t / a.Ho;
        const int oy = ho * a.osy + oyb, ox = wo * a.osx + oxb;
        const bool ok = m < a.M && (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
        voff[i][r] = ok ? (((n * a.OH + oy) * a.OW + ox) * ldc + a.out_coff + ncol) * 4 : -1;
      }
  }
  if (final && a.accumulate) {   // wave-uniform: out += result
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff[i][r], 128 * j, 0));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r] + bv[j];
          v = (v > 0.f ? v : v * slope) + old[r];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r] + bv[j];
          v = v > 0.f ? v : v * slope;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
        }
  }
}

// bf16 operands of v_mfma_f32_32x32x16_bf16; a float4 is rounded to four bf16 (v_cvt_pk_bf16_f32, round to nearest even)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x4 to_bf16x4(const float4& v) {
  bf16x4 p = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
  return p;
}

// three-term image of the first layer's weights (conv_first.hip), stored behind the packed f32 weights by dim_conv2d_pack_weight
constexpr int kC1Pairs = 25;
constexpr size_t kC1SplitBytes = 2 * (size_t)kC1Pairs * 3 * 2 * 32 * 16;   // both halves: 153 600 B behind the packed f32 weights

// taps of one axis of an input-gradient phase (see the dgrad section of conv.hip): the packer and the launcher walk the same phases
struct DgAxis {
  int ntaps, emin;
};
static inline DgAxis dg_axis(int K, int stride, int p, int ph) {
  if (stride == 1) return {K, -(K - 1 - p)};
  int emin = 1000, emax = -1000;
  for (int e = -K; e <= K; ++e) {
    int k = ph + p - 2 * e;
    if (k >= 0 && k < K) { emin = min(emin, e); emax = max(emax, e); }
  }
  if (emin > emax) return {0, 0};
  return {emax - emin + 1, emin};
}

// Reserves `bytes` of dynamic LDS for a kernel (hipFuncAttributeMaxDynamicSharedMemorySize), once per kernel: after the first success
// every call returns DIM_OK at once.  Kernel = the address of a __global__ function, e.g. reserve_lds<&conv_fwd_kernel<64, 64, 2, 2, false>>(n)
template <auto Kernel>
int reserve_lds(size_t bytes) {
  static bool done = false;
  if (!done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return set_err(DIM_ERR_LAUNCH, "hipFuncSetAttribute(LDS=%zu): %s", bytes, hipGetErrorString(e));
    done = true;
  }
  return DIM_OK;
}

// compute units of the current device, read once; 256 when the query fails (or answers fewer than the two that the paired
// first-layer workgroups need).  Sizes the persistent first-layer grids and the split tail of the "auto" plan.
inline int device_cu_count() {
  static const int n_cu = [] {
    int dev = 0, cus = 0;
    return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 1) ? cus : 256;
  }();
  return n_cu;
}

// ---- launchers, one per kernel family.  `a` is the ConvArgs that conv2d_fwd_impl has filled in and checked in general; each
// launcher checks what its own kernels require
// conv_gather.hip: tiles 1 - 4 and 8; tiles [tile_begin, tile_begin + tile_count) (-1: all) x `batch` problems x `splits` K ranges
int launch_conv_gather(const ConvArgs& a, int tile, int splits, hipStream_t st, int batch, int tile_begin, int tile_count);
int launch_conv_first(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st);       // conv_first.hip: tile 6
int launch_conv_bf16_halo(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st);   // conv_bf16_tiles.hip: tile 7
int launch_conv_bf16_patch(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st);  // conv_bf16_tiles.hip: tile 9
// conv_first.hip: packed f32 weights of flow_conv1 -> the three-term image behind them (conv1_split_weights_kernel)
int launch_conv1_split_weights(float* w_packed, hipStream_t st);

}  // namespace dim
