// The first-layer kernels, tile 6 (source map: conv_impl.h)
#include "conv_impl.h"

namespace dim {

// ---------------------------------------------------------------------------------------------------------------- first layer, LDS halo
// flow_conv1 (8 channels, 7x7 / stride 2 / pad 3 -> 64 channels; deepIM_flownet.py:67-75) from an LDS-resident input patch.
// In conv_fwd_kernel<.., CIN8> this layer was the furthest below its roof (0.60 ms = 103 TFLOP/s at B = 16): only 13 K chunks per
// workgroup, so the pipeline fill (first gathered loads -> LDS -> barrier) and drain cost ~14 %, another 6 % went into the K padding
// 392 -> 416, and the 49 taps re-gathered the input 3.7x from beyond L2.  Here a workgroup owns an 8 x 16 block of output pixels x
// all 64 output channels: it loads the 21 x 37 x 8 input patch ONCE (zero outside the image = the padding), every wave then reads
// its A fragments for all 49 taps from LDS at shifted addresses (ds_read_b128 with an immediate offset per tap) and runs 392 MFMAs
// without another barrier or global activation load.  Four workgroups fit a CU (37 KB of LDS each), so one workgroup's patch load
// and epilogue hide under the MFMAs of the others.  Weights: the packed [chunk][64][32] array of dim_conv2d_pack_weight as it is
// (a chunk = 4 flat taps x 8 channels, so tap t's 8 channels of an output channel are 32 contiguous bytes), fetched per tap from L2
// one tap ahead.  K is exactly 392.  Same products, same f32 accumulation chain per output as the direct kernel (k order differs).
template <int KH, int KW>
__global__ __launch_bounds__(256) void conv1_halo_kernel(ConvArgs a) {
  constexpr int TH = 8, TW = 16;                 // output pixels per workgroup: 4 waves x (2 rows x 16)
  constexpr int S = 2;
  constexpr int PH = (TH - 1) * S + KH, PW = (TW - 1) * S + KW;   // 21 x 37 input pixels
  constexpr int PS = 12;                         // floats per patch pixel: 8 channels + 4 pad (48 B: 2-way instead of 4-way conflicts)
  constexpr int NPIX = PH * PW;
  __shared__ __attribute__((aligned(16))) float patch[NPIX * PS];
  // the bias through LDS: its address depends on the lane half, so `a.bias[...]` in the epilogue is a VECTOR load, and the wait for it
  // (one in-order counter for vector loads and stores on this chip) also waits for the stores issued just before: four store round
  // trips per workgroup in series
  __shared__ __attribute__((aligned(16))) float sbias[64];
  if (threadIdx.x < 64) sbias[threadIdx.x] = a.has_bias ? a.bias[threadIdx.x] : 0.f;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_w = (a.Wo + TW - 1) / TW, tiles_h = (a.Ho + TH - 1) / TH;
  int id = wg_xcd_contiguous((int)blockIdx.x, (int)gridDim.x);   // neighbouring tiles (shared halo) on one XCD
  const int twi = id % tiles_w;
  id /= tiles_w;
  const int thi = id % tiles_h;
  const int n = id / tiles_h;
  const int ho0 = thi * TH, wo0 = twi * TW;
  const int hi0 = ho0 * S - a.pad_h, wi0 = wo0 * S - a.pad_w;

  // ---- patch: 2 float4 per pixel; out-of-image pixels read zeros through the descriptor's range check
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  constexpr int ITEMS = (NPIX * 2 + 255) / 256;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int item = it * 256 + tid;
    if (item < NPIX * 2) {
      const int pix = item >> 1, half = item & 1;
      const int py = pix / PW, px = pix - py * PW;
      const int hi = hi0 + py, wi = wi0 + px;
      const bool ok = (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      const float4 v = buf_load16(rx, ok ? (((n * a.H + hi) * a.W + wi) * a.in_cstride + half * 4) * 4 : -1, 0);
      *reinterpret_cast<float4*>(&patch[pix * PS + half * 4]) = v;
    }
  }
  // ---- fragments.  The WEIGHTS are the MFMA's A operand (rows = output channels) and the pixels its B operand (columns), so a
  // lane ends up with 4 consecutive output channels of ONE pixel per accumulator quad: the epilogue is 8 float4 stores per lane
  // instead of 32 scalar ones
  const int frow = lane & 31, khalf = lane >> 5;
  const int p = wave * 32 + frow;               // output pixel = this lane's B column inside the block
  const int ty = p / TW, tx = p - ty * TW;
  const float* abase = &patch[((ty * S) * PW + tx * S) * PS + 4 * khalf];
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.w_bytes, 0x00020000);
  // weight fragment of tap t, output-channel tile j: 16 bytes at ((t / 4) * 64 + 32 j + frow) * 32 + (t % 4) * 8 + 4 khalf floats
  const int b_voff = (frow * 32 + 4 * khalf) * 4;
  auto load_b = [&](int t, float4& b0, float4& b1) {
    const int soff = ((t >> 2) * 64 * 32 + (t & 3) * 8) * 4;
    b0 = buf_load16(rw, b_voff, soff);
    b1 = buf_load16(rw, b_voff + 32 * 32 * 4, soff);
  };
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  float4 b0, b1, nb0, nb1;
  load_b(0, b0, b1);
  __syncthreads();
  float4 fa = *reinterpret_cast<const float4*>(abase);
  for (int kh = 0; kh < KH; ++kh) {
    const float* arow = abase + kh * PW * PS;
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      const int t = kh * KW + kw;
      // next tap's operands in flight while this tap multiplies (the one past the end re-reads tap 0: in range, unused)
      const int tn = (t + 1 < KH * KW) ? t + 1 : 0;
      load_b(tn, nb0, nb1);
      const float* anext = (kw + 1 < KW) ? arow + (kw + 1) * PS : ((kh + 1 < KH) ? arow + PW * PS : abase);
      const float4 nfa = *reinterpret_cast<const float4*>(anext);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0.x, fa.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1.x, fa.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0.y, fa.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1.y, fa.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0.z, fa.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1.z, fa.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(b0.w, fa.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b1.w, fa.w, acc1, 0, 0, 0);
      fa = nfa;
      b0 = nb0;
      b1 = nb1;
    }
  }
  // ---- epilogue.  D layout: col = lane & 31 -> pixel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> output channel (+ 32 for acc1)
  const int oy = ho0 + ty, ox = wo0 + tx;
  if (oy < a.Ho && ox < a.Wo) {
    float* o = a.y + a.out_coff + ((long)(n * a.Ho + oy) * a.Wo + ox) * a.out_cstride + 4 * khalf;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv0 = *reinterpret_cast<const float4*>(&sbias[8 * g + 4 * khalf]);
      const float4 bv1 = *reinterpret_cast<const float4*>(&sbias[32 + 8 * g + 4 * khalf]);
      float4 v0 = make_float4(acc0[4 * g] + bv0.x, acc0[4 * g + 1] + bv0.y, acc0[4 * g + 2] + bv0.z, acc0[4 * g + 3] + bv0.w);
      float4 v1 = make_float4(acc1[4 * g] + bv1.x, acc1[4 * g + 1] + bv1.y, acc1[4 * g + 2] + bv1.z, acc1[4 * g + 3] + bv1.w);
      v0.x = v0.x > 0.f ? v0.x : v0.x * a.slope; v0.y = v0.y > 0.f ? v0.y : v0.y * a.slope;
      v0.z = v0.z > 0.f ? v0.z : v0.z * a.slope; v0.w = v0.w > 0.f ? v0.w : v0.w * a.slope;
      v1.x = v1.x > 0.f ? v1.x : v1.x * a.slope; v1.y = v1.y > 0.f ? v1.y : v1.y * a.slope;
      v1.z = v1.z > 0.f ? v1.z : v1.z * a.slope; v1.w = v1.w > 0.f ? v1.w : v1.w * a.slope;
      *reinterpret_cast<float4*>(o + 8 * g) = v0;
      *reinterpret_cast<float4*>(o + 32 + 8 * g) = v1;
    }
  }
}

// flow_conv1 on the bf16 pipe: PERSISTENT workgroups, the whole weight array and the input patches in LDS.  With 16x the matrix rate
// this layer is pure HBM traffic -- 157 MB of input, 315 MB of output at B = 16 = ~95 us -- and the gathered-tap kernel
// (conv_bf16_kernel<64,64,2,2,true>: 13 K chunks per workgroup, the 49 taps re-gathered 3.7x through the 64 B/clk vector memory path)
// took 0.28 ms.  A one-to-one twin of conv1_halo_kernel (weights per tap from L2, one block per workgroup) took 0.25 ms: without f32
// MFMAs to hide under, every wave streaming the 53 KB of weights from L2 (1.9 GB per launch) is the bound.  So: one 8-wave workgroup per
// CU keeps the bf16 image of the packed [chunk][64][32] weights in LDS (80-byte rows: conflict-free ds_read_b128) and walks a
// contiguous range of 16 x 16 pixel blocks; a block's 37 x 37 x 8 patch is loaded ONCE, rounded to bf16 on the way into LDS (16 B per
// pixel, two buffers), the next block's loads are in flight while this one multiplies, one barrier per block.  Roles as in
// conv1_halo_kernel (weights = the A operand, pixels = B: 8 float4 stores per lane); one v_mfma_f32_32x32x16_bf16 multiplies TWO taps:
// lane half h supplies tap 2 i + h, for the weights the 16 bytes k = 16 s + 8 h + {0..7} of chunk i / 2 (tap 49 = the zero padding
// of chunk 12; its pixel operand re-reads tap 48: finite, multiplied by zero).
template <int KH, int KW>
__global__ __launch_bounds__(512) void conv1_halo_bf16_kernel(ConvArgs a, int tiles, int per_wg) {
  constexpr int TH = 16, TW = 16, S = 2;
  constexpr int PH = (TH - 1) * S + KH, PW = (TW - 1) * S + KW;   // 37 x 37 input pixels
  constexpr int NPIX = PH * PW, NT = KH * KW, NPAIR = (NT + 1) / 2, NCH = (NT + 3) / 4;
  constexpr int WROW = 40;                                         // bf16 elements per weight row in LDS (32 + 8 pad)
  constexpr int ITEMS = (NPIX + 511) / 512;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16* sw = reinterpret_cast<__bf16*>(smem);                    // [NCH * 64][WROW]
  bf16x8* patch = reinterpret_cast<bf16x8*>(sw + NCH * 64 * WROW);  // [2][NPIX]
  // the bias too: a vector load in the epilogue would sit behind the next block's patch loads and this block's stores in the one
  // in-order vector-memory counter (measured: 0.45 ms for the layer, every block waiting for its own stores to land)
  __shared__ __attribute__((aligned(16))) float sbias[64];
  if (threadIdx.x < 64) sbias[threadIdx.x] = a.has_bias ? a.bias[threadIdx.x] : 0.f;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = wg_xcd_contiguous((int)blockIdx.x, (int)gridDim.x);   // neighbouring block ranges (shared halos) on one XCD
  const int t_begin = wg * per_wg, t_end = min(tiles, t_begin + per_wg);
  if (t_begin >= t_end) return;
  const int tiles_w = (a.Wo + TW - 1) / TW, tiles_h = (a.Ho + TH - 1) / TH;

  // ---- weights -> LDS, once: rows of 64 bytes, four 16-byte pieces each
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.w_bytes, 0x00020000);
  for (int it = tid; it < NCH * 64 * 4; it += 512) {
    const int row = it >> 2, piece = it & 3;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, (row * 32 + piece * 8) * 2, 0, 0);
    *reinterpret_cast<u32x4*>(sw + row * WROW + piece * 8) = v;
  }
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  float4 lo[ITEMS], hi[ITEMS];
  auto tile_origin = [&](int t, int& n, int& ho0, int& wo0) {
    const int twi = t % tiles_w;
    const int r = t / tiles_w;
    n = r / tiles_h;
    ho0 = (r - n * tiles_h) * TH;
    wo0 = twi * TW;
  };
  auto patch_load = [&](int t) {   // ITEMS x 2 loads in flight per thread; pixels outside the image read zeros (= the padding)
    int n, ho0, wo0;
    tile_origin(t, n, ho0, wo0);
    const int hi0 = ho0 * S - a.pad_h, wi0 = wo0 * S - a.pad_w;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int pix = it * 512 + tid;
      const int py = pix / PW, px = pix - py * PW;
      const int hy = hi0 + py, wx = wi0 + px;
      const bool ok = pix < NPIX && (unsigned)hy < (unsigned)a.H && (unsigned)wx < (unsigned)a.W;
      const int off = ok ? (((n * a.H + hy) * a.W + wx) * a.in_cstride) * 4 : -1;
      lo[it] = buf_load16(rx, off, 0);
      hi[it] = buf_load16(rx, ok ? off + 16 : -1, 0);
    }
  };
  auto patch_store = [&](int buf) {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int pix = it * 512 + tid;
      if (pix < NPIX) {
        const bf16x4 l = to_bf16x4(lo[it]), h = to_bf16x4(hi[it]);
        bf16x8 v = {l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
        patch[buf * NPIX + pix] = v;
      }
    }
  };
  const int frow = lane & 31, khalf = lane >> 5;
  const int p = wave * 32 + frow;               // output pixel = this lane's B column inside the block
  const int ty = p / TW, tx = p - ty * TW;
  const int b_off = (ty * S) * PW + tx * S;
  const __bf16* wbase = sw + frow * WROW + 8 * khalf;

  patch_load(t_begin);
  patch_store(0);
  __syncthreads();
  int buf = 0;
  for (int t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;
    if (more) patch_load(t + 1);
    const bf16x8* pb = patch + buf * NPIX + b_off;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
      const int t0 = 2 * i, t1 = (2 * i + 1 < NT) ? 2 * i + 1 : NT - 1;
      const int o0 = (t0 / KW) * PW + t0 % KW, o1 = (t1 / KW) * PW + t1 % KW;   // constants after unrolling
      const bf16x8 px = pb[khalf ? o1 : o0];
      const __bf16* wr = wbase + ((i >> 1) * 64) * WROW + (i & 1) * 16;
      const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(wr);
      const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(wr + 32 * WROW);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, px, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, px, acc1, 0, 0, 0);
    }
    // ---- epilogue: as conv1_halo_kernel.  D layout: col = lane & 31 -> pixel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> channel
    int n, ho0, wo0;
    tile_origin(t, n, ho0, wo0);
    const int oy = ho0 + ty, ox = wo0 + tx;
    if (oy < a.Ho && ox < a.Wo) {
      float* o = a.y + a.out_coff + ((long)(n * a.Ho + oy) * a.Wo + ox) * a.out_cstride + 4 * khalf;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bv0 = *reinterpret_cast<const float4*>(&sbias[8 * g + 4 * khalf]);
        const float4 bv1 = *reinterpret_cast<const float4*>(&sbias[32 + 8 * g + 4 * khalf]);
        float4 v0 = make_float4(acc0[4 * g] + bv0.x, acc0[4 * g + 1] + bv0.y, acc0[4 * g + 2] + bv0.z, acc0[4 * g + 3] + bv0.w);
        float4 v1 = make_float4(acc1[4 * g] + bv1.x, acc1[4 * g + 1] + bv1.y, acc1[4 * g + 2] + bv1.z, acc1[4 * g + 3] + bv1.w);
        v0.x = v0.x > 0.f ? v0.x : v0.x * a.slope; v0.y = v0.y > 0.f ? v0.y : v0.y * a.slope;
        v0.z = v0.z > 0.f ? v0.z : v0.z * a.slope; v0.w = v0.w > 0.f ? v0.w : v0.w * a.slope;
        v1.x = v1.x > 0.f ? v1.x : v1.x * a.slope; v1.y = v1.y > 0.f ? v1.y : v1.y * a.slope;
        v1.z = v1.z > 0.f ? v1.z : v1.z * a.slope; v1.w = v1.w > 0.f ? v1.w : v1.w * a.slope;
        // plain stores: a lane's eight 16-byte pieces of a pixel's 256-byte row meet in L2 (non-temporal ones went out as 32-byte
        // fragments: 0.45 ms for the layer)
        *reinterpret_cast<float4*>(o + 8 * g) = v0;
        *reinterpret_cast<float4*>(o + 32 + 8 * g) = v1;
      }
    }
    if (more) patch_store(buf ^ 1);   // the other buffer: its last readers passed the barrier that ended the previous block
    __syncthreads();
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------- first layer, three terms
// flow_conv1 with f32 operands on the bf16 matrix pipe: every weight and every input value is the exact sum of three bf16 terms and a
// product keeps the six largest term products, accumulated in f32 -- the arithmetic of wino_gemm_split.hip (error <= 3 * 2^-27 per
// product, below f32's own rounding of the sum; pinned by tests/test_gpu_split_conv1.py: one packed chunk of taps at a time, every
// output against float64 in units of its sum |x w|).  On the f32 pipe this layer is bound by its 392 MFMAs of 64 cycles per 32 x 64 block
// (conv1_halo_kernel: 0.60 ms at 16 pairs, 102 TFLOP/s); six MFMAs of 32 cycles per tap pair are 2.2x fewer pipe cycles.
// The three-term weights of all 64 output channels (150 KB) do not fit LDS beside a patch, and streamed per wave from L2 they are the
// bound (conv1_halo_bf16_kernel's note).  So a PERSISTENT 8-wave workgroup owns HALF the output channels: its 76.8 KB of weights stay in
// LDS, [tap pair 25][term 3][k half 2][channel 32][8 bf16] (a wave's A fragment = 1 KB contiguous, conflict-free), and it walks a range
// of 16 x 16 pixel blocks whose 37 x 37 x 8 patch is split on the way into LDS: three images of 16 B per pixel, the even and the odd
// input columns in separate planes with a 24-slot row pitch -- with stride 2 the 16 lanes that ds_read_b128 serves together read one
// tap of 16 consecutive output pixels = 16 consecutive slots of one column parity (two rows apart: 48 slots = a multiple of the 16
// slots the 64 banks hold) -- conflict-free.  The workgroups 2 j and 2 j + 1 (one XCD) walk the same blocks for the two channel halves:
// the second read of a patch comes out of L2.  One wave = 32 pixels x 32 channels, 150 MFMAs per block on two accumulators.
#ifndef DIM_C1_EXP   // timing experiments on conv1_halo_split_kernel (tools/split_exp.sh FILE=conv_first.hip): 1 no MFMAs, 2 no fragment reads,
#define DIM_C1_EXP 0 // 4 no patch split / store, 8 no output stores -- WRONG results with any bit set
#endif

struct C1Split {
  uint4 h, m, l;
};
__device__ __forceinline__ C1Split c1_split8(const float4 lo, const float4 hi) {
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  const f32x8 x = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const bf16x8 bh = __builtin_convertvector(x, bf16x8);
  const f32x8 r1 = x - __builtin_convertvector(bh, f32x8);
  const bf16x8 bm = __builtin_convertvector(r1, bf16x8);
  const f32x8 r2 = r1 - __builtin_convertvector(bm, f32x8);
  const bf16x8 bl = __builtin_convertvector(r2, bf16x8);
  C1Split s;
  s.h = __builtin_bit_cast(uint4, bh);
  s.m = __builtin_bit_cast(uint4, bm);
  s.l = __builtin_bit_cast(uint4, bl);
  return s;
}

// packed f32 weights [13 chunks][64][4 taps x 8 channels] -> the three-term image (layout above); one thread per (channel, tap slot)
__global__ __launch_bounds__(256) void conv1_split_weights_kernel(const float* __restrict__ wp, unsigned char* __restrict__ w3) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 64 * 2 * kC1Pairs) return;
  const int co = t & 63, slot = t >> 6;   // slot = 2 pair + k half = the tap (49 = padding)
  float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
  if (slot < 49) {
    const float* src = wp + ((slot >> 2) * 64 + co) * 32 + (slot & 3) * 8;
    lo = *reinterpret_cast<const float4*>(src);
    hi = *reinterpret_cast<const float4*>(src + 4);
  }
  const C1Split sp = c1_split8(lo, hi);
  const int pair = slot >> 1, kh = slot & 1, half = co >> 5;
  unsigned char* dst = w3 + ((((size_t)(half * kC1Pairs + pair) * 3) * 2 + kh) * 32 + (co & 31)) * 16;
  *reinterpret_cast<uint4*>(dst) = sp.h;
  *reinterpret_cast<uint4*>(dst + 1024) = sp.m;
  *reinterpret_cast<uint4*>(dst + 2048) = sp.l;
}

template <int KH, int KW>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv1_halo_split_kernel(ConvArgs a, const unsigned char* __restrict__ w3, int tiles, int per_pair) {
  constexpr int TH = 16, TW = 16, S = 2;
  constexpr int PH = (TH - 1) * S + KH, PW = (TW - 1) * S + KW;   // 37 x 37 input pixels
  constexpr int NPIX = PH * PW, NT = KH * KW, NPAIR = (NT + 1) / 2;
  constexpr int PITCH = 24;                  // 16-byte slots per patch row of one column parity (19 used)
  constexpr int PLANE = PH * PITCH;          // slots of one parity plane
  constexpr int TERM = 2 * PLANE;            // slots of one term's image
  constexpr int ITEMS = (NPIX + 511) / 512;
  constexpr int WBYTES = NPAIR * 3 * 2 * 32 * 16;
  static_assert(NPAIR == kC1Pairs, "7 x 7 taps");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_c1[];
  unsigned char* sw = smem_c1;                       // this half's weights
  uint4* sp = reinterpret_cast<uint4*>(smem_c1 + WBYTES);   // [3 terms][2 parities][PH][PITCH]
  float* sbias = reinterpret_cast<float*>(smem_c1 + WBYTES + 3 * TERM * 16);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = wg_xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
  const int half = wg & 1, pr = wg >> 1;
  const int t_begin = pr * per_pair, t_end = min(tiles, t_begin + per_pair);
  if (t_begin >= t_end) return;
  const int tiles_w = (a.Wo + TW - 1) / TW, tiles_h = (a.Ho + TH - 1) / TH;
  if (tid < 32) sbias[tid] = a.has_bias ? a.bias[half * 32 + tid] : 0.f;

  for (int it = tid; it < WBYTES / 16; it += 512)
    *reinterpret_cast<uint4*>(sw + it * 16) = *reinterpret_cast<const uint4*>(w3 + (size_t)half * WBYTES + it * 16);

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  float4 lo[ITEMS], hi[ITEMS];
  auto tile_origin = [&](int t, int& n, int& ho0, int& wo0) {
    const int twi = t % tiles_w;
    const int r = t / tiles_w;
    n = r / tiles_h;
    ho0 = (r - n * tiles_h) * TH;
    wo0 = twi * TW;
  };
  auto patch_load = [&](int t) {   // pixels outside the image read zeros (= the padding)
    int n, ho0, wo0;
    tile_origin(t, n, ho0, wo0);
    const int hi0 = ho0 * S - a.pad_h, wi0 = wo0 * S - a.pad_w;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int pix = it * 512 + tid;
      const int py = pix / PW, px = pix - py * PW;
      const int hy = hi0 + py, wx = wi0 + px;
      const bool ok = pix < NPIX && (unsigned)hy < (unsigned)a.H && (unsigned)wx < (unsigned)a.W;
      const int off = ok ? (((n * a.H + hy) * a.W + wx) * a.in_cstride) * 4 : -1;
      lo[it] = buf_load16(rx, off, 0);
      hi[it] = buf_load16(rx, ok ? off + 16 : -1, 0);
    }
  };
  // the split of the next block's pixels happens in registers while this block multiplies (the VALU work hides under the MFMAs of the
  // SIMD's other wave); after the barrier that ends the block only the LDS stores are left
  C1Split s3[ITEMS];
  auto patch_split = [&]() {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) s3[it] = c1_split8(lo[it], hi[it]);
  };
  auto patch_store = [&]() {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int pix = it * 512 + tid;
      if (pix < NPIX) {
        const int py = pix / PW, px = pix - py * PW;
        const int slot = (px & 1) * PLANE + py * PITCH + (px >> 1);
        sp[slot] = s3[it].h;
        sp[TERM + slot] = s3[it].m;
        sp[2 * TERM + slot] = s3[it].l;
      }
    }
  };
  const int frow = lane & 31, khalf = lane >> 5;
  const int p = wave * 32 + frow;               // output pixel = this lane's B column inside the block
  const int ty = p / TW, tx = p - ty * TW;
  const uint4* pb = sp + (ty * S) * PITCH + tx;
  const unsigned char* wa = sw + (khalf * 32 + frow) * 16;

  // stores through a descriptor: a pixel outside the output gets offset 0xFFFFFFFF, which the range check drops -- no branch around
  // the stores (with one, hipcc waits vmcnt(0) for the next block's patch loads and thereby for these stores: one in-order counter)
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y_bytes, 0x00020000);
  // (Measured and not kept, same-box A/B: the split dealt in fifteen steps behind the MFMAs of tap pairs 8 .. 22 and the outputs of a
  // block written during the next block's first four pairs -- 379 / 383 us against 368 / 397: inside the noise.)
  // (Measured and not kept: different orders for the two waves of a SIMD -- waves 4 .. 7 splitting late in the tap loop and writing their
  // outputs during the next block's first taps -- 407 us against 363: the wave-uniform branches inside the unrolled tap loop cost more
  // than the overlap returned.  Ablations of this form at 16 pairs: MFMAs 200 us of the 363, fragment reads 75, patch split + store 52,
  // output 46, roughly additive: the eight waves of the one workgroup a CU holds move through a block in step.)
  auto epilogue = [&](const f32x16& sum, int tt) {
    // D layout: col = lane & 31 -> pixel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> channel of this half
    int n, ho0, wo0;
    tile_origin(tt, n, ho0, wo0);
    const int oy = ho0 + ty, ox = wo0 + tx;
    const int o_off = (oy < a.Ho && ox < a.Wo) ? (a.out_coff + ((n * a.Ho + oy) * a.Wo + ox) * a.out_cstride + half * 32 + 4 * khalf) * 4 : -1;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = *reinterpret_cast<const float4*>(&sbias[8 * g + 4 * khalf]);
      float4 v = make_float4(sum[4 * g] + bv.x, sum[4 * g + 1] + bv.y, sum[4 * g + 2] + bv.z, sum[4 * g + 3] + bv.w);
      v.x = v.x > 0.f ? v.x : v.x * a.slope; v.y = v.y > 0.f ? v.y : v.y * a.slope;
      v.z = v.z > 0.f ? v.z : v.z * a.slope; v.w = v.w > 0.f ? v.w : v.w * a.slope;
      u32x4 u;
      u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y); u.z = __float_as_uint(v.z); u.w = __float_as_uint(v.w);
      if constexpr (DIM_C1_EXP & 8) asm volatile("" ::"v"(u)); else
      __builtin_amdgcn_raw_buffer_store_b128(u, ry, o_off == -1 ? -1 : o_off + 32 * g, 0, 0);
    }
  };
  patch_load(t_begin);
  patch_split();
  patch_store();
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const bool more = t + 1 < t_end;
    patch_load(more ? t + 1 : t);
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    // fragments of tap pair i + 1 are requested before the six MFMAs of pair i are issued (two register sets; fenced, or hipcc sinks
    // every read to its first use; a third set changed nothing)
    bf16x8 fx[2][3], fw[2][3];
    auto frags = [&](auto I_, auto SET_) {
      constexpr int i = decltype(I_)::value, set = decltype(SET_)::value;
      constexpr int t0 = 2 * i, t1 = (2 * i + 1 < NT) ? 2 * i + 1 : NT - 1;   // tap 49: zero weights, its pixel operand re-reads tap 48
      constexpr int o0 = ((t0 % KW) & 1) * PLANE + (t0 / KW) * PITCH + ((t0 % KW) >> 1);
      constexpr int o1 = ((t1 % KW) & 1) * PLANE + (t1 / KW) * PITCH + ((t1 % KW) >> 1);
      const uint4* ppx = pb + (khalf ? o1 : o0);
      const unsigned char* wr = wa + i * 3 * 1024;
#pragma unroll
      for (int tm = 0; tm < 3; ++tm) {
        fx[set][tm] = __builtin_bit_cast(bf16x8, ppx[tm * TERM]);
        fw[set][tm] = *reinterpret_cast<const bf16x8*>(wr + tm * 1024);
      }
    };
    frags(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    static_for<NPAIR>([&](auto I_) {
      constexpr int i = decltype(I_)::value, set = i & 1;
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (i + 1 < NPAIR && !(DIM_C1_EXP & 2)) frags(std::integral_constant<int, i + 1>{}, std::integral_constant<int, 1 - set>{});
      __builtin_amdgcn_sched_barrier(0);
#if DIM_C1_EXP & 1   // timing experiment: no MFMAs, the operands stay loaded
#pragma unroll
      for (int tm = 0; tm < 3; ++tm) asm volatile("" ::"v"(fw[set][tm]), "v"(fx[set][tm]));
#else
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][2], fx[set][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][0], fx[set][2], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][1], fx[set][1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][1], fx[set][0], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][0], fx[set][1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[set][0], fx[set][0], acc1, 0, 0, 0);
#endif
      if constexpr (i == NPAIR / 2 && !(DIM_C1_EXP & 4)) patch_split();   // the loads were issued a dozen tap pairs ago
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] += acc1[r];
    epilogue(acc0, t);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave has read this block's patch (LDS-only barrier)
    if constexpr (!(DIM_C1_EXP & 4)) patch_store();             // (after the last block: the same block again, unused)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

int launch_conv1_split_weights(float* w_packed, hipStream_t st) {
  hipLaunchKernelGGL(conv1_split_weights_kernel, dim3((64 * 2 * kC1Pairs + 255) / 256), dim3(256), 0, st, w_packed,
                     reinterpret_cast<unsigned char*>(w_packed + 13 * 32 * 64));
  return check_launch("conv1_split_weights");
}

int launch_conv_first(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st) {
  const int N = a.N, Cin = a.Cin, Cout = a.Cout, KH = a.KH, KW = a.KW, stride = a.stride;
  // the LDS-halo first-layer kernel (conv1_halo_kernel): 8 channels, 7x7 / stride 2, 64 output channels, dense output, no split-K
  DIM_REQUIRE(Cin == 8 && KH == 7 && KW == 7 && stride == 2 && Cout == 64, "tile 6 is the 8-channel 7x7 / stride-2 / 64-filter first layer");
  DIM_REQUIRE(splits == 1 && batch == 1 && a.dense_out && !a.accumulate && !partial_only, "tile 6: dense single-launch output only");
  const int tiles = N * ((a.Ho + 7) / 8) * ((a.Wo + 15) / 16);
  DIM_REQUIRE(a.out_cstride % 4 == 0 && a.out_coff % 4 == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0,
              "tile 6 stores float4: output channel stride / offset must be multiples of 4 and y 16-byte aligned");
  if (a.bf16) {  // persistent: one 8-wave workgroup per CU walks a contiguous range of 16 x 16 blocks
    const int tiles16 = N * ((a.Ho + 15) / 16) * ((a.Wo + 15) / 16);
    const int n_cu = device_cu_count();
    const int wgs = tiles16 < n_cu ? tiles16 : n_cu;
    const int per_wg = (tiles16 + wgs - 1) / wgs;
    constexpr size_t lds = (size_t)13 * 64 * 40 * 2 + 2 * (size_t)37 * 37 * 16;
    DIM_REQUIRE((reserve_lds<&conv1_halo_bf16_kernel<7, 7>>(lds)) == DIM_OK, "cannot reserve %zu bytes of LDS for the first-layer kernel", lds);
    hipLaunchKernelGGL((conv1_halo_bf16_kernel<7, 7>), dim3((tiles16 + per_wg - 1) / per_wg), dim3(512), lds, st, a, tiles16, per_wg);
  } else if (wino_get_split()) {  // three-term arithmetic: persistent, one 8-wave workgroup per CU, channel halves in pairs
    const int tiles16 = N * ((a.Ho + 15) / 16) * ((a.Wo + 15) / 16);
    const int n_cu = device_cu_count();
    const int pairs = tiles16 < n_cu / 2 ? tiles16 : n_cu / 2;
    const int per_pair = (tiles16 + pairs - 1) / pairs;
    constexpr size_t lds = (size_t)kC1Pairs * 3 * 2 * 32 * 16 + 3 * 2 * (size_t)37 * 24 * 16 + 32 * sizeof(float);
    DIM_REQUIRE((reserve_lds<&conv1_halo_split_kernel<7, 7>>(lds)) == DIM_OK, "cannot reserve %zu bytes of LDS for the first-layer kernel", lds);
    hipLaunchKernelGGL((conv1_halo_split_kernel<7, 7>), dim3(2 * ((tiles16 + per_pair - 1) / per_pair)), dim3(512), lds, st, a,
                       reinterpret_cast<const unsigned char*>(a.w + 13 * 32 * 64), tiles16, per_pair);
  } else {
    hipLaunchKernelGGL((conv1_halo_kernel<7, 7>), dim3(tiles), dim3(256), 0, st, a);
  }
  return check_launch("conv1_halo");
}

}  // namespace dim
