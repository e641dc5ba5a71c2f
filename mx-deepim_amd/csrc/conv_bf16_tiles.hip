// The bf16 LDS-halo and patch kernels, tiles 7 and 9 (source map: conv_impl.h)
#include "conv_impl.h"

namespace dim {

// ---------------------------------------------------------------------------------------------------------------- bf16, LDS halo
// The bf16 form of the large-map layers from an LDS-resident input patch (tile 7).  conv_bf16_kernel re-gathers its A tile from L2
// for EVERY tap (10.7 GB of L2 -> LDS traffic per forward at B = 16) and has 4 MFMAs of work per barrier, which leaves every layer
// at 0.11-0.24 of its bound once the matrix pipe is 16x faster.  Here a workgroup (4 waves, 64 pixels x 64 channels each) owns an
// 8 x 16 block of output pixels x 128 output channels; per 32-channel slice it stages the ((8-1) S + K) x ((16-1) S + K) input
// patch once (f32 -> bf16 on the way in, zeros outside the image = the padding) and then walks the K x K taps: the A fragments of a
// tap are ds_read_b128 at an immediate offset into the patch, the B tile of a tap (128 channels x 32 k, 8 KB of the packed bf16
// weights: one contiguous block) is staged through LDS two taps at a time, double buffered, so a barrier pair frames 16 MFMAs per
// wave and the activations leave L2 once per slice instead of once per tap.  Dense output only (forward layers and the stride-1
// input gradients); everything else stays on conv_bf16_kernel.
template <int KH, int S>
__global__ __launch_bounds__(256) void conv_bf16_halo_kernel(ConvArgs a) {
  constexpr int KW = KH, TAPS = KH * KW;
  constexpr int TH = 8, TW = 16, BN = 128;
  constexpr int PH = (TH - 1) * S + KH, PW = (TW - 1) * S + KW, NPIX = PH * PW;
  constexpr int PSE = 40;                        // bf16 elements per patch pixel / per weight row: 32 + 8 pad (80 B)
  constexpr int STEPS = (TAPS + 1) / 2;          // taps are processed two per barrier pair (the last step of a slice holds one)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16* patch = reinterpret_cast<__bf16*>(smem);             // [NPIX][PSE]
  __bf16* sB = patch + ((NPIX * PSE + 7) / 8) * 8;             // [2 buffers][2 taps][BN][PSE]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_w = (a.Wo + TW - 1) / TW, tiles_h = (a.Ho + TH - 1) / TH;
  const int ntn = a.Cout / BN;
  int id = blockIdx.x;
  const int n0 = (id % ntn) * BN;                // output-channel tiles fastest: the workgroups sharing a patch are adjacent
  id /= ntn;
  const int twi = id % tiles_w;
  id /= tiles_w;
  const int thi = id % tiles_h;
  const int n = id / tiles_h;
  const int ho0 = thi * TH, wo0 = twi * TW;
  const int hi0 = ho0 * S - a.pad_h, wi0 = wo0 * S - a.pad_w;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.w_bytes, 0x00020000);

  // ---- weights: tap t of slice cc is packed chunk cc * TAPS + t; this workgroup's 128 rows of it are 8 KB contiguous.
  // thread -> 2 x 16 B of a tap (row = idx / 4, 16-byte segment = idx % 4)
  const int wrow0 = tid >> 2, wseg = tid & 3;
  const int w_voff0 = ((n0 + wrow0) * 32 + wseg * 8) * 2, w_voff1 = w_voff0 + 64 * 32 * 2;
  const int w_lds0 = wrow0 * PSE + wseg * 8, w_lds1 = w_lds0 + 64 * PSE;
  u32x4 wr[2][2];  // [tap of the step][half]
  const int chunk_bytes = a.Cout * 32 * 2;
  auto load_w = [&](int chunk_first, int ntaps, bool ok) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bool live = ok && t < ntaps;
      const int soff = live ? (chunk_first + t) * chunk_bytes : 0;
      wr[t][0] = __builtin_amdgcn_raw_buffer_load_b128(rw, live ? w_voff0 : -1, soff, 0);
      wr[t][1] = __builtin_amdgcn_raw_buffer_load_b128(rw, live ? w_voff1 : -1, soff, 0);
    }
  };
  auto store_w = [&](int buf) {
    __bf16* d = sB + buf * 2 * BN * PSE;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      *reinterpret_cast<u32x4*>(d + t * BN * PSE + w_lds0) = wr[t][0];
      *reinterpret_cast<u32x4*>(d + t * BN * PSE + w_lds1) = wr[t][1];
    }
  };

  // ---- fragments
  const int frow = lane & 31, khalf = lane >> 5;
  const int ty_l = frow >> 4, tx = frow & 15;
  const int a_el = (((4 * wm + ty_l) * S) * PW + tx * S) * PSE + 8 * khalf;   // + (2 i S PW) PSE for MFMA tile i, + tap, + 16 ks
  const int b_el = (64 * wn + frow) * PSE + 8 * khalf;                        // + 32 j PSE, + 16 ks
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nslices = a.Cin / 32;
  constexpr int PITEMS = (NPIX * 8 + 255) / 256;   // float4 per thread and patch slice
  int wbuf = 0;
  load_w(0, TAPS >= 2 ? 2 : 1, true);
  for (int cc = 0; cc < nslices; ++cc) {
    // ---- stage the patch of this channel slice (the previous slice's readers passed the barrier at the end of its last step)
#pragma unroll
    for (int it0 = 0; it0 < PITEMS; it0 += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int item = (it0 + u) * 256 + tid;
        const int pix = item >> 3, q = item & 7;
        const int py = pix / PW, px = pix - py * PW;
        const int hi = hi0 + py, wi = wi0 + px;
        const bool ok = it0 + u < PITEMS && item < NPIX * 8 && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
        v[u] = buf_load16(rx, ok ? (((n * a.H + hi) * a.W + wi) * a.in_cstride + cc * 32 + q * 4) * 4 : -1, 0);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int item = (it0 + u) * 256 + tid;
        if (it0 + u < PITEMS && item < NPIX * 8) *reinterpret_cast<bf16x4*>(patch + (item >> 3) * PSE + (item & 7) * 4) = to_bf16x4(v[u]);
      }
    }
    store_w(wbuf);          // the first step's weights (loaded during the previous slice / before the loop)
    __syncthreads();
    for (int st = 0; st < STEPS; ++st) {
      const int ntaps = (2 * st + 2 <= TAPS) ? 2 : 1;
      // next step's weights in flight under this step's MFMAs (next slice's first step after the last one)
      {
        const int nst = st + 1 < STEPS ? st + 1 : 0;
        const int ncc = st + 1 < STEPS ? cc : cc + 1;
        load_w(ncc * TAPS + 2 * nst, (2 * nst + 2 <= TAPS) ? 2 : 1, ncc < nslices);
      }
      const __bf16* cB = sB + wbuf * 2 * BN * PSE + b_el;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t < ntaps) {
          const int tap = 2 * st + t;
          const int kh = tap / KW, kw = tap - kh * KW;
          const __bf16* pa = patch + a_el + (kh * PW + kw) * PSE;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(pa + (2 * i * S * PW) * PSE + 16 * ks);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(cB + t * BN * PSE + 32 * j * PSE + 16 * ks);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
          }
        }
      }
      if (st + 1 < STEPS) store_w(wbuf ^ 1);   // (the next slice's first step is stored after its patch, above)
      __syncthreads();
      if (st + 1 < STEPS) wbuf ^= 1;
    }
    wbuf ^= 1;
  }

  // ---- epilogue.  D layout: col = lane & 31 -> output channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> pixel of the tile.
  // Branch-free buffer stores (see conv_store_tiles): a pixel outside the map gets offset 0xFFFFFFFF and is dropped.
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.y_bytes, 0x00020000);
  int voff[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int pp = (r & 3) + 8 * (r >> 2) + 4 * khalf;           // 0..31 inside MFMA tile i
      const int oy = ho0 + 4 * wm + 2 * i + (pp >> 4), ox = wo0 + (pp & 15);
      voff[i][r] = (oy < a.Ho && ox < a.Wo) ? (((n * a.Ho + oy) * a.Wo + ox) * a.out_cstride + a.out_coff + n0 + 64 * wn + frow) * 4 : -1;
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float bv = a.has_bias ? a.bias[n0 + 64 * wn + 32 * j + frow] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float old[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        old[r] = a.accumulate ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff[i][r], 128 * j, 0)) : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r] + bv;
        v = (v > 0.f ? v : v * a.slope) + old[r];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- bf16, stride-1 patch
// Tile 9: every stride-1 bf16 convolution with a small rectangular tap set (KH, KW <= 3) on a large map -- the 3x3 forward layers,
// their input gradients, and the stride-1 phase convolutions a stride-2 input gradient or a 4x4 / stride-2 deconvolution splits into
// (2x2, 2x3, 3x2, 3x3 taps, scattered output).  PMC on the kernels above (bf16 training iteration): waves parked on s_waitcnt /
// barriers 60 % of their life, matrix pipe busy 12-26 % -- conv_bf16_kernel moves 12.7 TB/s out of L2 (the gather repeats per
// tap), conv_bf16_halo_kernel awaits its weight tiles and its patch with one step of flight time.  Here
//  * a workgroup (4 waves, 2 x 2) owns a 16 x 16 block of output pixels x 128 output channels, a wave 128 pixels x 64 channels
//    (8 accumulator tiles): 16 MFMAs per tap and k-slice against 8 LDS fragment reads and 4 weight-fragment loads;
//  * the (16+KH-1) x (16+KW-1) input patch of a 32-channel slice lives in LDS (f32 -> bf16 on the way in, zeros outside the image
//    = the padding), double buffered: the next slice's patch is fetched in batches at the first taps of the current slice, each
//    batch converted and stored one tap after the next one was issued -- two taps of flight time, ONE barrier per slice;
//  * the weights never touch LDS: a lane's B fragment is 16 contiguous bytes of the packed bf16 array (chunk = slice * taps + tap),
//    loaded NSETS-1 taps ahead into a rotating register set;
//  * patch rows are 1536 B apart (a multiple of 256 B) and pixels 80 B: a ds_read_b128 lane group ({0-3,12-15,20-27}: two pixel
//    rows of an MFMA tile) then covers all 64 banks exactly once.
template <int KH, int KW, int BN, int S>
__global__ __launch_bounds__(256) void conv_bf16_patch_kernel(ConvArgs a) {
  constexpr int NT = KH * KW;
  // S = 1: 16 x 16 output pixels per workgroup; S = 2 (the stride-2 forward layers): 8 x 16, and the patch keeps the even and the odd
  // input columns of a row in two halves (1536 B apart), so that the 16 pixels of a fragment row -- every second input column --
  // are 80 B apart again and the bank argument below holds for both strides
  constexpr int TH = S == 1 ? 16 : 8, TW = 16;
  constexpr int TMW = TH / 4;                         // 32-pixel MFMA tiles (2 rows x 16) per wave: the wave's TH / 2 rows
  constexpr int TN = BN / 64;                         // 32-channel tiles per wave: BN = 128 (2 x 64 per wave column) or 64 (2 x 32)
  static_assert((BN == 128 || BN == 64) && (S == 1 || S == 2), "channel tile / stride");
  constexpr int PH = (TH - 1) * S + KH, PW = (TW - 1) * S + KW;   // input rows / columns under the block
  constexpr int PXB = 80, HALF = 1536, PITCH = S * HALF, PBUF = PH * PITCH;
  constexpr int NITEM = PH * PW * 8;                 // float4 pieces of one patch slice
  constexpr int PITEMS = (NITEM + 255) / 256;        // per thread
  constexpr int NSETS = NT % 3 == 0 ? 3 : (NT % 4 == 0 ? 4 : (NT % 5 == 0 ? 5 : 2));
  constexpr int PF = NSETS - 1;                      // weight prefetch distance in taps
  constexpr int IPT = (PITEMS + (NT > 1 ? NT - 2 : 0)) / (NT > 1 ? NT - 1 : 1);   // patch pieces fetched per tap (taps 0 .. NT-2)
  static_assert(NT >= 2 && NT % NSETS == 0 && ((PW + S - 1) / S) * PXB <= HALF && IPT * (NT - 1) >= PITEMS, "tap plan");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* patch = reinterpret_cast<char*>(smem);       // [2][PH][PITCH] bytes + 256 B dump slot

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_w = (a.Wo + TW - 1) / TW, tiles_h = (a.Ho + TH - 1) / TH;
  const int ntn = a.Cout / BN;
  int id = blockIdx.x;
  const int n0 = (id % ntn) * BN;   // channel tiles fastest: the workgroups sharing a patch are neighbours in launch order
  id /= ntn;
  const int twi = id % tiles_w;
  id /= tiles_w;
  const int thi = id % tiles_h;
  const int n = id / tiles_h;
  const int ho0 = thi * TH, wo0 = twi * TW;
  const int hi0 = ho0 * S - a.pad_h, wi0 = wo0 * S - a.pad_w;
  const float* xb = a.x + (long)blockIdx.y * a.bx;
  const char* wb = reinterpret_cast<const char*>(a.w) + (long)blockIdx.y * a.bw * 2;
  float* yb = a.y + (long)blockIdx.y * a.by;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wb), 0, a.w_bytes, 0x00020000);
  const int nslices = a.Cin / 32;
  const int chunk_bytes = a.Cout * 64;

  // ---- patch pieces of this thread: global byte offset of slice 0 (-1: outside the image / past the patch), LDS byte offset
  int p_goff[PITEMS], p_loff[PITEMS];
#pragma unroll
  for (int u = 0; u < PITEMS; ++u) {
    const int item = u * 256 + tid;
    const int pix = item >> 3, q = item & 7;
    const int py = pix / PW, px = pix - py * PW;
    const int hi = hi0 + py, wi = wi0 + px;
    const bool ok = item < NITEM && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
    p_goff[u] = ok ? (((n * a.H + hi) * a.W + wi) * a.in_cstride + q * 4) * 4 : -1;
    p_loff[u] = item < NITEM ? py * PITCH + (S == 2 ? (px & 1) * HALF + (px >> 1) * PXB : px * PXB) + q * 8 : -1;
  }

  // ---- fragments (wave (wm, wn): output rows (TH / 2) wm .. + TH / 2, channels (BN / 2) wn .. + BN / 2)
  const int frow = lane & 31, khalf = lane >> 5;
  const int a_off = ((TH / 2) * wm + (frow >> 4)) * S * PITCH + (frow & 15) * PXB + 16 * khalf;   // + 2 i S PITCH, + tap offset, + 32 ks
  const int b_voff = ((n0 + (BN / 2) * wn + frow) * 32 + 8 * khalf) * 2;                      // + 32 j rows, + 16 ks elements
  bf16x8 fb[NSETS][2][TN];  // [set][k-step][channel tile]
  auto load_b = [&](auto SET, int chunk) {
    constexpr int set = decltype(SET)::value;
    const int soff = chunk * chunk_bytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, b_voff + (32 * j * 32 + 16 * ks) * 2, soff, 0);
        fb[set][ks][j] = *reinterpret_cast<bf16x8*>(&v);
      }
  };
  f32x16 acc[TMW][TN];
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- prologue: patch of slice 0 (exposed once), weight sets of taps 0 .. PF-1
  {
    float4 v[PITEMS];
#pragma unroll
    for (int u = 0; u < PITEMS; ++u) v[u] = buf_load16(rx, p_goff[u], 0);
#pragma unroll
    for (int u = 0; u < PITEMS; ++u)
      if (p_loff[u] >= 0) *reinterpret_cast<bf16x4*>(patch + p_loff[u]) = to_bf16x4(v[u]);
  }
  const int last_chunk = a.nchunks - 1;
  if constexpr (PF >= 1) load_b(std::integral_constant<int, 0>{}, 0);
  if constexpr (PF >= 2) load_b(std::integral_constant<int, 1>{}, min(1, last_chunk));
  if constexpr (PF >= 3) load_b(std::integral_constant<int, 2>{}, min(2, last_chunk));
  if constexpr (PF >= 4) load_b(std::integral_constant<int, 3>{}, min(3, last_chunk));
  __syncthreads();

  int buf = 0;
  float4 st[2][IPT];   // two batches of patch pieces in flight
  bf16x8 fa[2][2][TMW];  // [tap parity][k-step][pixel tile]
  auto load_a = [&](auto SET, const char* pc, auto TAP) {
    constexpr int set = decltype(SET)::value, tap = decltype(TAP)::value;
    constexpr int kh = tap / KW, kw = tap - kh * KW;
    constexpr int tap_off = kh * PITCH + (S == 2 ? (kw & 1) * HALF + (kw >> 1) * PXB : kw * PXB);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < TMW; ++i)
        fa[set][ks][i] = *reinterpret_cast<const bf16x8*>(pc + tap_off + 2 * i * S * PITCH + 32 * ks);
  };
  for (int cc = 0; cc < nslices; ++cc) {
    const char* pcur = patch + buf * PBUF + a_off;
    load_a(std::integral_constant<int, 0>{}, pcur, std::integral_constant<int, 0>{});   // tap 0: after the barrier that published this patch
    char* pnext = patch + (buf ^ 1) * PBUF;
    const int next_soff = (cc + 1) * 128;           // byte offset of the next slice's channels
    const bool have_next = cc + 1 < nslices;
    const int g0 = cc * NT;
    static_for<NT>([&](auto T) {
      constexpr int t = decltype(T)::value;
      // One scheduling region per tap.  Program order: patch pieces of batch t (next slice) and the weights of tap t + PF, the A
      // fragments of tap t + 1, the 16 MFMAs of tap t, rounding + LDS stores of batch t - 1.  With one wave per SIMD nothing else
      // fills the matrix pipe while the wave issues loads / LDS traffic / VALU, so the sched_group_barrier sequence below deals
      // them out one small group behind each MFMA (an MFMA holds the issue port 8 of its 32 cycles); without it hipcc either sinks
      // the loads to their first use (prefetch distance gone, one load even inside a branch followed by vmcnt(0)) or, fenced into
      // blocks, leaves the pipe idle during every non-MFMA block (measured: 43 % MFMA-busy inside a wave's life).
      constexpr int NLD = (t < NT - 1 ? (IPT < PITEMS - t * IPT ? IPT : (PITEMS - t * IPT > 0 ? PITEMS - t * IPT : 0)) : 0) + 2 * TN;
      constexpr int NST = t >= 1 ? (IPT < PITEMS - (t - 1) * IPT ? IPT : (PITEMS - (t - 1) * IPT > 0 ? PITEMS - (t - 1) * IPT : 0)) : 0;
      if (t < NT - 1) {
#pragma unroll
        for (int e = 0; e < IPT; ++e) {
          const int u = t * IPT + e;
          if (u < PITEMS) st[t & 1][e] = buf_load16(rx, (have_next && p_goff[u] >= 0) ? p_goff[u] + next_soff : -1, 0);
        }
      }
      load_b(std::integral_constant<int, (t + PF) % NSETS>{}, min(g0 + t + PF, last_chunk));
      if constexpr (t + 1 < NT) load_a(std::integral_constant<int, (t + 1) & 1>{}, pcur, std::integral_constant<int, t + 1>{});
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < TMW; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t & 1][ks][i], fb[t % NSETS][ks][j], acc[i][j], 0, 0, 0);
      if (t >= 1) {
#pragma unroll
        for (int e = 0; e < IPT; ++e) {
          const int u = (t - 1) * IPT + e;
          if (u < PITEMS) {
            char* dst = p_loff[u] >= 0 ? pnext + p_loff[u] : patch + 2 * PBUF + (tid & 31) * 8;
            *reinterpret_cast<bf16x4*>(dst) = to_bf16x4(st[(t - 1) & 1][e]);
          }
        }
      }
      constexpr int NM = 2 * TMW * TN;   // MFMAs of the tap
      static_for<NM>([&](auto Mi) {
        constexpr int m = decltype(Mi)::value;
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                       // one MFMA
        if constexpr (m < NLD) {
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                     // address arithmetic of ...
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                     // ... one global load
        }
        if constexpr (m < 2 * TMW && t + 1 < NT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one A-fragment read
        if constexpr (m >= NM - NST) {
          __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);                     // round one piece ...
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                     // ... and store it
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    // LDS-only barrier: the weight loads of the next taps stay in flight across it (__syncthreads would drain them)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    buf ^= 1;
  }

  // ---- epilogue.  D layout: col = lane & 31 -> output channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> pixel of the MFMA tile.
  // Branch-free: a pixel outside the output is a buffer store at offset 0xFFFFFFFF, which the range check drops.  (Stores inside
  // per-element `if` blocks cost 26 us per workgroup here: hipcc opens every block with s_waitcnt vmcnt(0) -- the bias load is
  // still "pending" at the block boundary -- and on gfx950 vmcnt also counts the stores, so the 128 stores went out one round
  // trip at a time.)
  const int by = blockIdx.y;
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(yb, 0, a.y_bytes, 0x00020000);
  const int oy_base = a.ooy + (by >> 1) * a.boy, ox_base = a.oox + (by & 1) * a.box;
  // this lane's 64 pixel slots: row 8 wm + 2 i + (r >> 3), column 4 khalf + (r & 3) + 8 ((r >> 2) & 1) of the 16 x 16 block; the byte
  // offset is affine in both (channel co of tile j = + 128 j bytes), and a block that lies inside the output needs no per-pixel test
  const int hob = ho0 + (TH / 2) * wm, wob = wo0 + 4 * khalf;
  const int row_b = a.osy * a.OW * a.out_cstride * 4, col_b = a.osx * a.out_cstride * 4;
  const int base_b = (((n * a.OH + hob * a.osy + oy_base) * a.OW + wob * a.osx + ox_base) * a.out_cstride + a.out_coff + n0 + (BN / 2) * wn + frow) * 4;
  const bool inside = ho0 + TH <= a.Ho && wo0 + TW <= a.Wo && ho0 * a.osy + oy_base >= 0 && (ho0 + TH - 1) * a.osy + oy_base < a.OH &&
                      wo0 * a.osx + ox_base >= 0 && (wo0 + TW - 1) * a.osx + ox_base < a.OW;   // workgroup-uniform
  int voff[TMW][16];
#pragma unroll
  for (int i = 0; i < TMW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dr = 2 * i + (r >> 3), dc = (r & 3) + 8 * ((r >> 2) & 1);
      voff[i][r] = base_b + dr * row_b + dc * col_b;
    }
  if (!inside) {
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ho = hob + 2 * i + (r >> 3), wo = wob + (r & 3) + 8 * ((r >> 2) & 1);
        const int oy = ho * a.osy + oy_base, ox = wo * a.osx + ox_base;
        const bool ok = ho < a.Ho && wo < a.Wo && (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
        voff[i][r] = ok ? voff[i][r] : -1;
      }
  }
  float bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) bv[j] = a.has_bias ? a.bias[n0 + (BN / 2) * wn + 32 * j + frow] : 0.f;
  if (a.mask) {   // wave-uniform: the LeakyReLU' of the layer below and its bias gradient, folded in (see ConvArgs.mask)
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.mask) + (long)blockIdx.y * a.by, 0, a.y_bytes, 0x00020000);
    float cs[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      cs[j] = 0.f;
#pragma unroll
      for (int i = 0; i < TMW; ++i) {
        float mk[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) mk[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, voff[i][r], 128 * j, 0));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r] + bv[j];
          v = v > 0.f ? v : v * a.slope;
          v *= mk[r] > 0.f ? 1.f : a.mask_slope;
          cs[j] += voff[i][r] != -1 ? v : 0.f;   // a pixel slot outside the output is not stored and must not count
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
        }
      }
    }
    // the two lane halves hold different pixels of the same channel; then one plain store per (block, wave row, channel): no atomics,
    // the reduce over blocks sums in a fixed order
    float* crow = a.colsum + ((long)a.colsum_row0 + 2L * (blockIdx.x / ntn) + wm) * a.Cout + n0 + (BN / 2) * wn + frow;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float tot = cs[j] + __shfl_xor(cs[j], 32);
      if (khalf == 0) crow[32 * j] = tot;
    }
  } else if (a.accumulate) {   // wave-uniform: out += result (gradients that meet in one buffer)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TMW; ++i) {
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff[i][r], 128 * j, 0));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r] + bv[j];
          v = (v > 0.f ? v : v * a.slope) + old[r];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
        }
      }
  } else {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TMW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r] + bv[j];
          v = v > 0.f ? v : v * a.slope;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, voff[i][r], 128 * j, 0);
        }
  }
}

template <int K, int S>
static int launch_halo16(const ConvArgs& a, int blocks, size_t lds, hipStream_t st) {
  const int rc = reserve_lds<&conv_bf16_halo_kernel<K, S>>(lds);
  if (rc != DIM_OK) return rc;
  hipLaunchKernelGGL((conv_bf16_halo_kernel<K, S>), dim3(blocks), dim3(256), lds, st, a);
  return check_launch("conv_bf16_halo");
}

int launch_conv_bf16_halo(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st) {
  const int N = a.N, Cin = a.Cin, Cout = a.Cout, KH = a.KH, KW = a.KW, stride = a.stride;
  // the bf16 LDS-halo kernel (conv_bf16_halo_kernel): square 3x3 or 5x5 taps, stride 1 or 2, Cin % 32 == 0, Cout % 128 == 0, dense
  DIM_REQUIRE(a.bf16 && KH == KW && (KH == 3 || KH == 5) && (stride == 1 || stride == 2) && Cin % 32 == 0 && Cout % 128 == 0,
              "tile 7: bf16, 3x3 or 5x5, stride 1 or 2, Cin %% 32 == 0, Cout %% 128 == 0");
  DIM_REQUIRE(!(KH == 5 && stride == 1), "tile 7: 5x5 is built for stride 2");
  DIM_REQUIRE(splits == 1 && batch == 1 && a.dense_out && !partial_only, "tile 7: dense single-launch output only");
  const int blocks = N * ((a.Ho + 7) / 8) * ((a.Wo + 15) / 16) * (Cout / 128);
  const int ph = 7 * stride + KH, pw = 15 * stride + KW;
  const size_t lds = (size_t)((ph * pw * 40 + 7) / 8 * 8) * 2 + (size_t)2 * 2 * 128 * 40 * 2;
  if (KH == 3 && stride == 1) return launch_halo16<3, 1>(a, blocks, lds, st);
  if (KH == 3) return launch_halo16<3, 2>(a, blocks, lds, st);
  return launch_halo16<5, 2>(a, blocks, lds, st);
}

template <int KH, int KW, int BN, int S>
static int launch_patch16(const ConvArgs& a, int blocks, int batch, size_t lds, hipStream_t st) {
  const int rc = reserve_lds<&conv_bf16_patch_kernel<KH, KW, BN, S>>(lds);
  if (rc != DIM_OK) return rc;
  hipLaunchKernelGGL((conv_bf16_patch_kernel<KH, KW, BN, S>), dim3(blocks, batch), dim3(256), lds, st, a);
  return check_launch("conv_bf16_patch");
}

int launch_conv_bf16_patch(const ConvArgs& a, int splits, int batch, int partial_only, hipStream_t st) {
  const int N = a.N, Cin = a.Cin, Cout = a.Cout, KH = a.KH, KW = a.KW, stride = a.stride;
  // the bf16 patch kernel (conv_bf16_patch_kernel).  Stride 1: 2 .. 9 taps with KH, KW <= 3, 16 x 16 output pixels x 128 or 64
  // channels per workgroup; stride 2: 3x3 or 5x5, 8 x 16 pixels x 128 channels.  Cin % 32 == 0; dense or scattered output, batched
  // launch (deconvolution phases) allowed, no split-K
  DIM_REQUIRE(a.bf16 && Cin % 32 == 0 && splits == 1 && !partial_only, "tile 9: bf16, Cin %% 32 == 0, no split-K");
  if (stride == 1)
    DIM_REQUIRE(KH >= 1 && KH <= 3 && KW >= 1 && KW <= 3 && KH * KW >= 2 && Cout % 64 == 0,
                "tile 9, stride 1: 2..9 taps (KH, KW <= 3), Cout %% 64 == 0");
  else
    DIM_REQUIRE(stride == 2 && KH == KW && (KH == 3 || KH == 5) && Cout % 128 == 0, "tile 9, stride 2: 3x3 or 5x5, Cout %% 128 == 0");
  const int bn = Cout % 128 == 0 ? 128 : 64;   // 64: the 64-channel layers (input gradient of flow_conv2)
  const int th = stride == 1 ? 16 : 8;
  const int blocks = N * ((a.Ho + th - 1) / th) * ((a.Wo + 15) / 16) * (Cout / bn);
  const size_t lds = (size_t)2 * ((th - 1) * stride + KH) * (1536 * stride) + 256;   // two patch buffers + the dump slot
  if (stride == 2)
    return KH == 5 ? launch_patch16<5, 5, 128, 2>(a, blocks, batch, lds, st) : launch_patch16<3, 3, 128, 2>(a, blocks, batch, lds, st);
#define DIM_PATCH16(KHc, KWc) \
  return bn == 128 ? launch_patch16<KHc, KWc, 128, 1>(a, blocks, batch, lds, st) : launch_patch16<KHc, KWc, 64, 1>(a, blocks, batch, lds, st);
  switch (KH * 4 + KW) {
    case 1 * 4 + 2: DIM_PATCH16(1, 2)
    case 2 * 4 + 1: DIM_PATCH16(2, 1)
    case 1 * 4 + 3: DIM_PATCH16(1, 3)
    case 3 * 4 + 1: DIM_PATCH16(3, 1)
    case 2 * 4 + 2: DIM_PATCH16(2, 2)
    case 2 * 4 + 3: DIM_PATCH16(2, 3)
    case 3 * 4 + 2: DIM_PATCH16(3, 2)
    default: DIM_PATCH16(3, 3)
  }
#undef DIM_PATCH16
}

}  // namespace dim
