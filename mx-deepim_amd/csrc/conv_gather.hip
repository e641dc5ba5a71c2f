// im2col-free direct convolution on the CDNA4 f32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
// Replaces the cuDNN Convolution / FullyConnected calls of the reference's FlowNetS encoder
// (/root/reference/deepim/symbols/deepIM_flownet.py:67-208).  Activations are NHWC fp32 in HBM,
// weights are pre-packed once into [K/32 chunks][Cout][32] (chunk order: 32-channel slice outer, taps inner); implicit GEMM
//     Y[m = (n,ho,wo)][co] = sum_k X[n, ho*s-p+kh, wo*s-p+kw, c] * Wp[k][co]
// with a 32-deep K chunk that is one tap x 32 channels (Cin % 32 == 0) or, for the 8-channel
// first layer, four consecutive taps (flat, row-major over the kernel window) x 8 channels.
// The 3x3 / stride-1 and 5x5 / stride-2 layers normally run in the Winograd domain instead (winograd.hip + wino_gemm.hip).
//
// Block = 4 (or 8) waves; wave tile = (BM/WM) x (BN/WN) in 32x32 MFMA tiles.
// LDS: the A (pixel) chunk [BM][32+4], k-contiguous: staged with one ds_write_b128 per float4 and read back as ds_read_b128 =
//      four k-steps of MFMA operands per LDS instruction; two buffers, software-pipelined (see the loop).  The B operand
//      (weights) never passes through LDS: the packed layout is the fragment layout, every wave loads its own fragments from
//      L2 one chunk ahead (the k order inside a chunk is permuted identically for A and B).
// Epilogue: bias + LeakyReLU fused; with gridDim.z > 1 (split-K) raw partials go to a slab
// and dim_splitk_reduce finishes (deterministic, no atomics).
#include "conv_impl.h"

namespace dim {

template <int BM, int BN, int WM, int WN, bool CIN8>
__global__ __launch_bounds__(WM * WN * 64) void conv_fwd_kernel(ConvArgs a) {
  constexpr int BK = 32;
  constexpr int NT = WM * WN * 64;  // 4 or 8 waves
  constexpr int RP = NT / 8;        // rows staged per pass (8 threads x float4 = one 32-float row)
  constexpr int LDK = BK + 4;       // row stride (floats): 16 rows x 4 dwords hit 16 distinct 4-bank slots for ds_read_b128
  constexpr int TM = BM / WM / 32;  // MFMA tiles per wave along M
  constexpr int TN = BN / WN / 32;
  constexpr int A_PER_T = BM / RP;  // float4 loads per thread for the A chunk
  static_assert((WM * WN == 4 || WM * WN == 8) && A_PER_T >= 1 && A_PER_T <= 4, "staging plan");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                       // [2][BM][LDK]   pixel-major, k contiguous

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // 1-D tile grid, N tiles fastest: the Cout/BN workgroups that share one A (pixel) tile are adjacent.  Workgroups are
  // dealt round-robin to the 8 XCDs (each with its own L2), so with xcd_chunk = tiles/8 the id is remapped such that XCD k
  // walks tiles [k*chunk, (k+1)*chunk) in order: the A tile is fetched into ONE L2 and re-used there by its N tiles, and
  // neighbouring pixel tiles (which share the 3x3 halo rows) follow on the same XCD.
  int id = blockIdx.x + a.tile_off;
  if (a.xcd_chunk > 0) id = (id & 7) * a.xcd_chunk + (id >> 3);
  const int ntiles_n = a.Cout / BN;
  const int mtile = id / ntiles_n;
  const int m0 = mtile * BM;
  const int n0 = (id - mtile * ntiles_n) * BN;
  const int split = blockIdx.z;
  const int kc_begin = split * a.chunks_per_split;
  const int kc_end = min(a.nchunks, kc_begin + a.chunks_per_split);

  // ---- per-thread staging descriptors: thread (q, srow) moves float4 #q of row srow (+32 per pass) for A and for B
  const int q = tid & 7;
  const int srow = tid >> 3;
  int a_hi0[A_PER_T], a_wi0[A_PER_T], a_pix[A_PER_T];
#pragma unroll
  for (int i = 0; i < A_PER_T; ++i) {
    int m = m0 + srow + RP * i;
    bool ok = m < a.M;
    int mm = ok ? m : 0;
    int wo = mm % a.Wo;
    int t = mm / a.Wo;
    int ho = t % a.Ho;
    int n = t / a.Ho;
    a_hi0[i] = ok ? ho * a.stride - a.pad_h : -(1 << 28);  // rows past M: every tap fails the bounds test
    a_wi0[i] = wo * a.stride - a.pad_w;
    // BYTE offset of this thread's float4 at tap (0,0), channel 0 (may be negative in the padding; 32 bits, host-checked).
    // 8-channel layer: a chunk is 4 taps x 8 channels, thread q holds channel half q & 1 of tap q >> 1 (tap offset added per chunk).
    a_pix[i] = ((n * a.H + (ok ? a_hi0[i] : 0)) * a.W * a.in_cstride + (wo * a.stride - a.pad_w) * a.in_cstride + (CIN8 ? (q & 1) * 4 : q * 4)) * 4;
  }
  // Both operands go through buffer descriptors: a padding tap is a load at offset 0xFFFFFFFF (the range check returns
  // zeros: one v_cndmask on a 32-bit offset, no pointer select, no exec juggling, and -- unlike the flat loads a pointer
  // select compiles to -- nothing that counts on lgkmcnt next to the LDS fragment reads); the weights take the chunk as
  // a scalar offset, so their per-lane offset is loop-invariant.
  const float* xb = a.x + (long)blockIdx.y * a.bx;  // blockIdx.y = problem of a batched launch (0 otherwise)
  const float* wb = a.w + (long)blockIdx.y * a.bw;
  float* yb = a.y + (long)blockIdx.y * a.by;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, a.w_bytes, 0x00020000);
  const int wchunk_bytes = a.Cout * BK * 4;  // packed [chunk][Cout][32]

  // chunk -> (kh, kw, c0) counters
  int kh, kw, c0;
  if (CIN8) {
    // 8-channel layer: K = (tap, channel) flattened, 4 taps per chunk, taps numbered row-major over KH x KW with NO padding per
    // kernel row (7x7: 49 taps = 13 chunks instead of the 14 that "two chunks per row" needed).  `kw` holds this thread's flat tap.
    kw = 4 * kc_begin + (q >> 1);
    kh = 0;
    c0 = 0;
  } else {
    // K order for Cin % 32 == 0: 32-channel slice OUTER, taps INNER -- consecutive chunks read the same channels at the
    // (kh,kw)-shifted pixels, i.e. mostly the same cache lines (reuse distance 1 chunk instead of Cin/32 chunks).
    // With taps outer the L2 hit rate of conv3_1 was 50 % (rocprofv3 TCC_HIT/TCC_MISS): every tap re-fetched its
    // activations from beyond L2.
    int taps = a.KH * a.KW;
    int cc = kc_begin / taps;
    int tap = kc_begin - cc * taps;
    c0 = cc << 5;
    kh = tap / a.KW;
    kw = tap - kh * a.KW;
  }

  float4 ra0, ra1, ra2, ra3;  // staging registers of the A chunk, named (arrays + lambdas ended up in scratch)

  // tap_off is wave-uniform (scalar): one vector add per load.  (It cannot ride in the instruction's scalar offset: that
  // one is excluded from the range check, and a_pix alone is negative = out of range in the top/left padding.)
#define DIM_LOAD_A(REG, I)                                                                                         \
  if (I < A_PER_T) {                                                                                                \
    bool ok = pf_ok && (unsigned)(a_hi0[I] + tkh) < (unsigned)a.H && (unsigned)(a_wi0[I] + tkw) < (unsigned)a.W;    \
    REG = buf_load16(rx, ok ? a_pix[I] + tap_off : -1, 0);                                                          \
  }
  // PF_OK = false on the one prefetch past the last chunk: its (kh,kw,c0) counters already point one channel slice beyond
  // the tensor, so the (unused) activation read is dropped like a padding tap
#define DIM_LOAD_CHUNK(PF_OK)                                      \
  {                                                                \
    /* (tkh, tkw) = the tap this thread loads: wave-uniform for the 32-channel layers, per thread (from its flat tap) for the */ \
    /* 8-channel one, where a tap past KH*KW lands on a row >= KH only if the bounds test below rejects it explicitly */ \
    const int tkh = CIN8 ? (int)fastdiv((unsigned)kw, a.div_kw) : kh;                                   \
    const int tkw = CIN8 ? kw - tkh * a.KW : kw;                                                        \
    const bool pf_ok = (PF_OK) && (!CIN8 || tkh < a.KH);           \
    const int tap_off = ((tkh * a.W + tkw) * a.in_cstride + c0) * 4; \
    DIM_LOAD_A(ra0, 0) DIM_LOAD_A(ra1, 1) DIM_LOAD_A(ra2, 2) DIM_LOAD_A(ra3, 3) \
  }
#define DIM_ADVANCE()                        \
  if (CIN8) {                                \
    kw += 4;                                 \
  } else {                                   \
    if (++kw == a.KW) {                      \
      kw = 0;                                \
      if (++kh == a.KH) { kh = 0; c0 += 32; } \
    }                                        \
  }
#define DIM_STORE_A(REG, I) \
  if (I < A_PER_T) *reinterpret_cast<float4*>(dA + (srow + RP * I) * LDK + q * 4) = REG;
#define DIM_STORE_CHUNK(BUF)                          \
  {                                                   \
    float* dA = sA + (BUF) * BM * LDK;                \
    DIM_STORE_A(ra0, 0) DIM_STORE_A(ra1, 1) DIM_STORE_A(ra2, 2) DIM_STORE_A(ra3, 3) \
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment addressing: lane (half h, row r) reads 4 consecutive k = 8s + 4h + {0..3} of its row with one ds_read_b128;
  // MFMA #j of group s then contracts k = 8s + j (lanes 0-31) and k = 8s + 4 + j (lanes 32-63): every k of the chunk
  // is used exactly once, identically for A and B.
  const int frow = lane & 31;
  const int khalf = lane >> 5;
  const int a_off = (wm * (BM / WM) + frow) * LDK + 4 * khalf;
  float4 fa[2][TM];
#define DIM_FRAG_READ(IDX, PA, PB, S)                                                                  \
  {                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[IDX][i] = *reinterpret_cast<const float4*>((PA) + 32 * i * LDK + 8 * (S)); \
  }
  // the weights never pass through LDS: every wave fetches its own B fragments (lane (row n, k half) = 16 contiguous bytes of the
  // packed [chunk][Cout][32] array) one whole chunk ahead; fbq[set][group][tile]
  float4 fbq[2][4][TN];
  const int bf_voff = ((n0 + wn * (BN / WN) + frow) * BK + 4 * khalf) * 4;
#define DIM_LOAD_BFRAG(SET, KC)                                                                         \
  {                                                                                                    \
    const int bsoff = (KC) * wchunk_bytes;                                                             \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) _Pragma("unroll") for (int j = 0; j < TN; ++j)        \
      fbq[SET][g][j] = buf_load16(rw, bf_voff + (32 * j * BK + 8 * g) * 4, bsoff);                      \
  }
#define DIM_MFMA_GROUP(IDX, SET, G)                                                                     \
  {                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) {     \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[IDX][i].x, fbq[SET][G][j].x, acc[i][j], 0, 0, 0); \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[IDX][i].y, fbq[SET][G][j].y, acc[i][j], 0, 0, 0); \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[IDX][i].z, fbq[SET][G][j].z, acc[i][j], 0, 0, 0); \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[IDX][i].w, fbq[SET][G][j].w, acc[i][j], 0, 0, 0); \
    }                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                 \
  }

  // ---- software pipeline (per K chunk of 32 = four MFMA groups g0..g3):
  //   g0 | g1 | [registers -> LDS for chunk k+1, then global loads for chunk k+2] | g2 | barrier | [fragments g0 of chunk k+1] | g3
  // The LDS stores and the barrier sit INSIDE the MFMA sequence and the next chunk's first fragments are in flight during g3, so
  // no wave ever reaches a point with nothing to feed the MFMA pipe.  (With stores + barrier + first fragment read at the chunk
  // boundary the four workgroups of a CU ran in lock step and the pipe idled ~20 % of the time: PMC 74-78 % MFMA-busy.)
  // The barrier only orders LDS traffic (s_waitcnt lgkmcnt(0); s_barrier): __syncthreads() would also wait for the global
  // prefetch that has just been issued.  Hazards: buffer b^1 is written in the middle of chunk k; its last readers were the g3
  // fragments of chunk k-1, which every wave has in registers before it passes that chunk's barrier.
  if (kc_begin < kc_end) {
    DIM_LOAD_CHUNK(true)
    DIM_ADVANCE()
    DIM_STORE_CHUNK(0)
    DIM_LOAD_BFRAG(0, kc_begin)
  }
  __syncthreads();
  DIM_LOAD_CHUNK(kc_begin + 1 < kc_end)
  DIM_ADVANCE()
  DIM_FRAG_READ(0, sA + a_off, 0, 0)

#define DIM_CHUNK_BODY(SET, KCUR)                                                    \
  {                                                                                  \
    const float* cA = sA + buf * BM * LDK + a_off;                                   \
    const float* nA = sA + (buf ^ 1) * BM * LDK + a_off;                             \
    DIM_LOAD_BFRAG(1 - SET, min((KCUR) + 1, a.nchunks - 1))                          \
    DIM_FRAG_READ(1, cA, 0, 1)                                                      \
    DIM_MFMA_GROUP(0, SET, 0)                                                        \
    DIM_FRAG_READ(0, cA, 0, 2)                                                      \
    DIM_MFMA_GROUP(1, SET, 1)                                                        \
    DIM_STORE_CHUNK(buf ^ 1)                                                         \
    DIM_LOAD_CHUNK((KCUR) + 2 < kc_end)                                              \
    DIM_ADVANCE()                                                                    \
    DIM_FRAG_READ(1, cA, 0, 3)                                                      \
    DIM_MFMA_GROUP(0, SET, 2)                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                  \
    DIM_FRAG_READ(0, nA, 0, 0)                                                      \
    DIM_MFMA_GROUP(1, SET, 3)                                                        \
    buf ^= 1;                                                                        \
  }
  int buf = 0;
  for (int kc = kc_begin; kc < kc_end; kc += 2) {
    DIM_CHUNK_BODY(0, kc)
    if (kc + 1 < kc_end) DIM_CHUNK_BODY(1, kc + 1)
  }
#undef DIM_CHUNK_BODY
#undef DIM_LOAD_BFRAG
#undef DIM_FRAG_READ
#undef DIM_MFMA_GROUP
#undef DIM_LOAD_A
#undef DIM_LOAD_CHUNK
#undef DIM_ADVANCE
#undef DIM_STORE_A
#undef DIM_STORE_CHUNK

  // ---- epilogue (conv_store_tiles in conv_impl.h: branch-free buffer stores)
  conv_store_tiles<TM, TN>(a, acc, yb, m0 + wm * (BM / WM) + 4 * khalf, n0 + wn * (BN / WN) + frow, split);
}

// ---------------------------------------------------------------------------------------------------------------- bf16 MFMA
// The same implicit GEMM on v_mfma_f32_32x32x16_bf16 (16x the f32 matrix rate, f32 accumulate): the training mode of BASELINE
// configs[2].  Activations stay fp32 in HBM (every other kernel of the graph reads them); a thread rounds its float4 to four bf16
// (v_cvt_pk_bf16_f32, round to nearest even) on the way into LDS, so the LDS traffic and the fragment reads halve.  Weights are the
// SAME packed [chunk][Cout][32] arrays converted element-wise to bf16 (dim_f32_to_bf16): a lane's B fragment of k-step s is the 16
// contiguous bytes k = 16 s + 8 h + {0..7} of its output channel -- the operand map of the instruction -- straight from L2.
// With the matrix pipe 16x faster every layer is bound by its operand traffic (L2 -> LDS for the gathered A tile): the loop is a
// plain two-buffer pipeline, and occupancy (<= 64 VGPRs at the 64x32 wave tile) does the latency hiding.
template <int BM, int BN, int WM, int WN, bool CIN8>
__global__ __launch_bounds__(WM * WN * 64) void conv_bf16_kernel(ConvArgs a) {
  constexpr int BK = 32;
  constexpr int NT = WM * WN * 64;
  constexpr int RP = NT / 8;        // rows staged per pass (8 threads x float4 = one 32-value row)
  constexpr int LDH = BK + 8;       // row stride in bf16 elements (80 B): 16 rows x 16 B land on 16 distinct 4-bank slots (ds_read_b128)
  constexpr int TM = BM / WM / 32;
  constexpr int TN = BN / WN / 32;
  constexpr int A_PER_T = BM / RP;
  static_assert((WM * WN == 4 || WM * WN == 8) && A_PER_T >= 1 && A_PER_T <= 4, "staging plan");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16* sA = reinterpret_cast<__bf16*>(smem);  // [2][BM][LDH]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  int id = blockIdx.x + a.tile_off;
  if (a.xcd_chunk > 0) id = (id & 7) * a.xcd_chunk + (id >> 3);
  const int ntiles_n = a.Cout / BN;
  const int mtile = id / ntiles_n;
  const int m0 = mtile * BM;
  const int n0 = (id - mtile * ntiles_n) * BN;
  const int split = blockIdx.z;
  const int kc_begin = split * a.chunks_per_split;
  const int kc_end = min(a.nchunks, kc_begin + a.chunks_per_split);

  const int q = tid & 7;
  const int srow = tid >> 3;
  int a_hi0[A_PER_T], a_wi0[A_PER_T], a_pix[A_PER_T];
#pragma unroll
  for (int i = 0; i < A_PER_T; ++i) {
    int m = m0 + srow + RP * i;
    bool ok = m < a.M;
    int mm = ok ? m : 0;
    int wo = mm % a.Wo;
    int t = mm / a.Wo;
    int ho = t % a.Ho;
    int n = t / a.Ho;
    a_hi0[i] = ok ? ho * a.stride - a.pad_h : -(1 << 28);
    a_wi0[i] = wo * a.stride - a.pad_w;
    a_pix[i] = ((n * a.H + (ok ? a_hi0[i] : 0)) * a.W * a.in_cstride + (wo * a.stride - a.pad_w) * a.in_cstride + (CIN8 ? (q & 1) * 4 : q * 4)) * 4;
  }
  const float* xb = a.x + (long)blockIdx.y * a.bx;
  const char* wb = reinterpret_cast<const char*>(a.w) + (long)blockIdx.y * a.bw * 2;  // bw counts elements; bf16 = 2 bytes
  float* yb = a.y + (long)blockIdx.y * a.by;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(wb), 0, a.w_bytes, 0x00020000);
  const int wchunk_bytes = a.Cout * BK * 2;

  int kh, kw, c0;
  if (CIN8) {
    kw = 4 * kc_begin + (q >> 1);
    kh = 0;
    c0 = 0;
  } else {
    int taps = a.KH * a.KW;
    int cc = kc_begin / taps;
    int tap = kc_begin - cc * taps;
    c0 = cc << 5;
    kh = tap / a.KW;
    kw = tap - kh * a.KW;
  }
  float4 ra[A_PER_T];
  auto load_chunk = [&](bool pf) {
    const int tkh = CIN8 ? (int)fastdiv((unsigned)kw, a.div_kw) : kh;
    const int tkw = CIN8 ? kw - tkh * a.KW : kw;
    const bool pf_ok = pf && (!CIN8 || tkh < a.KH);
    const int tap_off = ((tkh * a.W + tkw) * a.in_cstride + c0) * 4;
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) {
      bool ok = pf_ok && (unsigned)(a_hi0[i] + tkh) < (unsigned)a.H && (unsigned)(a_wi0[i] + tkw) < (unsigned)a.W;
      ra[i] = buf_load16(rx, ok ? a_pix[i] + tap_off : -1, 0);
    }
    if (CIN8) {
      kw += 4;
    } else if (++kw == a.KW) {
      kw = 0;
      if (++kh == a.KH) { kh = 0; c0 += 32; }
    }
  };
  auto store_chunk = [&](int buf) {
    __bf16* dA = sA + buf * BM * LDH;
#pragma unroll
    for (int i = 0; i < A_PER_T; ++i) *reinterpret_cast<bf16x4*>(dA + (srow + RP * i) * LDH + q * 4) = to_bf16x4(ra[i]);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31;
  const int khalf = lane >> 5;
  const int a_off = (wm * (BM / WM) + frow) * LDH + 8 * khalf;
  const int bf_voff = ((n0 + wn * (BN / WN) + frow) * BK + 8 * khalf) * 2;
  bf16x8 fb[2][2][TN];  // [set][k-step][tile]
  auto load_bfrag = [&](const int set, int kc) {  // always called with a literal / constexpr set: inlined, indices fold
    const int bsoff = kc * wchunk_bytes;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw, bf_voff + (32 * j * BK + 16 * s) * 2, bsoff, 0);
        fb[set][s][j] = *reinterpret_cast<bf16x8*>(&v);
      }
  };

  if (kc_begin < kc_end) {
    load_chunk(true);
    store_chunk(0);
    load_bfrag(0, kc_begin);
  }
  __syncthreads();
  load_chunk(kc_begin + 1 < kc_end);
  int buf = 0;
  // two chunks per trip so that the B-fragment set (a register array) is indexed by a compile-time constant
  auto chunk_body = [&](auto SET, int kc) {
    constexpr int set = decltype(SET)::value;
    const __bf16* cA = sA + buf * BM * LDH + a_off;
    load_bfrag(set ^ 1, min(kc + 1, a.nchunks - 1));
    bf16x8 fa[2][TM];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[s][i] = *reinterpret_cast<const bf16x8*>(cA + 32 * i * LDH + 16 * s);
    // the staged registers of chunk kc+1 go to the other buffer (its readers finished before the previous barrier), then the
    // loads of chunk kc+2 are issued: they fly over the MFMAs below and the next chunk's
    store_chunk(buf ^ 1);
    load_chunk(kc + 2 < kc_end);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][i], fb[set][s][j], acc[i][j], 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    buf ^= 1;
  };
  for (int kc = kc_begin; kc < kc_end; kc += 2) {
    chunk_body(std::integral_constant<int, 0>{}, kc);
    if (kc + 1 < kc_end) chunk_body(std::integral_constant<int, 1>{}, kc + 1);
  }

  // ---- epilogue (conv_store_tiles in conv_impl.h: branch-free buffer stores)
  conv_store_tiles<TM, TN>(a, acc, yb, m0 + wm * (BM / WM) + 4 * khalf, n0 + wn * (BN / WN) + frow, split);
}

template <int BM, int BN, int WM, int WN, bool CIN8>
static int launch_conv(const ConvArgs& a, int splits, hipStream_t st, int batch = 1, int tile_begin = 0, int tile_count = -1) {
  // A tiles only: the weights go global -> registers.  f32: [2][BM][36] floats; bf16: [2][BM][40] halves
  const size_t lds = a.bf16 ? (size_t)2 * BM * (32 + 8) * 2 : (size_t)2 * BM * (32 + 4) * sizeof(float);
  int rc = reserve_lds<&conv_fwd_kernel<BM, BN, WM, WN, CIN8>>((size_t)2 * BM * (32 + 4) * sizeof(float));   // the f32 kernel only
  if (rc != DIM_OK) return rc;
  const int tiles = ceil_div(a.M, BM) * (a.Cout / BN);
  ConvArgs b = a;
  static const int xcd_mode = getenv("DIM_CONV_XCD") ? atoi(getenv("DIM_CONV_XCD")) : 0;  // experiment switch
  const bool whole = tile_begin == 0 && (tile_count < 0 || tile_count == tiles);
  b.xcd_chunk = (whole && xcd_mode > 0 && tiles % 8 == 0 && tiles >= xcd_mode) ? tiles / 8 : 0;
  b.tile_off = tile_begin;
  dim3 grid(tile_count < 0 ? tiles : tile_count, batch, splits);
  if (a.bf16)
    hipLaunchKernelGGL((conv_bf16_kernel<BM, BN, WM, WN, CIN8>), grid, dim3(WM * WN * 64), lds, st, b);
  else
    hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, WM, WN, CIN8>), grid, dim3(WM * WN * 64), lds, st, b);
  return check_launch("conv_fwd");
}

// bf16-only workgroup tiles (no f32 instantiation): 8 = 128 rows x 256 channels on 8 waves of 64 x 64
template <int BM, int BN, int WM, int WN>
static int launch_conv_bf16(const ConvArgs& a, int splits, hipStream_t st, int batch, int tile_begin, int tile_count) {
  const size_t lds = (size_t)2 * BM * (32 + 8) * 2;
  const int tiles = ceil_div(a.M, BM) * (a.Cout / BN);
  ConvArgs b = a;
  b.xcd_chunk = 0;
  b.tile_off = tile_begin;
  dim3 grid(tile_count < 0 ? tiles : tile_count, batch, splits);
  hipLaunchKernelGGL((conv_bf16_kernel<BM, BN, WM, WN, false>), grid, dim3(WM * WN * 64), lds, st, b);
  return check_launch("conv_bf16");
}

// tile -> instantiation (source map: conv_impl.h); the 8-channel layer has tiles 1 - 3 and no batched launch
int launch_conv_gather(const ConvArgs& args, int tile, int nsplit, hipStream_t st, int batch, int t0, int tn) {
  if (args.Cin == 8) {
    if (tile == 1) return launch_conv<128, 128, 2, 2, true>(args, nsplit, st, 1, t0, tn);
    if (tile == 2) return launch_conv<128, 64, 2, 2, true>(args, nsplit, st, 1, t0, tn);
    return launch_conv<64, 64, 2, 2, true>(args, nsplit, st, 1, t0, tn);
  }
  if (tile == 8) return launch_conv_bf16<128, 256, 2, 4>(args, nsplit, st, batch, t0, tn);
  if (tile == 4) return launch_conv<128, 128, 2, 4, false>(args, nsplit, st, batch, t0, tn);
  if (tile == 1) return launch_conv<128, 128, 2, 2, false>(args, nsplit, st, batch, t0, tn);
  if (tile == 2) return launch_conv<128, 64, 2, 2, false>(args, nsplit, st, batch, t0, tn);
  return launch_conv<64, 64, 2, 2, false>(args, nsplit, st, batch, t0, tn);
}

}  // namespace dim
