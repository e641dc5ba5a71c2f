// Direct convolution, host side: conv2d_fwd_impl, launch plans, split-K, dgrad, deconvolution (source map: conv_impl.h)
#include "conv_impl.h"

namespace dim {

// sum split-K slabs + bias + LeakyReLU.  One float4 per thread.
__global__ void splitk_reduce_kernel(const float* __restrict__ slabs, const float* __restrict__ bias, float* __restrict__ y,
                                     long MC, int Cout, int splits, float slope, int has_bias) {
  long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long i = i4 * 4;
  if (i >= MC) return;
  float4 s = *reinterpret_cast<const float4*>(slabs + i);
  for (int k = 1; k < splits; ++k) {
    float4 p = *reinterpret_cast<const float4*>(slabs + (long)k * MC + i);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  if (has_bias) {
    int c = (int)(i % Cout);
    s.x += bias[c]; s.y += bias[c + 1]; s.z += bias[c + 2]; s.w += bias[c + 3];
  }
  s.x = s.x > 0.f ? s.x : s.x * slope;
  s.y = s.y > 0.f ? s.y : s.y * slope;
  s.z = s.z > 0.f ? s.z : s.z * slope;
  s.w = s.w > 0.f ? s.w : s.w * slope;
  *reinterpret_cast<float4*>(y + i) = s;
}

// the same sum for many slabs of a small array (the first layers' weight gradients: 512 slabs of 26 624 floats, where one thread per
// float4 walking all slabs left 26 workgroups with 512 dependent-latency loads each: 181 us): workgroup = 8 float4 columns x 32 slab
// lanes, lane p sums slabs p, p + 32, ..., then a fixed binary tree over the 32 partial sums (deterministic)
__global__ __launch_bounds__(256) void splitk_reduce_par_kernel(const float* __restrict__ slabs, const float* __restrict__ bias,
                                                                float* __restrict__ y, long MC, int Cout, int splits, float slope,
                                                                int has_bias) {
  __shared__ float4 red[32][8];
  const int qi = threadIdx.x & 7, part = threadIdx.x >> 3;
  const long i = ((long)blockIdx.x * 8 + qi) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < MC)
    for (int k = part; k < splits; k += 32) {
      const float4 p = *reinterpret_cast<const float4*>(slabs + (long)k * MC + i);
      s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
  red[part][qi] = s;
  __syncthreads();
#pragma unroll
  for (int h = 16; h >= 1; h >>= 1) {
    if (part < h) {
      const float4 u = red[part + h][qi];
      float4 t = red[part][qi];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      red[part][qi] = t;
    }
    __syncthreads();
  }
  if (part == 0 && i < MC) {
    s = red[0][qi];
    if (has_bias) {
      int c = (int)(i % Cout);
      s.x += bias[c]; s.y += bias[c + 1]; s.z += bias[c + 2]; s.w += bias[c + 3];
    }
    s.x = s.x > 0.f ? s.x : s.x * slope;
    s.y = s.y > 0.f ? s.y : s.y * slope;
    s.z = s.z > 0.f ? s.z : s.z * slope;
    s.w = s.w > 0.f ? s.w : s.w * slope;
    *reinterpret_cast<float4*>(y + i) = s;
  }
}

}  // namespace dim

using namespace dim;

extern "C" {

// splits == 0 ("auto", see dim_conv2d_fwd): room for the split tail (fewer than one tile per CU on a 304-CU part at most, <= 8 slabs)
static const long kTailWorkspaceFloats = 8L * 304 * 128 * 128;

long dim_conv2d_workspace_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int splits) {
  int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  if (splits == 0) {
    long full = 8L * N * Ho * Wo * Cout;
    return full < kTailWorkspaceFloats ? full : kTailWorkspaceFloats;
  }
  if (splits <= 1) return 0;
  return (long)splits * N * Ho * Wo * Cout;
}

// Plan of the "auto" mode.  All workgroups of a launch are equal, so the launch takes ceil(tiles / CUs) tile-times on the busiest
// CU while the average CU has tiles / CUs of work: conv3 at batch 16 = 1200 tiles on 256 CUs = 4.69 -> 5, i.e. 6 % of the machine
// idles.  The plan runs k*CUs tiles (k whole tiles per CU) as one launch and the remaining `tail` tiles as a second, split-K
// launch of tail*s workgroups of 1/s the length, s chosen to minimise ceil(tail*s / CUs) / s; the slabs are summed by
// dim_splitk_reduce.  -> first tile of the tail (a multiple of nt, so the tail is a row range) and s (1 = single launch).
static void conv_tail_plan(int M, int Cout, int nchunks, int tile, int* tail_begin, int* tail_splits) {
  const int BM = tile == 3 ? 64 : 128, BN = (tile == 3 || tile == 2) ? 64 : 128;
  const int n_cu = device_cu_count();
  const int mt = ceil_div(M, BM), nt = Cout / BN, tiles = mt * nt;
  *tail_begin = tiles;
  *tail_splits = 1;
  const int k = tiles / n_cu;
  if (k < 1) return;                       // small layers: plain split-K chosen by the caller
  const int full = (k * n_cu) / nt * nt;
  const int tail = tiles - full;
  if (tail == 0) return;
  const double single = (double)ceil_div(tiles, n_cu);
  double best = 1e30;
  int best_s = 1;
  for (int s = 2; s <= 8 && s * 4 <= nchunks; ++s) {
    if ((long)s * (M - full / nt * BM) * Cout > kTailWorkspaceFloats) break;
    double t = (double)ceil_div((long)tail * s, n_cu) / s + 0.02 * s;  // 2 % of a tile-time per slab: extra prologues, slab traffic, reduce
    if (t < best) { best = t; best_s = s; }
  }
  if (k + best < single * 0.98) {
    *tail_begin = full;
    *tail_splits = best_s;
  }
}

// ONE copy of the default launch plans of the f32 forward path: the Python executor (FlowNetHip) and the C resident loop
// (dim_refiner_create) both call these, so the two cannot drift apart.
// (tile, splits) of a direct layer (tools/tune_conv.py, batch 16, MI355X): 128 x 128 tiles on 8 waves (tile 4) wherever Cout allows,
// 64 x 64 (tile 3) for Cout = 64 and the 8-channel first layer; splits 0 = "auto" (whole tiles per CU + split-K tail inside the
// library) when every CU gets at least one tile, otherwise the split-K count that minimises the busiest CU's share: all workgroups
// of a launch are equal, the busiest CU gets ceil(tiles s / CUs) of them, each 1 / s of a tile-time long, + 2 % of a tile-time per
// slab for the extra prologues, slab traffic and the reduce.
int dim_conv_auto_plan(long M, int Cout, int nchunks, int cin, int* tile, int* splits) {
  DIM_REQUIRE(tile && splits && M > 0 && Cout > 0 && nchunks > 0, "bad arguments");
  const int n_cu = 256;
  auto best_split = [&](long tiles, int smax) {
    double best = 1e30;
    int bs = 1;
    for (int s = 1; s <= smax; ++s) {
      if (!(s * 4 <= nchunks || s == 1)) continue;
      const double t = (double)((tiles * s + n_cu - 1) / n_cu) / s + 0.02 * s;
      if (t < best) { best = t; bs = s; }
    }
    return bs;
  };
  const bool wide = Cout % 128 == 0 && cin != 8;
  const long tiles = wide ? (M + 127) / 128 * (Cout / 128) : (M + 63) / 64 * (Cout / 64);
  *tile = wide ? 4 : 3;
  *splits = tiles >= n_cu ? 0 : best_split(tiles, 8);
  return DIM_OK;
}

// Plane GEMMs with every f32 operand as three bf16 terms and six MFMA products (wino_gemm_split.hip; default on, DIM_WINO_SPLIT=0 or
// dim_set_winograd_split(0) = the f32 matrix pipe).  Read when a layer is planned, i.e. at the next launch / graph capture.
int dim_set_winograd_split(int on) {
  wino_set_split(on ? 1 : 0);
  return DIM_OK;
}
int dim_get_winograd_split(void) { return wino_get_split(); }

// The plane GEMM of the Winograd layers on its own (wino_gemm.hip / wino_gemm_split.hip), as the layers plan and run it: the entry the
// tests use to pin the arithmetic of one K chunk, which no layer-level bar sees (tests/test_gpu_split_gemm.py).
static bool plane_gemm_on_device(const void* p) {
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();   // a plain host pointer is reported as an error by some runtimes: not a sticky one
  return e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
}
long dim_winograd_plane_gemm_weight_floats(int K, int Cout, int P) {
  if (K <= 0 || Cout <= 0 || P <= 0) return 0;
  return wino_packed_with_split((long)P * K * Cout);
}
int dim_winograd_plane_gemm_split_weights(float* U_packed, int K, int Cout, int P, void* stream) {
  DIM_REQUIRE(K > 0 && K % 32 == 0 && Cout > 0 && Cout % 64 == 0 && P > 0, "winograd plane gemm: K %% 32 == 0 and Cout %% 64 == 0 required");
  DIM_REQUIRE(U_packed, "null pointer");
  DIM_REQUIRE(plane_gemm_on_device(U_packed), "winograd plane gemm: U_packed is not a device pointer");
  return wino_split_weights(U_packed, (long)P * (K / 32), Cout, as_stream(stream));
}
int dim_winograd_plane_gemm(const float* V, const float* U_packed, float* M, int T, int K, int Cout, int P, int tile, int* used_split,
                            void* stream) {
  DIM_REQUIRE(T > 0 && K > 0 && K % 32 == 0 && Cout > 0 && Cout % 64 == 0 && P > 0,
              "winograd plane gemm: T, P > 0, K %% 32 == 0 and Cout %% 64 == 0 required");
  DIM_REQUIRE(V && U_packed && M && used_split, "null pointer");
  DIM_REQUIRE(plane_gemm_on_device(V) && plane_gemm_on_device(U_packed) && plane_gemm_on_device(M),
              "winograd plane gemm: V, U_packed and M must be device pointers");
  WGemmArgs plan;
  const int rc = wino_gemm_plan(&plan, V, U_packed, M, T, K, Cout, P, tile);
  if (rc != DIM_OK) return rc;
  *used_split = plan.split;
  return wino_gemm_run(plan, /*zeroed=*/false, as_stream(stream));
}

// workgroup tile of a Winograd layer's plane GEMMs (wino_gemm.hip): 5 = 128 rows x 256 output channels (V is streamed once per 256
// channels: conv3, conv3_1, conv4_1), 4 = 128 x 128 (conv2: Cout = 128); for the few-row layers (under 1024 tile rows: conv5 .. conv6_1)
// the tile that wastes the fewest MFMA cycles on padded rows -- 6 = 160 x 128 (conv5, conv5_1: 320 rows at 16 pairs), 7 = 96 x 128
// (conv6_1: 96 rows), 3 = 64 x 64 -- weighted by what each reaches of the matrix peak (measured: 0.54 / 0.70 / 0.74).
// DIM_WINO_BN256=0 keeps the 128 x 128 tile everywhere, DIM_WINO_FEWROW=0 the 64 x 64 tile on the few-row layers (A/B timing).
int dim_winograd_gemm_tile_planes(int Cout, long tiles, int planes) {
  static const int bn256 = [] { const char* e = getenv("DIM_WINO_BN256"); return e ? atoi(e) : 1; }();
  static const int fewrow = [] { const char* e = getenv("DIM_WINO_FEWROW"); return e ? atoi(e) : 1; }();
  if (Cout % 128) return 3;
  if (tiles < 1024) {
    if (!fewrow) return 3;
    if (wino_get_split()) {
      // three-term kernels (wino_gemm_split.hip): 128 x 128 (tile 4) or 96 x 128 (tile 7), two 4-wave workgroups per CU.  Cost = rows a
      // workgroup multiplies: items per workgroup (whole workgroups per CU when there are fewer items than slots, as wino_gemm_plan
      // deals them) x tile rows / what the tile reaches (measured at 16 pairs: conv5_1 51.8 us on 7 against 57.2 on 4 and 73.7 on the
      // f32 pipe; conv5, 81 planes, 93.6 on 4 against 110.0 on 7 and 140.8 on the f32 pipe)
      const struct { int tile, bm; double eff; } cand[2] = {{4, 128, 1.0}, {7, 96, planes > 36 ? 0.75 : 0.85}};   // (conv6, 81 planes x 96 rows: 102 us on 4, 116 on 7)
      const int cus = 256, slots = 512;
      int best = 7;
      double best_cost = 1e30;
      for (const auto& c : cand) {
        const long items = (tiles + c.bm - 1) / c.bm * (Cout / 128) * planes;
        long G = items < slots ? items : slots;
        if (G > cus && G < slots) G = G / cus * cus;
        const double cost = (double)items / (double)G * c.bm / c.eff;
        if (cost < best_cost) { best_cost = cost; best = c.tile; }
      }
      return best;
    }
    const struct { int tile, bm; double eff; } cand[3] = {{3, 64, 0.54}, {7, 96, 0.70}, {6, 160, 0.74}};
    int best = 3;
    double best_cost = 1e30;
    for (const auto& c : cand) {
      const double cost = (double)((tiles + c.bm - 1) / c.bm * c.bm) / c.eff;
      if (cost < best_cost) { best_cost = cost; best = c.tile; }
    }
    return best;
  }
  static const int big = [] { const char* e = getenv("DIM_WINO_BIG_TILE"); return e ? atoi(e) : 0; }();   // A/B timing: 6 or 7 on the big layers
  if (big == 6 || big == 7) return big;
  return (Cout % 256 == 0 && bn256) ? 5 : 4;
}
int dim_winograd_gemm_tile(int Cout, long tiles) { return dim_winograd_gemm_tile_planes(Cout, tiles, 36); }

int dim_conv2d_tail_plan(int M, int Cout, int Cin, int KH, int KW, int tile, int* tail_begin_tile, int* tail_splits) {
  DIM_REQUIRE(tail_begin_tile && tail_splits, "null pointer");
  if (tile == 0) tile = (Cout % 128 == 0 && Cin != 8 && M >= 128) ? 4 : 3;
  conv_tail_plan(M, Cout, (Cin == 8) ? (KH * KW + 3) / 4 : KH * KW * (Cin / 32), tile, tail_begin_tile, tail_splits);
  return DIM_OK;
}

int dim_splitk_reduce(const float* slabs, const float* bias, float* y, long M, int Cout, int splits, float slope, void* stream) {
  if (M == 0) return DIM_OK;
  DIM_REQUIRE(slabs && y, "null pointer");
  DIM_REQUIRE(Cout % 4 == 0 && splits >= 1, "bad geometry");
  long MC = M * Cout;
  if (MC / 4 < 65536 && splits >= 64)  // fewer than 256 workgroups of serial sums: spread the slabs over lanes instead
    hipLaunchKernelGGL(splitk_reduce_par_kernel, dim3(ceil_div(MC / 4, 8)), dim3(256), 0, as_stream(stream), slabs, bias, y, MC, Cout,
                       splits, slope, bias != nullptr);
  else
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(ceil_div(MC / 4, 256)), dim3(256), 0, as_stream(stream), slabs, bias, y, MC, Cout,
                       splits, slope, bias != nullptr);
  return check_launch("splitk_reduce");
}

// tile: 0 = auto, 1 = 128x128 (4 waves), 2 = 128x64, 3 = 64x64, 4 = 128x128 with 8 waves (64x32 per wave), 8 = bf16 128x256 (8 waves);
// 6 = first layer (conv_first.hip), 7 / 9 = bf16 LDS-halo / patch kernels (conv_bf16_tiles.hip)
struct ConvEx {
  int in_cstride, out_cstride, out_coff, OH, OW, osy, osx, ooy, oox;  // 0 / 0 / 0 / 0.. = dense defaults
  int accumulate = 0;    // out += result (skip-connection gradients)
  int pad_w = -1;        // >= 0: horizontal padding differs from `pad` (sub-pixel phases of a strided dgrad)
  int Ho = 0, Wo = 0;    // > 0: explicit output grid instead of floor((H+2p-k)/s)+1 (asymmetric padding)
  int batch = 1;         // > 1: `batch` independent problems, strides below (elements)
  long bx = 0, bw = 0, by = 0;
  int boy = 0, box = 0;  // scattered output: per-problem offset increments (see ConvArgs)
  int bf16 = 0;          // w_packed holds bf16 (dim_f32_to_bf16 of the f32 packed array): run on the bf16 matrix pipe
  int slab_full = 0;     // split-K into output-shaped slabs (ConvArgs.slab_full): the caller sums them (slab_sum_rows)
  const float* mask = nullptr;   // tile 9 only: LeakyReLU' of the layer below + its bias-gradient partial sums (ConvArgs.mask)
  float mask_slope = 1.f;
  float* colsum = nullptr;
  int colsum_row0 = 0;
};

static int conv2d_fwd_impl(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                           int Cin, int Cout, int KH, int KW, int stride, int pad, float slope, int splits, int tile,
                           int partial_only, void* stream, const ConvEx* ex = nullptr) {
  if (N == 0) return DIM_OK;  // empty batch
  DIM_REQUIRE(x && w_packed && y, "null pointer");
  DIM_REQUIRE(Cin == 8 || Cin % 32 == 0, "Cin must be 8 or a multiple of 32 (got %d)", Cin);
  DIM_REQUIRE(Cout % 64 == 0, "Cout must be a multiple of 64 (got %d)", Cout);
  DIM_REQUIRE(stride >= 1 && pad >= 0 && KH >= 1 && KW >= 1, "bad geometry");
  DIM_REQUIRE(Cin != 8 || KW <= 8, "Cin==8 path needs KW<=8");
  ConvArgs a;
  a.y_bytes = 0;
  a.x = x; a.w = w_packed; a.bias = bias;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride;
  a.pad_h = pad;
  a.pad_w = (ex && ex->pad_w >= 0) ? ex->pad_w : pad;
  // a map smaller than the kernel has no output: C division rounds (H + 2 pad - KH) / stride towards zero, which would turn -1 / 2 into
  // one output row that lies outside the caller's (empty) buffer
  DIM_REQUIRE((ex && ex->Ho > 0) || H + 2 * pad >= KH, "empty output");
  DIM_REQUIRE((ex && ex->Wo > 0) || W + 2 * a.pad_w >= KW, "empty output");
  a.Ho = (ex && ex->Ho > 0) ? ex->Ho : (H + 2 * pad - KH) / stride + 1;
  a.Wo = (ex && ex->Wo > 0) ? ex->Wo : (W + 2 * a.pad_w - KW) / stride + 1;
  DIM_REQUIRE(a.Ho > 0 && a.Wo > 0, "empty output");
  a.accumulate = ex ? ex->accumulate : 0;
  a.in_cstride = (ex && ex->in_cstride) ? ex->in_cstride : Cin;
  a.out_cstride = (ex && ex->out_cstride) ? ex->out_cstride : Cout;
  a.out_coff = ex ? ex->out_coff : 0;
  a.dense_out = !(ex && ex->osy);
  a.OH = a.dense_out ? a.Ho : ex->OH; a.OW = a.dense_out ? a.Wo : ex->OW;
  a.osy = a.dense_out ? 1 : ex->osy; a.osx = a.dense_out ? 1 : ex->osx;
  a.ooy = a.dense_out ? 0 : ex->ooy; a.oox = a.dense_out ? 0 : ex->oox;
  DIM_REQUIRE(a.in_cstride >= Cin && a.in_cstride % 4 == 0, "in_cstride must be >= Cin and a multiple of 4");
  DIM_REQUIRE(a.out_cstride >= a.out_coff + Cout, "out_cstride < out_coff + Cout");
  DIM_REQUIRE((long)N * H * W * a.in_cstride < (1L << 29), "input too large for 32-bit byte offsets (%ld elements)",
              (long)N * H * W * a.in_cstride);
  a.x_bytes = (unsigned)((long)N * H * W * a.in_cstride * 4);
  a.M = N * a.Ho * a.Wo;
  a.nchunks = (Cin == 8) ? (KH * KW + 3) / 4 : KH * KW * (Cin / 32);
  a.div_kw = make_fastdiv((unsigned)KW);
  DIM_REQUIRE((long)a.nchunks * Cout * 32 * 4 < (1L << 31), "packed weights too large for 32-bit byte offsets");
  a.bf16 = ex ? ex->bf16 : 0;
  a.w_bytes = (unsigned)((long)a.nchunks * Cout * 32 * (a.bf16 ? 2 : 4));
  const bool auto_split = splits == 0;
  if (splits < 1) splits = 1;
  if (splits > a.nchunks) splits = a.nchunks;
  a.chunks_per_split = (a.nchunks + splits - 1) / splits;
  splits = (a.nchunks + a.chunks_per_split - 1) / a.chunks_per_split;
  DIM_REQUIRE(splits == 1 || workspace, "split-K needs a workspace (dim_conv2d_workspace_floats)");
  a.slab_full = (ex && ex->slab_full && splits > 1) ? 1 : 0;
  a.mask = ex ? ex->mask : nullptr;
  a.mask_slope = ex ? ex->mask_slope : 1.f;
  a.colsum = ex ? ex->colsum : nullptr;
  a.colsum_row0 = ex ? ex->colsum_row0 : 0;
  DIM_REQUIRE(!a.mask || (tile == 9 && a.colsum && !a.accumulate && splits == 1), "the LeakyReLU' / bias-gradient fold exists in tile 9 only");
  DIM_REQUIRE(splits == 1 || !ex || a.slab_full || (a.dense_out && a.out_cstride == Cout && a.out_coff == 0),
              "split-K writes a dense [M][Cout] result: not available with a strided / scattered output");
  DIM_REQUIRE(!a.slab_full || (a.bf16 && (tile == 3 || tile == 4) && (!ex || ex->batch == 1)),
              "output-shaped split-K slabs: bf16 gathered-tap kernel (tile 3 / 4), single problem");
  a.y = splits > 1 ? workspace : y;
  // every kernel stores through a buffer descriptor with 32-bit byte offsets (branch-free epilogues)
  DIM_REQUIRE((long)N * a.OH * a.OW * a.out_cstride * 4 < (1L << 31), "output too large for 32-bit byte offsets (%ld bytes)",
              (long)N * a.OH * a.OW * a.out_cstride * 4);
  a.y_bytes = (unsigned)((long)N * a.OH * a.OW * a.out_cstride * 4);
  DIM_REQUIRE(splits == 1 || (long)a.M * Cout * 4 < (1L << 31), "split-K slab too large for 32-bit byte offsets (%ld bytes)", (long)a.M * Cout * 4);
  a.tile_off = 0;
  a.slab_row0 = 0;
  a.slab_stride = a.slab_full ? (long)N * a.OH * a.OW * a.out_cstride : (long)N * a.Ho * a.Wo * Cout;
  const int batch = ex ? ex->batch : 1;
  a.bx = ex ? ex->bx : 0; a.bw = ex ? ex->bw : 0; a.by = ex ? ex->by : 0;
  a.boy = ex ? ex->boy : 0; a.box = ex ? ex->box : 0;
  DIM_REQUIRE(batch == 1 || splits == 1, "batched launch does not combine with split-K");
  a.slope = slope;
  a.has_bias = bias != nullptr;
  hipStream_t st = as_stream(stream);
  if (tile == 0) {
    tile = (Cout % 128 == 0 && Cin != 8 && a.M >= 128) ? 4 : 3;  // same rule as lib/hip/ops.py conv_auto_plan
  }
  if (tile == 7) return launch_conv_bf16_halo(a, splits, batch, partial_only, st);
  if (tile == 9) return launch_conv_bf16_patch(a, splits, batch, partial_only, st);
  if (tile == 6) return launch_conv_first(a, splits, batch, partial_only, st);
  DIM_REQUIRE((tile != 1 && tile != 4) || Cout % 128 == 0, "tile 128x128 needs Cout %% 128 == 0");
  DIM_REQUIRE(tile != 8 || (a.bf16 && Cout % 256 == 0 && Cin != 8 && !auto_split), "tile 8 (128x256): bf16, Cout %% 256 == 0, explicit splits");
  DIM_REQUIRE(Cin != 8 || tile != 4, "tile 4 (128x128, 8 waves) is not built for the 8-channel layer");
  DIM_REQUIRE(Cin != 8 || batch == 1, "batched launch is not built for the 8-channel layer");
  // "auto" (splits == 0): whole tiles per CU in one launch, the remainder as a split-K launch + reduce (conv_tail_plan)
  if (auto_split && batch == 1 && workspace && a.dense_out && a.out_cstride == Cout && a.out_coff == 0 && !a.accumulate && !partial_only) {
    int tail_begin = 0, ts = 1;
    conv_tail_plan(a.M, Cout, a.nchunks, tile, &tail_begin, &ts);
    if (ts >= 2) {
      const int BMt = tile == 3 ? 64 : 128, BNt = (tile == 3 || tile == 2) ? 64 : 128;
      const int nt = Cout / BNt, tiles = ceil_div(a.M, BMt) * nt;
      const int row0 = tail_begin / nt * BMt;
      int rc = launch_conv_gather(a, tile, 1, st, batch, 0, tail_begin);
      if (rc != DIM_OK) return rc;
      ConvArgs t = a;
      t.y = workspace;
      t.slab_row0 = row0;
      t.slab_stride = (long)(a.M - row0) * Cout;
      t.chunks_per_split = (a.nchunks + ts - 1) / ts;
      const int nsplit = (a.nchunks + t.chunks_per_split - 1) / t.chunks_per_split;
      DIM_REQUIRE(nsplit * t.slab_stride <= kTailWorkspaceFloats, "tail workspace bound exceeded");
      rc = launch_conv_gather(t, tile, nsplit, st, batch, tail_begin, tiles - tail_begin);
      if (rc != DIM_OK) return rc;
      return dim_splitk_reduce(workspace, bias, y + (long)row0 * Cout, (long)(a.M - row0), Cout, nsplit, slope, stream);
    }
  }
  int rc = launch_conv_gather(a, tile, splits, st, batch, 0, -1);
  if (rc != DIM_OK) return rc;
  if (a.slab_full) return DIM_OK;   // the caller sums the output-shaped slabs once all its launches are in
  if (splits > 1 && !partial_only) return dim_splitk_reduce(workspace, bias, y, (long)a.M, Cout, splits, slope, stream);
  return DIM_OK;
}

int dim_conv2d_fwd(const float* x, const float* w_packed, const float* bias, float* y, float* workspace, int N, int H, int W,
                   int Cin, int Cout, int KH, int KW, int stride, int pad, float slope, int splits, int tile, void* stream) {
  return conv2d_fwd_impl(x, w_packed, bias, y, workspace, N, H, W, Cin, Cout, KH, KW, stride, pad, slope, splits, tile, 0, stream);
}

// ---- bf16 twins: identical arguments, `w_packed` is the bf16 image (dim_f32_to_bf16) of the f32 packed array
int dim_conv2d_fwd_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, float* workspace, int N, int H, int W,
                        int Cin, int Cout, int KH, int KW, int stride, int pad, float slope, int splits, int tile, void* stream) {
  ConvEx ex = {};
  ex.bf16 = 1;
  DIM_REQUIRE(splits >= 1, "the bf16 path takes an explicit split-K count (>= 1)");
  return conv2d_fwd_impl(x, reinterpret_cast<const float*>(w_packed_bf16), bias, y, workspace, N, H, W, Cin, Cout, KH, KW, stride, pad,
                         slope, splits, tile, 0, stream, &ex);
}

int dim_conv2d_fwd_ex_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, int N, int H, int W, int Cin,
                           int in_cstride, int Cout, int KH, int KW, int stride, int pad, float slope, int tile, int out_cstride,
                           int out_coff, int OH, int OW, int osy, int osx, int ooy, int oox, int Ho, int Wo, int pad_w, int accumulate,
                           void* stream) {
  ConvEx ex = {in_cstride, out_cstride, out_coff, OH, OW, osy, osx, ooy, oox};
  ex.Ho = Ho;
  ex.Wo = Wo;
  ex.pad_w = pad_w;
  ex.accumulate = accumulate;
  ex.bf16 = 1;
  return conv2d_fwd_impl(x, reinterpret_cast<const float*>(w_packed_bf16), bias, y, nullptr, N, H, W, Cin, Cout, KH, KW, stride, pad, slope,
                         1, tile, 0, stream, &ex);
}

int dim_conv2d_fwd_ex(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int in_cstride,
                      int Cout, int KH, int KW, int stride, int pad, float slope, int tile, int out_cstride, int out_coff, int OH,
                      int OW, int osy, int osx, int ooy, int oox, int Ho, int Wo, int pad_w, int accumulate, void* stream) {
  ConvEx ex = {in_cstride, out_cstride, out_coff, OH, OW, osy, osx, ooy, oox};
  ex.Ho = Ho;
  ex.Wo = Wo;
  ex.pad_w = pad_w;
  ex.accumulate = accumulate;
  return conv2d_fwd_impl(x, w_packed, bias, y, nullptr, N, H, W, Cin, Cout, KH, KW, stride, pad, slope, 1, tile, 0, stream, &ex);
}

// ---------------------------------------------------------------------------------------------------------------- dgrad
// Gradient w.r.t. the input of y = conv(x, W (Cout,Cin,KH,KW), stride s in {1,2}, pad p) on the SAME MFMA kernel with re-packed
// weights (channel roles swapped).
//   s = 1:  dX[i] = sum_j dY[i - (K-1-p) + j] * W[K-1-j]                      one stride-1 convolution over dY
//   s = 2:  input rows iy = 2t + ph (phase ph):  dX[2t+ph] = sum_e dY[t + e] * W[ph + p - 2e],  e in [emin, emax]
//           = stride-1 convolution over dY with KH' = emax-emin+1 taps and pad' = -emin, scattered to rows 2t+ph.
// Packed layout: phases (py,px) one after the other, each [chunk][CinPad][32] with chunk = (32-slice of Cout, jy, jx) and
// CinPad = Cin rounded up to 64 (the kernel's channel tile; padded outputs are zero).
// (DgAxis / dg_axis: conv_impl.h; the packers of this layout: conv_pack.hip)

// dx (N,H,W,dx_cstride)[..., :Cin] (+)= dgrad(dy (N,Ho,Wo,dy_cstride)[..., :Cout]).  accumulate != 0 adds to dx (skip connections).
// dst[row][0:width] (+)= sum over the slabs of slab[row][0:width]; rows are `pitch` floats apart in dst and in every slab
__global__ __launch_bounds__(256) void slab_sum_rows_kernel(const float* __restrict__ slabs, long slab_stride, int nslabs,
                                                            float* __restrict__ dst, long rows, int width4, int pitch, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * width4) return;
  const long row = i / width4;
  const int c = (int)(i - row * width4) * 4;
  const long o = row * pitch + c;
  float4 s = accumulate ? *reinterpret_cast<const float4*>(dst + o) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < nslabs; ++k) {   // fixed order: deterministic
    const float4 v = *reinterpret_cast<const float4*>(slabs + (long)k * slab_stride + o);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  *reinterpret_cast<float4*>(dst + o) = s;
}

// rows of the bias-gradient partial sums one folded input gradient writes: 2 per 16 x 16 block of every phase image
static long dgrad_fold_rows(int N, int H, int W, int stride) {
  long rows = 0;
  const int nph = stride == 1 ? 1 : 2;
  for (int py = 0; py < nph; ++py)
    for (int px = 0; px < nph; ++px) {
      const int Th = stride == 1 ? H : (H - py + 1) / 2, Tw = stride == 1 ? W : (W - px + 1) / 2;
      if (Th > 0 && Tw > 0) rows += 2L * N * ((Th + 15) / 16) * ((Tw + 15) / 16);
    }
  return rows;
}

static int conv2d_dgrad_impl(const float* dy, const float* w_dgrad_packed, float* dx, int N, int H, int W, int Cin, int dx_cstride, int Ho,
                             int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad, int accumulate, int tile, int bf16,
                             void* stream, float* workspace = nullptr, int splits = 1, const float* mask = nullptr, float mask_slope = 1.f,
                             float* colsum = nullptr) {
  if (N == 0) return DIM_OK;
  long fold_row = 0;
  // split-K (bf16, gathered-tap tiles): the small maps give 80-600 workgroups to 1280 resident slots and every workgroup walks
  // K = 4608 .. 9216 alone on its CU; `splits` K ranges write output-shaped slabs (every phase of a strided gradient into the same
  // slabs, each to its own pixels) and ONE pass sums them into dx
  const bool split = splits > 1;
  DIM_REQUIRE(!split || (bf16 && workspace && (tile == 3 || tile == 4)), "split-K input gradient: bf16, tile 3 or 4, workspace required");
  DIM_REQUIRE(stride == 1 || stride == 2, "dgrad supports stride 1 or 2");
  int CinPad = (Cin + 63) / 64 * 64;
  DIM_REQUIRE(dx_cstride >= CinPad, "dx channel stride (%d) must be >= Cin rounded up to 64 (%d)", dx_cstride, CinPad);
  int nph = stride == 1 ? 1 : 2;
  long off = 0;
  for (int py = 0; py < nph; ++py)
    for (int px = 0; px < nph; ++px) {
      DgAxis ah = dg_axis(KH, stride, pad, py), aw = dg_axis(KW, stride, pad, px);
      long total = (long)(Cout / 32) * ah.ntaps * aw.ntaps * CinPad * 32;
      int Th = stride == 1 ? H : (H - py + 1) / 2, Tw = stride == 1 ? W : (W - px + 1) / 2;
      if (Th > 0 && Tw > 0) {
        ConvEx ex = {dy_cstride, dx_cstride, 0, H, W, stride == 1 ? 0 : 2, stride == 1 ? 0 : 2, py, px};
        ex.pad_w = -aw.emin;
        ex.Ho = Th;
        ex.Wo = Tw;
        ex.accumulate = split ? 0 : accumulate;
        ex.bf16 = bf16;
        ex.slab_full = split ? 1 : 0;
        ex.mask = mask;
        ex.mask_slope = mask_slope;
        ex.colsum = colsum;
        ex.colsum_row0 = (int)fold_row;
        fold_row += 2L * N * ((Th + 15) / 16) * ((Tw + 15) / 16);
        if (total > 0) {
          // tile 9 (bf16 patch kernel) takes the phases with 2 .. 9 taps; a single-tap phase is a 1x1 convolution: gathered-tap kernel
          int ptile = tile;
          if (tile == 9 && !(bf16 && ah.ntaps <= 3 && aw.ntaps <= 3 && ah.ntaps * aw.ntaps >= 2))
            ptile = CinPad % 128 == 0 ? 4 : 3;
          DIM_REQUIRE(!mask || ptile == 9, "folded input gradient: phase (%d,%d) has %d x %d taps, which the patch kernel does not take", py, px,
                      ah.ntaps, aw.ntaps);
          // every slab of every phase must be written: the phase's K chunks have to make exactly `splits` non-empty ranges
          const int nch = ah.ntaps * aw.ntaps * (Cout / 32);
          const int psplits = split ? splits : 1;
          DIM_REQUIRE(!split || (nch >= splits && (nch + (nch + splits - 1) / splits - 1) / ((nch + splits - 1) / splits) == splits),
                      "split-K input gradient: a phase has %d K chunks, which do not make %d non-empty splits", nch, splits);
          int rc = conv2d_fwd_impl(dy, bf16 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(w_dgrad_packed) + 2 * off)
                                            : w_dgrad_packed + off, nullptr, dx, split ? workspace : nullptr, N, Ho, Wo, Cout, CinPad,
                                   ah.ntaps, aw.ntaps, 1, -ah.emin, 1.0f, psplits, ptile, 0, stream, &ex);
          if (rc != DIM_OK) return rc;
        } else if (!accumulate || mask || split) {
          // (split: the slab rows of a tap-less phase would never be written, and slab_sum_rows_kernel adds every row of every slab)
          return set_err(DIM_ERR_ARG, "phase (%d,%d) has no taps: dX rows of that phase would stay unwritten", py, px);
        }
      }
      off += total;
    }
  if (split) {
    const long rows = (long)N * H * W;
    hipLaunchKernelGGL(slab_sum_rows_kernel, dim3(ceil_div(rows * (CinPad / 4), 256)), dim3(256), 0, as_stream(stream), workspace,
                       rows * dx_cstride, splits, dx, rows, CinPad / 4, dx_cstride, accumulate);
    return check_launch("slab_sum_rows");
  }
  return DIM_OK;
}

int dim_conv2d_dgrad(const float* dy, const float* w_dgrad_packed, float* dx, int N, int H, int W, int Cin, int dx_cstride, int Ho,
                     int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad, int accumulate, int tile, void* stream) {
  return conv2d_dgrad_impl(dy, w_dgrad_packed, dx, N, H, W, Cin, dx_cstride, Ho, Wo, Cout, dy_cstride, KH, KW, stride, pad, accumulate, tile,
                           0, stream);
}

int dim_conv2d_dgrad_bf16(const float* dy, const void* w_dgrad_packed_bf16, float* dx, int N, int H, int W, int Cin, int dx_cstride,
                          int Ho, int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad, int accumulate, int tile,
                          void* stream) {
  return conv2d_dgrad_impl(dy, reinterpret_cast<const float*>(w_dgrad_packed_bf16), dx, N, H, W, Cin, dx_cstride, Ho, Wo, Cout, dy_cstride,
                           KH, KW, stride, pad, accumulate, tile, 1, stream);
}

long dim_conv2d_dgrad_splitk_workspace_floats(int N, int H, int W, int dx_cstride, int splits) {
  return splits > 1 ? (long)splits * N * H * W * dx_cstride : 0;
}

int dim_conv2d_dgrad_bf16_splitk(const float* dy, const void* w_dgrad_packed_bf16, float* dx, float* workspace, int N, int H, int W, int Cin,
                                 int dx_cstride, int Ho, int Wo, int Cout, int dy_cstride, int KH, int KW, int stride, int pad,
                                 int accumulate, int tile, int splits, void* stream) {
  DIM_REQUIRE(splits >= 1, "splits >= 1");
  DIM_REQUIRE(dx_cstride % 4 == 0 && (reinterpret_cast<uintptr_t>(dx) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "split-K input gradient: dx / workspace 16-byte aligned, channel stride a multiple of 4");
  return conv2d_dgrad_impl(dy, reinterpret_cast<const float*>(w_dgrad_packed_bf16), dx, N, H, W, Cin, dx_cstride, Ho, Wo, Cout, dy_cstride,
                           KH, KW, stride, pad, accumulate, tile, 1, stream, workspace, splits);
}

long dim_conv2d_dgrad_lrelu_workspace_floats(int N, int H, int W, int Cin, int stride) {
  const long rows = dgrad_fold_rows(N, H, W, stride);
  const int CinPad = (Cin + 63) / 64 * 64;
  return rows * CinPad + dim_bias_grad_workspace_floats(rows, CinPad);
}

// dz = dX * LeakyReLU'(y_act) and db = column sums of dz, both inside the input gradient's epilogue (tile 9) + one small reduce
int dim_conv2d_dgrad_bf16_lrelu(const float* dy, const void* w_dgrad_packed_bf16, float* dz, const float* y_act, float slope, float* db,
                                float* workspace, int N, int H, int W, int Cin, int dx_cstride, int Ho, int Wo, int Cout, int dy_cstride,
                                int KH, int KW, int stride, int pad, int accumulate_db, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(y_act && db && workspace, "null pointer");
  const int CinPad = (Cin + 63) / 64 * 64;
  DIM_REQUIRE(Cin == CinPad && dx_cstride == Cin, "folded input gradient: dz and the stored activation must both be dense (N, H, W, Cin %% 64 == 0)");
  const long rows = dgrad_fold_rows(N, H, W, stride);
  int rc = conv2d_dgrad_impl(dy, reinterpret_cast<const float*>(w_dgrad_packed_bf16), dz, N, H, W, Cin, dx_cstride, Ho, Wo, Cout, dy_cstride, KH,
                             KW, stride, pad, 0, 9, 1, stream, nullptr, 1, y_act, slope, workspace);
  if (rc != DIM_OK) return rc;
  return dim_bias_grad(workspace, db, workspace + rows * CinPad, rows, CinPad, CinPad, 0, accumulate_db, stream);
}

int dim_conv2d_fwd_partial(const float* x, const float* w_packed, float* workspace, int N, int H, int W, int Cin, int Cout, int KH,
                           int KW, int stride, int pad, int splits, int tile, void* stream) {
  DIM_REQUIRE(splits > 1, "dim_conv2d_fwd_partial is the split-K first phase: splits must be > 1");
  return conv2d_fwd_impl(x, w_packed, nullptr, workspace, workspace, N, H, W, Cin, Cout, KH, KW, stride, pad, 1.0f, splits, tile, 1,
                         stream);
}

// y[:, oy, ox, out_coff : out_coff+Cout] = LeakyReLU(Crop(Deconvolution(x, k=4, s=2, p=0) + bias, offset=(crop,crop)))   (NHWC)
// x (N,H,W,in_cstride) with Cin valid channels, zero weights for the padding up to a multiple of 32.
static int deconv4x4s2_fwd_impl(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin,
                                int in_cstride, int Cout, int OH, int OW, int crop, float slope, int out_cstride, int out_coff, int tile,
                                int bf16, void* stream) {
  if (N == 0) return DIM_OK;
  int CinPad = (Cin + 31) / 32 * 32;
  DIM_REQUIRE(in_cstride >= CinPad, "in_cstride (%d) must cover the padded channel count %d (pad channels must hold zeros)", in_cstride,
              CinPad);
  DIM_REQUIRE(OH + crop <= 2 * H + 2 && OW + crop <= 2 * W + 2, "crop window outside the deconvolution output");
  // the four output phases read the same input windows and differ in weights and in where they land: ONE batched launch
  // (blockIdx.y = phase), 4x the workgroups of a per-phase launch on maps as small as 15x20
  const long per_phase = (long)CinPad * 4 * Cout;
  ConvEx ex = {in_cstride, out_cstride, out_coff, OH, OW, 2, 2, -crop, -crop};
  ex.batch = 4;
  ex.bw = per_phase;
  ex.boy = 1;
  ex.box = 1;
  ex.bf16 = bf16;
  return conv2d_fwd_impl(x, w_packed, bias, y, nullptr, N, H, W, CinPad, Cout, 2, 2, 1, 1, slope, 1, tile, 0, stream, &ex);
}

int dim_deconv4x4s2_fwd(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin,
                        int in_cstride, int Cout, int OH, int OW, int crop, float slope, int out_cstride, int out_coff, int tile,
                        void* stream) {
  return deconv4x4s2_fwd_impl(x, w_packed, bias, y, N, H, W, Cin, in_cstride, Cout, OH, OW, crop, slope, out_cstride, out_coff, tile, 0,
                              stream);
}

int dim_deconv4x4s2_fwd_bf16(const float* x, const void* w_packed_bf16, const float* bias, float* y, int N, int H, int W, int Cin,
                             int in_cstride, int Cout, int OH, int OW, int crop, float slope, int out_cstride, int out_coff, int tile,
                             void* stream) {
  return deconv4x4s2_fwd_impl(x, reinterpret_cast<const float*>(w_packed_bf16), bias, y, N, H, W, Cin, in_cstride, Cout, OH, OW, crop,
                              slope, out_cstride, out_coff, tile, 1, stream);
}

}  // extern "C"
