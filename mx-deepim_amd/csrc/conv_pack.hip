// Weight packers and f32 <-> bf16 converters (source map: conv_impl.h)
#include "conv_impl.h"

namespace dim {

// element-wise f32 -> bf16 (round to nearest even): the packed weight arrays of the bf16 kernels, the flat gradient bucket
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    *reinterpret_cast<bf16x4*>(dst + i) = to_bf16x4(*reinterpret_cast<const float4*>(src + i));
  } else {
    for (long k = i; k < n; ++k) dst[k] = (__bf16)src[k];
  }
}
__global__ void bf16_to_f32_kernel(const __bf16* __restrict__ src, float* __restrict__ dst, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(src + i);
    *reinterpret_cast<float4*>(dst + i) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  } else {
    for (long k = i; k < n; ++k) dst[k] = (float)src[k];
  }
}

// OIHW (MXNet / reference layout) -> packed [chunk][Cout][32]  (a workgroup's B chunk is one contiguous block)
template <typename PT>
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, PT* __restrict__ wp, int Cout, int Cin, int KH, int KW,
                                        int nchunks, int cin8, int CoutValid) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)nchunks * 32 * Cout;
  if (idx >= total) return;
  int kin = (int)(idx % 32);
  long t = idx / 32;
  int co = (int)(t % Cout);
  int kc = (int)(t / Cout);
  int kh, kw, c;
  if (cin8) {
    const int t = kc * 4 + (kin >> 3);  // flat tap, row-major over KH x KW (taps past KH*KW: kh >= KH -> zero weight)
    kh = t / KW;
    kw = t - kh * KW;
    c = kin & 7;
  } else {
    int taps = KH * KW;
    int cc = kc / taps;
    int tap = kc - cc * taps;
    c = cc * 32 + kin;
    kh = tap / KW;
    kw = tap - kh * KW;
  }
  float v = 0.f;
  if (kh < KH && kw < KW && c < Cin && co < CoutValid) v = w[(((long)co * Cin + c) * KH + kh) * KW + kw];
  wp[idx] = (PT)v;
}

// FullyConnected weight (out, in) with `in` flattened (c,h,w) [mx Flatten of NCHW] -> packed
// [chunk][out][32] with chunk = (32-channel slice, h, w) so that fc6 runs through conv_fwd_kernel on the NHWC conv6_1 output.
__global__ void pack_fc_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Out, int C, int H, int W) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)Out * C * H * W;
  if (idx >= total) return;
  int kin = (int)(idx % 32);
  long t = idx / 32;
  int o = (int)(t % Out);
  long kc = t / Out;                       // chunk = (channel slice, tap) with the tap (h,w) fastest, as in the conv kernel
  int c = (int)(kc / ((long)H * W)) * 32 + kin;
  long hw = kc % ((long)H * W);
  wp[idx] = w[(long)o * C * H * W + (long)c * H * W + hw];
}

// Deconvolution(k=4, s=2, p=0) weight (Cin, Cout, 4, 4) [MXNet layout] -> four packed 2x2 convolution weights, one per output
// phase (py,px): out[2t+py, 2u+px] = sum_{dy,dx} in[t-1+dy, u-1+dx] * w[ci][co][py+2(1-dy)][px+2(1-dx)]   (pad 1, stride 1).
// Cin is zero-padded to CinPad (multiple of 32).  Layout per phase: [chunk][Cout][32], chunk = (channel slice, dy, dx).
template <typename PT>
__global__ void pack_deconv4x4s2_weight_kernel(const float* __restrict__ w, PT* __restrict__ wp, int Cin, int CinPad, int Cout) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per_phase = (long)CinPad * 4 * Cout;
  if (idx >= 4 * per_phase) return;
  int phase = (int)(idx / per_phase);
  long r = idx % per_phase;
  int kin = (int)(r % 32);
  long t = r / 32;
  int co = (int)(t % Cout);
  int kc = (int)(t / Cout);
  int cc = kc / 4, tap = kc % 4, dy = tap / 2, dx = tap % 2;
  int ci = cc * 32 + kin;
  int py = phase / 2, px = phase % 2;
  float v = 0.f;
  if (ci < Cin) v = w[(((long)ci * Cout + co) * 4 + (py + 2 * (1 - dy))) * 4 + (px + 2 * (1 - dx))];
  wp[idx] = (PT)v;
}

__global__ void pack_small_cout_weight_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int CinPad,
                                              int KH, int KW) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)Cout * KH * KW * CinPad;
  if (idx >= total) return;
  int ci = (int)(idx % CinPad);
  long t = idx / CinPad;
  int kw = (int)(t % KW); t /= KW;
  int kh = (int)(t % KH);
  int co = (int)(t / KH);
  wp[idx] = ci < Cin ? w[(((long)co * Cin + ci) * KH + kh) * KW + kw] : 0.f;
}

}  // namespace dim

using namespace dim;

extern "C" {

long dim_conv2d_packed_weight_floats(int Cout, int Cin, int KH, int KW) {
  if (Cin == 8)  // 4 taps x 8 channels per chunk, taps flat over KH x KW; the first layer's three-term image behind it
    return (long)((KH * KW + 3) / 4) * 32 * Cout + (KH == 7 && KW == 7 && Cout == 64 ? (long)(kC1SplitBytes / 4) : 0);
  return (long)KH * KW * Cin * Cout;
}

// OIHW -> [chunk][CoutPad][32], rows >= Cout zero.  Cin % 32 == 0: tiled (workgroup = (32-channel slice, G output channels):
// rows = w[co][cc * 32 + r][tap], packed run tap at ((cc * T + tap) * CoutPad + co) * 32); the 8-channel first layer: per element
extern "C++" template <typename PT>
int pack_conv_weight_any(const float* w_oihw, PT* w_packed, int Cout, int CoutPad, int Cin, int KH, int KW, void* stream) {
  const int cin8 = Cin == 8, T = KH * KW;
  const int nchunks = cin8 ? (T + 3) / 4 : T * (Cin / 32);
  const int G = cin8 ? 0 : wtile_group(CoutPad, T, Cin / 32);
  if (G) {
    WTileArgs a = {};
    a.src = w_oihw; a.dst = w_packed;
    a.G = G; a.Q = T; a.gmax = Cout; a.rmax = Cin; a.g_fast = 0; a.nj = 0;
    a.sg = (long)Cin * T; a.sr = T; a.rows_x = 32L * T; a.rows_y = (long)G * Cin * T;
    a.dq = (long)CoutPad * 32; a.packed_x = (long)T * CoutPad * 32;
    wtile_launch<true, PT>(a, Cin / 32, CoutPad / G, as_stream(stream));
  } else {
    long total = (long)nchunks * 32 * CoutPad;
    hipLaunchKernelGGL((pack_conv_weight_kernel<PT>), dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed, CoutPad,
                       Cin, KH, KW, nchunks, cin8, Cout);
  }
  return check_launch("pack_conv_weight");
}

int dim_conv2d_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(Cin == 8 || Cin % 32 == 0, "Cin must be 8 or a multiple of 32 (got %d)", Cin);
  DIM_REQUIRE(Cin != 8 || KW <= 8, "Cin==8 path needs KW<=8 (got %d)", KW);
  int rc = pack_conv_weight_any(w_oihw, w_packed, Cout, Cout, Cin, KH, KW, stream);
  if (rc == DIM_OK && Cin == 8 && KH == 7 && KW == 7 && Cout == 64)   // flow_conv1: + the image conv1_halo_split_kernel reads
    rc = launch_conv1_split_weights(w_packed, as_stream(stream));
  return rc;
}

// same, with the output-channel count padded with zero rows up to CoutPad (a multiple of 64): w_oihw has Cout rows
int dim_conv2d_pack_weight_padded(const float* w_oihw, float* w_packed, int Cout, int CoutPad, int Cin, int KH, int KW, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null weight pointer");
  DIM_REQUIRE(Cin % 32 == 0 && CoutPad >= Cout && CoutPad % 64 == 0, "Cin %% 32 == 0 and CoutPad a multiple of 64 >= Cout required");
  return pack_conv_weight_any(w_oihw, w_packed, Cout, CoutPad, Cin, KH, KW, stream);
}

// the bf16 image of the same packed array in one pass (== dim_f32_to_bf16 of dim_conv2d_pack_weight_padded's output); CoutPad == Cout
// for an unpadded layer
int dim_conv2d_pack_weight_bf16(const float* w_oihw, void* w_packed_bf16, int Cout, int CoutPad, int Cin, int KH, int KW, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed_bf16, "null weight pointer");
  DIM_REQUIRE(Cin == 8 || Cin % 32 == 0, "Cin must be 8 or a multiple of 32 (got %d)", Cin);
  DIM_REQUIRE(Cin != 8 || KW <= 8, "Cin==8 path needs KW<=8 (got %d)", KW);
  DIM_REQUIRE(CoutPad >= Cout, "CoutPad < Cout");
  return pack_conv_weight_any(w_oihw, reinterpret_cast<__bf16*>(w_packed_bf16), Cout, CoutPad, Cin, KH, KW, stream);
}

int dim_fc_pack_weight(const float* w_out_in, float* w_packed, int Out, int C, int H, int W, void* stream) {
  DIM_REQUIRE(w_out_in && w_packed, "null weight pointer");
  long total = (long)Out * C * H * W;
  const int HW = H * W, G = C % 32 == 0 ? wtile_group(Out, HW, C / 32) : 0;
  if (G) {  // workgroup (channel slice cb, G outputs): rows = w[o][cb * 32 + r][q], packed run q at ((cb * HW + q) * Out + o) * 32
    WTileArgs a = {};
    a.src = w_out_in; a.dst = w_packed;
    a.G = G; a.Q = HW; a.gmax = Out; a.rmax = C; a.g_fast = 0; a.nj = 0;
    a.sg = (long)C * HW; a.sr = HW; a.rows_x = 32L * HW; a.rows_y = (long)G * C * HW;
    a.dq = (long)Out * 32; a.packed_x = (long)HW * Out * 32;
    wtile_launch<true, float>(a, C / 32, Out / G, as_stream(stream));
  } else {
    hipLaunchKernelGGL(pack_fc_weight_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_out_in, w_packed, Out,
                       C, H, W);
  }
  return check_launch("pack_fc_weight");
}

// element-wise converters: the bf16 kernels take the bf16 image (dim_f32_to_bf16) of an f32 packed array
int dim_f32_to_bf16(const float* src, void* dst_bf16, long n, void* stream) {
  if (n == 0) return DIM_OK;
  DIM_REQUIRE(src && dst_bf16 && n > 0, "null pointer");
  DIM_REQUIRE(reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_bf16) % 8 == 0,
              "dim_f32_to_bf16: src must be 16-byte and dst 8-byte aligned (vector accesses)");
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(ceil_div((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), src,
                     reinterpret_cast<__bf16*>(dst_bf16), n);
  return check_launch("f32_to_bf16");
}

int dim_bf16_to_f32(const void* src_bf16, float* dst, long n, void* stream) {
  if (n == 0) return DIM_OK;
  DIM_REQUIRE(src_bf16 && dst && n > 0, "null pointer");
  DIM_REQUIRE(reinterpret_cast<uintptr_t>(src_bf16) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0,
              "dim_bf16_to_f32: src must be 8-byte and dst 16-byte aligned (vector accesses)");
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(ceil_div((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const __bf16*>(src_bf16), dst, n);
  return check_launch("bf16_to_f32");
}

// ---- input gradient (the dgrad section of conv.hip has the phase arithmetic and the packed layout)
extern "C++" template <typename PT>
__global__ void pack_dgrad_weight_kernel(const float* __restrict__ w, PT* __restrict__ wp, int Cout, int Cin, int CinPad, int KH, int KW,
                                         int stride, int pad, int py, int px, int nth, int ntw, int eminh, int eminw, int deconv_layout) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)(Cout / 32) * nth * ntw * CinPad * 32;
  if (idx >= total) return;
  int kin = (int)(idx % 32);
  long t = idx / 32;
  int ci = (int)(t % CinPad);
  int kc = (int)(t / CinPad);
  int taps = nth * ntw;
  int cc = kc / taps, tap = kc % taps, jy = tap / ntw, jx = tap % ntw;
  int co = cc * 32 + kin;
  int ky = (stride == 1) ? KH - 1 - jy : py + pad - 2 * (jy + eminh);
  int kx = (stride == 1) ? KW - 1 - jx : px + pad - 2 * (jx + eminw);
  float v = 0.f;
  if (ci < Cin && ky >= 0 && ky < KH && kx >= 0 && kx < KW)
    v = deconv_layout ? w[(((long)ci * Cout + co) * KH + ky) * KW + kx]   // never used (deconv dgrad is a plain forward conv)
                      : w[(((long)co * Cin + ci) * KH + ky) * KW + kx];
  wp[idx] = (PT)v;
}

long dim_conv2d_dgrad_packed_weight_floats(int Cout, int Cin, int KH, int KW, int stride, int pad) {
  int CinPad = (Cin + 63) / 64 * 64;
  long total = 0;
  int nph = stride == 1 ? 1 : 2;
  for (int py = 0; py < nph; ++py)
    for (int px = 0; px < nph; ++px)
      total += (long)(Cout / 32) * dg_axis(KH, stride, pad, py).ntaps * dg_axis(KW, stride, pad, px).ntaps * CinPad * 32;
  return total;
}

// tiled: workgroup = (32-slice cc of Cout, G input channels): rows = w[cc * 32 + r][ci][ky][kx], packed run (phase, jy, jx) at
// phase offset + ((cc * taps + jtap) * CinPad + ci) * 32 -- all phases in one launch through the tap table (<= 32 runs)
extern "C++" template <typename PT>
int dgrad_pack_weight_any(const float* w_oihw, PT* w_packed, int Cout, int Cin, int KH, int KW, int stride, int pad, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null pointer");
  DIM_REQUIRE(stride == 1 || stride == 2, "dgrad supports stride 1 or 2");
  DIM_REQUIRE(Cout % 32 == 0, "Cout must be a multiple of 32 (it is the contraction dimension of dgrad)");
  int CinPad = (Cin + 63) / 64 * 64;
  int nph = stride == 1 ? 1 : 2;
  int runs = 0;
  for (int py = 0; py < nph; ++py)
    for (int px = 0; px < nph; ++px) runs += dg_axis(KH, stride, pad, py).ntaps * dg_axis(KW, stride, pad, px).ntaps;
  const int T = KH * KW, G = runs <= 32 ? wtile_group(CinPad, T, Cout / 32) : 0;
  WTileArgs t = {};
  long off = 0;
  for (int py = 0; py < nph; ++py)
    for (int px = 0; px < nph; ++px) {
      DgAxis ah = dg_axis(KH, stride, pad, py), aw = dg_axis(KW, stride, pad, px);
      long total = (long)(Cout / 32) * ah.ntaps * aw.ntaps * CinPad * 32;
      if (total > 0 && !G) {
        hipLaunchKernelGGL((pack_dgrad_weight_kernel<PT>), dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw,
                           w_packed + off, Cout, Cin, CinPad, KH, KW, stride, pad, py, px, ah.ntaps, aw.ntaps, ah.emin, aw.emin, 0);
      } else if (total > 0) {
        for (int jy = 0; jy < ah.ntaps; ++jy)
          for (int jx = 0; jx < aw.ntaps; ++jx) {
            const int ky = (stride == 1) ? KH - 1 - jy : py + pad - 2 * (jy + ah.emin);
            const int kx = (stride == 1) ? KW - 1 - jx : px + pad - 2 * (jx + aw.emin);
            t.jq[t.nj] = (ky >= 0 && ky < KH && kx >= 0 && kx < KW) ? ky * KW + kx : -1;
            t.jbase[t.nj] = off + (long)(jy * aw.ntaps + jx) * CinPad * 32;
            t.jx[t.nj] = (long)ah.ntaps * aw.ntaps * CinPad * 32;
            ++t.nj;
          }
      }
      off += total;
    }
  if (G && t.nj > 0) {
    t.src = w_oihw; t.dst = w_packed;
    t.G = G; t.Q = T; t.gmax = Cin; t.rmax = Cout; t.g_fast = 1;
    t.sg = T; t.sr = (long)Cin * T; t.rows_x = 32L * Cin * T; t.rows_y = (long)G * T;
    wtile_launch<true, PT>(t, Cout / 32, CinPad / G, as_stream(stream));
  }
  return check_launch("pack_dgrad_weight");
}

int dim_conv2d_dgrad_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, int stride, int pad,
                                 void* stream) {
  return dgrad_pack_weight_any(w_oihw, w_packed, Cout, Cin, KH, KW, stride, pad, stream);
}

int dim_conv2d_dgrad_pack_weight_bf16(const float* w_oihw, void* w_packed_bf16, int Cout, int Cin, int KH, int KW, int stride, int pad,
                                      void* stream) {
  return dgrad_pack_weight_any(w_oihw, reinterpret_cast<__bf16*>(w_packed_bf16), Cout, Cin, KH, KW, stride, pad, stream);
}

long dim_deconv4x4s2_packed_weight_floats(int Cin, int Cout) {
  int CinPad = (Cin + 31) / 32 * 32;
  return 4L * CinPad * 4 * Cout;
}

// tiled: workgroup = (32-slice cc of Cin, G output channels): rows = w[cc * 32 + r][co][ky][kx], packed run (phase, dy, dx) at
// phase * per_phase + ((cc * 4 + tap) * Cout + co) * 32
extern "C++" template <typename PT>
int deconv_pack_weight_any(const float* w_iohw, PT* w_packed, int Cin, int Cout, void* stream) {
  DIM_REQUIRE(w_iohw && w_packed, "null pointer");
  int CinPad = (Cin + 31) / 32 * 32;
  long total = 4L * CinPad * 4 * Cout;
  const int G = wtile_group(Cout, 16, CinPad / 32);
  if (G) {
    WTileArgs t = {};
    const long per_phase = (long)CinPad * 4 * Cout;
    for (int phase = 0; phase < 4; ++phase)
      for (int tap = 0; tap < 4; ++tap) {
        const int py = phase / 2, px = phase % 2, dy = tap / 2, dx = tap % 2;
        t.jq[t.nj] = (py + 2 * (1 - dy)) * 4 + (px + 2 * (1 - dx));
        t.jbase[t.nj] = phase * per_phase + (long)tap * Cout * 32;
        t.jx[t.nj] = 4L * Cout * 32;
        ++t.nj;
      }
    t.src = w_iohw; t.dst = w_packed;
    t.G = G; t.Q = 16; t.gmax = Cout; t.rmax = Cin; t.g_fast = 1;
    t.sg = 16; t.sr = (long)Cout * 16; t.rows_x = 32L * Cout * 16; t.rows_y = (long)G * 16;
    wtile_launch<true, PT>(t, CinPad / 32, Cout / G, as_stream(stream));
  } else {
    hipLaunchKernelGGL((pack_deconv4x4s2_weight_kernel<PT>), dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_iohw, w_packed,
                       Cin, CinPad, Cout);
  }
  return check_launch("pack_deconv_weight");
}

int dim_deconv4x4s2_pack_weight(const float* w_iohw, float* w_packed, int Cin, int Cout, void* stream) {
  return deconv_pack_weight_any(w_iohw, w_packed, Cin, Cout, stream);
}

int dim_deconv4x4s2_pack_weight_bf16(const float* w_iohw, void* w_packed_bf16, int Cin, int Cout, void* stream) {
  return deconv_pack_weight_any(w_iohw, reinterpret_cast<__bf16*>(w_packed_bf16), Cin, Cout, stream);
}

int dim_conv_small_cout_pack_weight(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, void* stream) {
  DIM_REQUIRE(w_oihw && w_packed, "null pointer");
  int CinPad = (Cin + 31) / 32 * 32;
  long total = (long)Cout * KH * KW * CinPad;
  hipLaunchKernelGGL(pack_small_cout_weight_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), w_oihw, w_packed,
                     Cout, Cin, CinPad, KH, KW);
  return check_launch("pack_small_cout_weight");
}

}  // extern "C"
