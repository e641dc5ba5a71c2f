// Decoder and pose heads (source map: conv_impl.h)
#include "common.h"

namespace dim {

// Convolution with a handful of output channels (flow / mask heads, Cout <= 2).  HBM/L2-bound on the activations; weights (Cout,Cin,3,3
// MXNet layout) are re-packed to [Cout][kh][kw][CinPad].  A wave owns PX horizontally adjacent output pixels; a lane strides the channel
// quads (float4), and for every quad and kernel row loads the PX + KW - 1 input pixels of the row and the KW x COUT weight quads ONCE
// for all PX outputs; PX x COUT wave reductions at the end.  History at 16 x 30 x 40 x 770 -> 2 / -> 1: one wave per output pixel (1 + COUT
// float4 loads per 4 COUT multiply-adds: 55 KB of weights + 28 KB of activations per pixel through the vector L1): 36 / 50 us; four
// pixels per wave: 34 / 29 us at 60 % of the chip's vector-memory issue rate; the weights staged in LDS per workgroup with eight pixels
// per wave: 57 / 32 us (60 KB of staging for 32 pixels, two workgroups per CU) -- dropped.
template <int COUT, int KW, int PX>
__global__ __launch_bounds__(256) void conv_small_cout_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                              const float* __restrict__ bias, float* __restrict__ y, int N, int H,
                                                              int W, int CinPad, int in_cstride, int KH, int pad, int out_cstride,
                                                              int out_coff) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c4 = CinPad >> 2;
  const int segs = (W + PX - 1) / PX;   // pixel groups per row
  // XCD-contiguous numbering: neighbouring groups read the same input rows; in launch order they sit on eight different L2s
  const long grp = (long)wg_xcd_contiguous((int)blockIdx.x, (int)gridDim.x) * 4 + wave;
  if (grp >= (long)N * H * segs) return;
  const int wo0 = (int)(grp % segs) * PX;
  const int ho = (int)((grp / segs) % H);
  const int n = (int)(grp / ((long)segs * H));
  float acc[PX][COUT];
#pragma unroll
  for (int p = 0; p < PX; ++p)
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[p][c] = 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int kh = 0; kh < KH; ++kh) {
    const int hi = ho - pad + kh;
    if ((unsigned)hi >= (unsigned)H) continue;   // wave-uniform
    const float* xrow = x + (long)(n * H + hi) * W * in_cstride;
    for (int i = lane; i < c4; i += 64) {
      float4 xv[PX + KW - 1], wv[KW][COUT];
#pragma unroll
      for (int q = 0; q < PX + KW - 1; ++q) {
        const int wi = wo0 - pad + q;
        const bool ok = (unsigned)wi < (unsigned)W;   // wave-uniform; clamped address + select keeps the loads branch-free
        const float4 v = reinterpret_cast<const float4*>(xrow + (long)(ok ? wi : 0) * in_cstride)[i];
        xv[q] = ok ? v : zero;
      }
#pragma unroll
      for (int kw = 0; kw < KW; ++kw)
#pragma unroll
        for (int c = 0; c < COUT; ++c) wv[kw][c] = reinterpret_cast<const float4*>(wp + ((long)(c * KH + kh) * KW + kw) * CinPad)[i];
#pragma unroll
      for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int kw = 0; kw < KW; ++kw)
#pragma unroll
          for (int c = 0; c < COUT; ++c) {
            const float4 v = xv[p + kw], w4 = wv[kw][c];
            acc[p][c] = fmaf(v.x, w4.x, fmaf(v.y, w4.y, fmaf(v.z, w4.z, fmaf(v.w, w4.w, acc[p][c]))));
          }
    }
  }
#pragma unroll
  for (int p = 0; p < PX; ++p)
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
      float v = acc[p][c];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0 && wo0 + p < W) y[((long)(n * H + ho) * W + wo0 + p) * out_cstride + out_coff + c] = v + (bias ? bias[c] : 0.f);
    }
}

// Deconvolution(k=4, s=2, p=0) on a tiny channel count (upsample_flow6to5 / 5to4: 2 -> 2) + Crop(offset) written into a
// concat buffer.  x (N,H,W,xstride) NHWC; w (Cin,Cout,4,4) MXNet layout; out pixel (oy,ox) <- full-res (oy+crop, ox+crop).
__global__ void deconv4x4s2_tiny_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                        float* __restrict__ y, int N, int H, int W, int Cin, int xstride, int Cout, int OH, int OW,
                                        int crop, int out_cstride, int out_coff) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)N * OH * OW * Cout;
  if (idx >= total) return;
  int co = (int)(idx % Cout);
  long t = idx / Cout;
  int ox = (int)(t % OW); t /= OW;
  int oy = (int)(t % OH);
  int n = (int)(t / OH);
  int fy = oy + crop, fx = ox + crop;
  float acc = bias ? bias[co] : 0.f;
  for (int ky = fy & 1; ky < 4; ky += 2) {
    int iy = (fy - ky) >> 1;
    if ((unsigned)iy >= (unsigned)H) continue;
    for (int kx = fx & 1; kx < 4; kx += 2) {
      int ix = (fx - kx) >> 1;
      if ((unsigned)ix >= (unsigned)W) continue;
      const float* xs = x + ((long)(n * H + iy) * W + ix) * xstride;
      for (int ci = 0; ci < Cin; ++ci) acc = fmaf(xs[ci], w[(((long)ci * Cout + co) * 4 + ky) * 4 + kx], acc);
    }
  }
  y[((long)(n * OH + oy) * OW + ox) * out_cstride + out_coff + co] = acc;
}

// Deconvolution(k=32, s=16, group = C, no bias) + Crop(offset 8,8): the frozen bilinear x16 upsampling of the flow / mask heads
// (deepIM_flownet.py:326-340, :513-529).  x (N,h,w,C) NHWC; wk (C,1,32,32); y (N,C,OH,OW) NCHW planes.
// mode 0: plain * scale   mode 1: sigmoid (mask probability)
__global__ __launch_bounds__(256) void upsample16_kernel(const float* __restrict__ x, const float* __restrict__ wk, float* __restrict__ y,
                                                         int C, int h, int w, int OH, int OW, int crop, float scale, int mode) {
  const int n = blockIdx.z / C, c = blockIdx.z % C;
  const int oy = blockIdx.y;
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  if (ox >= OW) return;
  const int fy = oy + crop, fx = ox + crop;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    int iy = (fy >> 4) - a;
    int ky = fy - 16 * iy;  // in [0,32)
    if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      int ix = (fx >> 4) - b;
      int kx = fx - 16 * ix;
      if ((unsigned)ix >= (unsigned)w) continue;
      acc = fmaf(x[((long)(n * h + iy) * w + ix) * C + c], wk[((long)c * 32 + ky) * 32 + kx], acc);
    }
  }
  acc *= scale;
  if (mode == 1) acc = 1.f / (1.f + expf(-acc));
  y[(((long)n * C + c) * OH + oy) * OW + ox] = acc;
}

// the same for four adjacent output pixels per thread (crop % 4 == 0, OW % 4 == 0, 16-byte aligned rows): they share their 2 x 2 input
// pixels, the kernel taps are one float4 per (ky, b), the store is one float4.  One output per thread: 32 + 19 us for the two heads at
// 16 x 480 x 640 (1.2 / 1.0 TB/s of output).
__global__ __launch_bounds__(256) void upsample16_x4_kernel(const float* __restrict__ x, const float* __restrict__ wk, float* __restrict__ y,
                                                            int C, int h, int w, int OH, int OW, int crop, float scale, int mode) {
  const int n = blockIdx.z / C, c = blockIdx.z % C;
  const int oy = blockIdx.y;
  const int ox = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (ox >= OW) return;
  const int fy = oy + crop, fx = ox + crop;   // fx % 4 == 0: fx .. fx + 3 share their 16-block
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int iy = (fy >> 4) - a;
    const int ky = fy - 16 * iy;  // in [0,32)
    if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ix = (fx >> 4) - b;
      const int kx = fx - 16 * ix;   // multiple of 4
      if ((unsigned)ix >= (unsigned)w) continue;
      const float xv = x[((long)(n * h + iy) * w + ix) * C + c];
      const float4 k4 = *reinterpret_cast<const float4*>(wk + ((long)c * 32 + ky) * 32 + kx);
      acc.x = fmaf(xv, k4.x, acc.x);
      acc.y = fmaf(xv, k4.y, acc.y);
      acc.z = fmaf(xv, k4.z, acc.z);
      acc.w = fmaf(xv, k4.w, acc.w);
    }
  }
  acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
  if (mode == 1) {
    acc.x = 1.f / (1.f + expf(-acc.x)); acc.y = 1.f / (1.f + expf(-acc.y));
    acc.z = 1.f / (1.f + expf(-acc.z)); acc.w = 1.f / (1.f + expf(-acc.w));
  }
  *reinterpret_cast<float4*>(y + (((long)n * C + c) * OH + oy) * OW + ox) = acc;
}

// Pose head: fc7 + LeakyReLU + rot (4) + trans (3) + inverse ZoomTrans -> se3 (B,7).
// deepIM_flownet.py:203-208, :956-971; zoom_trans.py:37-41 (b_inv_zoom: dx*wx, dy*wx).
// CLS (network.REGRESSOR_NUM = K > 1): wr (4K,256) / br (4K) / wt (3K,256) / bt (3K) hold one head per class and the sample reads the
// rows of class_index[b] -- a workgroup-uniform offset (one scalar load and an add), everything after it is the shared head's code,
// so a sample's se3 is bit for bit the shared kernel's with that class's slice.  A class outside [0, K): identity delta + status bit.
template <bool CLS>
__device__ __forceinline__ void pose_head_body(const float* __restrict__ fc6, const float* __restrict__ w7, const float* __restrict__ b7,
                                               const float* __restrict__ wr, const float* __restrict__ br, const float* __restrict__ wt,
                                               const float* __restrict__ bt, const int* __restrict__ class_index, int n_regressors,
                                               const float* __restrict__ zoom_factor, float* __restrict__ se3,
                                               float* __restrict__ fc7_out, int* __restrict__ status) {
  __shared__ float s_h[256];
  const int b = blockIdx.x, t = threadIdx.x;
  bool bad_class = false;
  if constexpr (CLS) {
    const int c = class_index[b];
    bad_class = (unsigned)c >= (unsigned)n_regressors;
    if (!bad_class) {
      wr += (long)c * 4 * 256; br += c * 4;
      wt += (long)c * 3 * 256; bt += c * 3;
    } else if (t == 0 && status) {
      status[b] |= DIM_STATUS_BAD_CLASS;
    }
  }
  const int wave = t >> 6, lane = t & 63;
  // fc7 (256 x 256): for each output the 64 lanes of a wave read the weight row as one coalesced 1 KB load (a float4 per lane against
  // the lane's own four fc6 values) and fold their partial dots with a fixed shuffle tree.  (The first version gave every thread one
  // output and let it walk its row alone: 64 cache lines per wave-load, 256 loads per thread, 15-16 us for 16 samples.)
  // (16-byte loads when fc6 and w7 are 16-byte aligned; a flat parameter blob may place w7 on any 4-byte boundary: scalar loads then)
  const bool al = ((reinterpret_cast<uintptr_t>(fc6) | reinterpret_cast<uintptr_t>(w7)) & 15) == 0;
  const float* xr = fc6 + (long)b * 256 + 4 * lane;
  const float4 xin = al ? *reinterpret_cast<const float4*>(xr) : make_float4(xr[0], xr[1], xr[2], xr[3]);
  // 16 waves x 16 outputs: every wave issues its 16 row loads before the first use -- one memory round trip for the layer (with 4 rows
  // at a time on 4 waves the kernel still took 16 us: sixteen round trips in series)
  {
    const int o0 = wave * 16;
    float4 wv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const float* wr_ = w7 + (long)(o0 + u) * 256 + 4 * lane;
      wv[u] = al ? *reinterpret_cast<const float4*>(wr_) : make_float4(wr_[0], wr_[1], wr_[2], wr_[3]);
    }
    float p[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) p[u] = fmaf(xin.w, wv[u].w, fmaf(xin.z, wv[u].z, fmaf(xin.y, wv[u].y, xin.x * wv[u].x)));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < 16; ++u) p[u] += __shfl_down(p[u], off, 64);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        float acc = p[u] + b7[o0 + u];
        acc = acc > 0.f ? acc : 0.1f * acc;
        s_h[o0 + u] = acc;
        if (fc7_out) fc7_out[(long)b * 256 + o0 + u] = acc;
      }
    }
  }
  __syncthreads();
  // 7 outputs, one wave each would be overkill: 7 x 64-lane partial dot + shuffle reduce
  for (int o = wave; o < 7; o += 16) {
    const float* wv = (o < 4) ? (wr + o * 256) : (wt + (o - 4) * 256);
    float p = 0.f;
    for (int k = lane; k < 256; k += 64) p = fmaf(s_h[k], wv[k], p);
    for (int off = 32; off > 0; off >>= 1) p += __shfl_down(p, off, 64);
    if (lane == 0) {
      float v = p + ((o < 4) ? br[o] : bt[o - 4]);
      if (o == 4 || o == 5) v = v * zoom_factor[b * 4 + 0];
      if (CLS && bad_class) v = o == 0 ? 1.f : 0.f;
      se3[b * 7 + o] = v;
    }
  }
}

__global__ __launch_bounds__(1024) void pose_head_kernel(const float* __restrict__ fc6, const float* __restrict__ w7,
                                                         const float* __restrict__ b7, const float* __restrict__ wr,
                                                         const float* __restrict__ br, const float* __restrict__ wt,
                                                         const float* __restrict__ bt, const float* __restrict__ zoom_factor,
                                                         float* __restrict__ se3, float* __restrict__ fc7_out) {
  pose_head_body<false>(fc6, w7, b7, wr, br, wt, bt, nullptr, 1, zoom_factor, se3, fc7_out, nullptr);
}

__global__ __launch_bounds__(1024) void pose_head_cls_kernel(const float* __restrict__ fc6, const float* __restrict__ w7,
                                                             const float* __restrict__ b7, const float* __restrict__ wr,
                                                             const float* __restrict__ br, const float* __restrict__ wt,
                                                             const float* __restrict__ bt, const int* __restrict__ class_index,
                                                             int n_regressors, const float* __restrict__ zoom_factor,
                                                             float* __restrict__ se3, float* __restrict__ fc7_out,
                                                             int* __restrict__ status) {
  pose_head_body<true>(fc6, w7, b7, wr, br, wt, bt, class_index, n_regressors, zoom_factor, se3, fc7_out, status);
}

}  // namespace dim

using namespace dim;

extern "C" {

int dim_conv_small_cout_fwd(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin,
                            int in_cstride, int Cout, int KH, int KW, int pad, int out_cstride, int out_coff, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(x && w_packed && y, "null pointer");
  DIM_REQUIRE(Cout == 1 || Cout == 2, "small-Cout kernel handles Cout 1 or 2 (got %d)", Cout);
  int CinPad = (Cin + 31) / 32 * 32;
  DIM_REQUIRE(in_cstride >= CinPad && in_cstride % 4 == 0, "in_cstride must cover the padded channel count");
  DIM_REQUIRE(KW == 3 || KW == 1, "small-Cout kernel is built for 3- and 1-wide kernels (got KW = %d)", KW);
  constexpr int PX = 4;   // eight pixels per wave halve the wave count of these small maps: 42 / 31 / 22 / 18 us against 34 / 28 / 17 / 11
  const long groups = (long)N * H * ((W + PX - 1) / PX);
  dim3 grid(ceil_div(groups, 4)), block(256);
#define DIM_SMALL_COUT(CO, KWc)                                                                                                           \
  hipLaunchKernelGGL((conv_small_cout_kernel<CO, KWc, PX>), grid, block, 0, as_stream(stream), x, w_packed, bias, y, N, H, W, CinPad,     \
                     in_cstride, KH, pad, out_cstride, out_coff)
  if (Cout == 1) { if (KW == 3) DIM_SMALL_COUT(1, 3); else DIM_SMALL_COUT(1, 1); }
  else { if (KW == 3) DIM_SMALL_COUT(2, 3); else DIM_SMALL_COUT(2, 1); }
#undef DIM_SMALL_COUT
  return check_launch("conv_small_cout");
}

int dim_deconv4x4s2_tiny_fwd(const float* x, const float* w_iohw, const float* bias, float* y, int N, int H, int W, int Cin,
                             int in_cstride, int Cout, int OH, int OW, int crop, int out_cstride, int out_coff, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(x && w_iohw && y, "null pointer");
  long total = (long)N * OH * OW * Cout;
  hipLaunchKernelGGL(deconv4x4s2_tiny_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), x, w_iohw, bias, y, N, H,
                     W, Cin, in_cstride, Cout, OH, OW, crop, out_cstride, out_coff);
  return check_launch("deconv_tiny");
}

int dim_upsample16_fwd(const float* x_nhwc, const float* w_c1_32_32, float* y_nchw, int N, int C, int h, int w, int OH, int OW,
                       int crop, float scale, int mode, void* stream) {
  if (N == 0) return DIM_OK;
  DIM_REQUIRE(x_nhwc && w_c1_32_32 && y_nchw, "null pointer");
  DIM_REQUIRE(mode == 0 || mode == 1, "mode 0 (linear) or 1 (sigmoid)");
  DIM_REQUIRE(OH + crop <= 16 * h + 16 && OW + crop <= 16 * w + 16, "crop window outside the deconvolution output");
  if (crop % 4 == 0 && OW % 4 == 0 && (reinterpret_cast<uintptr_t>(y_nchw) & 15) == 0 && (reinterpret_cast<uintptr_t>(w_c1_32_32) & 15) == 0)
    hipLaunchKernelGGL(upsample16_x4_kernel, dim3(ceil_div(OW / 4, 256), OH, N * C), dim3(256), 0, as_stream(stream), x_nhwc, w_c1_32_32,
                       y_nchw, C, h, w, OH, OW, crop, scale, mode);
  else
    hipLaunchKernelGGL(upsample16_kernel, dim3(ceil_div(OW, 256), OH, N * C), dim3(256), 0, as_stream(stream), x_nhwc, w_c1_32_32,
                       y_nchw, C, h, w, OH, OW, crop, scale, mode);
  return check_launch("upsample16");
}

int dim_pose_head_fwd(const float* fc6, const float* fc7_w, const float* fc7_b, const float* rot_w, const float* rot_b,
                      const float* trans_w, const float* trans_b, const float* zoom_factor, float* se3, float* fc7_out, int B,
                      void* stream) {
  DIM_REQUIRE(fc6 && fc7_w && fc7_b && rot_w && rot_b && trans_w && trans_b && zoom_factor && se3, "null pointer");
  if (B == 0) return DIM_OK;
  hipLaunchKernelGGL(pose_head_kernel, dim3(B), dim3(1024), 0, as_stream(stream), fc6, fc7_w, fc7_b, rot_w, rot_b, trans_w,
                     trans_b, zoom_factor, se3, fc7_out);
  return check_launch("pose_head");
}

int dim_pose_head_fwd_cls(const float* fc6, const float* fc7_w, const float* fc7_b, const float* rot_w, const float* rot_b,
                          const float* trans_w, const float* trans_b, const int* class_index, int n_regressors,
                          const float* zoom_factor, float* se3, float* fc7_out, int* status, int B, void* stream) {
  DIM_REQUIRE(n_regressors >= 1, "n_regressors must be >= 1 (got %d)", n_regressors);
  if (n_regressors == 1) return dim_pose_head_fwd(fc6, fc7_w, fc7_b, rot_w, rot_b, trans_w, trans_b, zoom_factor, se3, fc7_out, B, stream);
  DIM_REQUIRE(fc6 && fc7_w && fc7_b && rot_w && rot_b && trans_w && trans_b && zoom_factor && se3, "null pointer");
  DIM_REQUIRE(class_index, "class_index is required with n_regressors > 1");
  if (B == 0) return DIM_OK;
  hipLaunchKernelGGL(pose_head_cls_kernel, dim3(B), dim3(1024), 0, as_stream(stream), fc6, fc7_w, fc7_b, rot_w, rot_b, trans_w, trans_b,
                     class_index, n_regressors, zoom_factor, se3, fc7_out, status);
  return check_launch("pose_head_cls");
}

}  // extern "C"
