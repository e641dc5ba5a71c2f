// Float64 sums across lanes in an order that never changes, so that a replay is bit-identical: the workgroup sum of the accumulate
// kernels (icp.hip, flow_pnp.hip, photo.hip, sil.hip, vsd.hip) and the 64-lane butterflies (hyp.hip, metrics.hip).
#pragma once
#include "common.h"

namespace dim {

// Sum of TERMS float64 values per lane over a 256-lane workgroup: lane k < TERMS returns the total of term k (the other lanes 0).
// Order: 8 chunks of 32 lanes per term (chunk tid >> 5, a chunk row padded to 33 doubles against bank conflicts), the 32 lanes of a
// chunk added in lane order, then the 8 chunk sums in chunk order.  (A shuffle butterfly per term -- 29 chains of 6 dependent 64-bit
// lane exchanges -- cost more than the pixels of an ICP iteration.)  Every lane of the workgroup must call it.
template <int TERMS>
__device__ __forceinline__ double block_sum(const double (&v)[TERMS]) {
  static_assert(TERMS * 8 <= 256, "one lane per (term, chunk)");
  constexpr int kRow = 8 * 33;   // LDS doubles per term
  __shared__ double red[TERMS * kRow];
  __shared__ double red8[TERMS * 8];
  const int tid = threadIdx.x;
  const int slot = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int k = 0; k < TERMS; ++k) red[k * kRow + slot] = v[k];
  __syncthreads();
  if (tid < TERMS * 8) {
    const double* r = red + (tid >> 3) * kRow + (tid & 7) * 33;
    double s = 0.0;
    for (int j = 0; j < 32; ++j) s += r[j];
    red8[tid] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (tid < TERMS) {
    s = red8[8 * tid];
    for (int w = 1; w < 8; ++w) s += red8[8 * tid + w];
  }
  return s;
}

// xor butterflies over the 64 lanes of a wave: every lane ends with the result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace dim
