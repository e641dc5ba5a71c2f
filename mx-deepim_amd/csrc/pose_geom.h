// Float64 pose algebra of the pose errors (metrics.hip, bop.hip) as lib/utils/pose_error.py computes it in numpy.
// The order of the operations is the contract: a transform is ((R0 x + R1 y) + R2 z) + t, the projection is K (R p + t) row by row
// and then two divisions by the third row.  Products and sums are plain operators; the Makefile's -ffp-contract=off keeps them
// un-fused.  Anything else differs from numpy in the last bits.
#pragma once
#include "common.h"

namespace dim {

struct CamK {
  double k[9];
};

// the pair's camera: row b of K_per_sample (B, 9) when given, else the one K of the call
__device__ __forceinline__ CamK cam_k_pick(const CamK& K, const double* __restrict__ K_per_sample, int b) {
  if (!K_per_sample) return K;
  CamK o;
#pragma unroll
  for (int k = 0; k < 9; ++k) o.k[k] = K_per_sample[9L * b + k];
  return o;
}

template <typename PT>
__device__ __forceinline__ void load_pose(const PT* __restrict__ p, double* o) {
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = (double)p[k];
}

__device__ __forceinline__ void transform(const double* P, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  oy = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  oz = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
}

__device__ __forceinline__ void project(const CamK& K, double x, double y, double z, double& u, double& v) {
  const double a = (K.k[0] * x + K.k[1] * y) + K.k[2] * z;
  const double b = (K.k[3] * x + K.k[4] * y) + K.k[5] * z;
  const double c = (K.k[6] * x + K.k[7] * y) + K.k[8] * z;
  u = a / c;
  v = b / c;
}

// class cls -> first row and row count of its points in the table; false (off = n = 0): the index is out of range.  What a table
// that runs backwards (off < 0, n < 0) or an empty class means is the caller's rule.
__device__ __forceinline__ bool class_points(const int* __restrict__ table_off, int n_classes, int cls, int& off, int& n) {
  off = n = 0;
  if (cls < 0 || cls >= n_classes) return false;
  off = table_off[cls];
  n = table_off[cls + 1] - off;
  return true;
}

}  // namespace dim
