// Float64 device helpers shared by the Gauss-Newton pose stages (icp.hip, flow_pnp.hip) and the pose algebra (se3.hip): the 6x6
// Cholesky solve of the normal equations, the Rodrigues rotation of a twist's omega, and rotation matrix -> quaternion.
#pragma once
#include "common.h"

namespace dim {

__device__ inline void twist_rodrigues(const double* w, double* Rw) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double Wx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double a = 1.0, bq = 0.0;
  if (th >= 1e-12) {
    a = sin(th) / th;
    bq = (1.0 - cos(th)) / (th * th);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double w2 = 0.0;
      for (int k = 0; k < 3; ++k) w2 += Wx[3 * i + k] * Wx[3 * k + j];
      Rw[3 * i + j] = (i == j ? 1.0 : 0.0) + a * Wx[3 * i + j] + bq * w2;
    }
}

// -> false when A is not positive definite
__device__ inline bool cholesky_solve6(const double* A, const double* rhs, double* x) {
  double L[36] = {};
  for (int j = 0; j < 6; ++j) {
    double s = A[6 * j + j];
    for (int k = 0; k < j; ++k) s -= L[6 * j + k] * L[6 * j + k];
    if (!(s > 0.0)) return false;
    L[6 * j + j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
      for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = v / L[6 * j + j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = rhs[i];
    for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
    y[i] = v / L[6 * i + i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * x[k];
    x[i] = v / L[6 * i + i];
  }
  return true;
}

// rotation matrix -> (w,x,y,z), w >= 0.  The reference takes the dominant eigenvector of the
// Bar-Itzhack matrix (mat2quat, RT_transform.py:446-523); for a rotation matrix that vector is
// the usual quaternion, computed here with Shepperd's branch selection and normalised.
__device__ inline void mat2quat_d(const double M[9], double q[4]) {
  double tr = M[0] + M[4] + M[8];
  double w, x, y, z;
  if (tr > M[0] && tr > M[4] && tr > M[8]) {
    w = 1.0 + tr; x = M[7] - M[5]; y = M[2] - M[6]; z = M[3] - M[1];
  } else if (M[0] > M[4] && M[0] > M[8]) {
    x = 1.0 + M[0] - M[4] - M[8]; w = M[7] - M[5]; y = M[1] + M[3]; z = M[2] + M[6];
  } else if (M[4] > M[8]) {
    y = 1.0 - M[0] + M[4] - M[8]; w = M[2] - M[6]; x = M[1] + M[3]; z = M[5] + M[7];
  } else {
    z = 1.0 - M[0] - M[4] + M[8]; w = M[3] - M[1]; x = M[2] + M[6]; y = M[5] + M[7];
  }
  double n = sqrt(w * w + x * x + y * y + z * z);
  if (w < 0) n = -n;
  q[0] = w / n; q[1] = x / n; q[2] = y / n; q[3] = z / n;
}

}  // namespace dim
