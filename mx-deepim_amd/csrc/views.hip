// Several calibrated cameras on one object: a batch of B = G x V samples holds G groups (one object instance each) with V views,
// sample b = g V + v; cam_T_rig row b is the rigid X_b = [R_b | t_b] with p_cam = X_b p_rig, and a group has one pose T_g in the rig
// frame, X_b T_g in the camera of sample b.  Restated in float64 numpy by tests/views_reference.py.
//   views_from_rig_kernel   one lane per sample: pose_views[b] = X_b T_g
//   views_consensus_kernel  one lane per group: the eligible view with the best score gives the group's rig pose, and every other
//                           view its pose from that
// Both in float64, rounded once, as track.hip's update kernel; no atomics, no workspace: a replay is bit-identical.
// The joint Gauss-Newton solve over a group's views is gn_solve_views_kernel of twist_solve.h, launched by icp.hip, photo.hip, sil.hip.
#include "common.h"
#include "twist_solve.h"

namespace dim {

__global__ __launch_bounds__(64) void views_from_rig_kernel(const float* __restrict__ pose_rig, const float* __restrict__ cam_T_rig, int B,
                                                           int V, float* __restrict__ pose_views) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double Rx[9], tx[3], Rg[9], tg[3], R[9], t[3];
  rigid_load(cam_T_rig + 12 * (long)b, Rx, tx);
  rigid_load(pose_rig + 12 * (long)(b / V), Rg, tg);
  rigid_mul(Rx, tx, Rg, tg, R, t);
  rigid_store(R, t, pose_views + 12 * (long)b);
}

__global__ __launch_bounds__(64) void views_consensus_kernel(const float* __restrict__ score, const int* __restrict__ status, int fatal_mask,
                                                            const float* pose, const float* __restrict__ cam_T_rig, int G, int V,
                                                            int* __restrict__ choice, float* __restrict__ pose_rig, float* pose_views,
                                                            int* status_out) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const long b0 = (long)g * V;
  int c = -1;
  float best = 0.f;
  for (int v = 0; v < V; ++v) {   // upwards, strictly greater: the lowest v wins a tie
    const float sc = score[b0 + v];
    if (!isfinite(sc) || (status && (status[b0 + v] & fatal_mask) != 0)) continue;
    if (c < 0 || sc > best) {
      c = v;
      best = sc;
    }
  }
  choice[g] = c;
  if (c < 0) {
    if (status_out)
      for (int v = 0; v < V; ++v) status_out[b0 + v] |= DIM_STATUS_VIEWS_NO_CONSENSUS;
    c = 0;
  }
  const long bc = b0 + c;
  float keep[12];   // pose_views may be pose itself: the chosen row is read before anything is written
  for (int k = 0; k < 12; ++k) keep[k] = pose[12 * bc + k];
  double Rc[9], tc[3], Ri[9], ti[3], Rp[9], tp[3], Rg[9], tg[3];
  rigid_load(cam_T_rig + 12 * bc, Rc, tc);
  rigid_inverse(Rc, tc, Ri, ti);
  rigid_load(keep, Rp, tp);
  rigid_mul(Ri, ti, Rp, tp, Rg, tg);
  rigid_store(Rg, tg, pose_rig + 12 * (long)g);
  for (int v = 0; v < V; ++v) {
    float* out = pose_views + 12 * (b0 + v);
    if (v == c) {   // bit for bit
      for (int k = 0; k < 12; ++k) out[k] = keep[k];
      continue;
    }
    double Rx[9], tx[3], R[9], t[3];
    rigid_load(cam_T_rig + 12 * (b0 + v), Rx, tx);
    rigid_mul(Rx, tx, Rg, tg, R, t);   // from the float64 product, not from the rounded pose_rig
    rigid_store(R, t, out);
  }
}

}  // namespace dim

using namespace dim;

extern "C" int dim_views_from_rig(const float* pose_rig, const float* cam_T_rig, int G, int V, float* pose_views, void* stream) {
  DIM_REQUIRE(G > 0 && V >= 1 && V <= kGnMaxViews && (long)G * V <= 0x7fffffffL / 12, "views_from_rig: G = %d, V = %d (V in 1 .. %d)", G, V,
              kGnMaxViews);
  DIM_REQUIRE(pose_rig && cam_T_rig && pose_views, "views_from_rig: null pointer");
  const int B = G * V;
  hipLaunchKernelGGL(views_from_rig_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), pose_rig, cam_T_rig, B, V, pose_views);
  return check_launch("views_from_rig");
}

extern "C" int dim_views_consensus(const float* score, const int* status, int fatal_mask, const float* pose, const float* cam_T_rig, int G,
                                   int V, int* choice, float* pose_rig, float* pose_views, int* status_out, void* stream) {
  DIM_REQUIRE(G > 0 && V >= 1 && V <= kGnMaxViews && (long)G * V <= 0x7fffffffL / 12, "views_consensus: G = %d, V = %d (V in 1 .. %d)", G, V,
              kGnMaxViews);
  DIM_REQUIRE(score && pose && cam_T_rig && choice && pose_rig && pose_views, "views_consensus: null pointer");
  hipLaunchKernelGGL(views_consensus_kernel, dim3(ceil_div(G, 64)), dim3(64), 0, as_stream(stream), score, status, fatal_mask, pose,
                     cam_T_rig, G, V, choice, pose_rig, pose_views, status_out);
  return check_launch("views_consensus");
}
