// Host driver of the sliced Winograd pipelines (winograd.hip: forward F(m x m, 3x3) and 5x5 / stride 2, input gradient of 5x5 / stride 2;
// wino_s2.hip: forward 3x3 / stride 2): input transform -> plane GEMMs (wino_gemm.hip) -> output transform, through one workspace
//   V [T][planes][K]   M [T][planes][Nout]
// Large batches run as several slices of whole images through the same workspace (stream order keeps them apart).
#pragma once
#include <cstdlib>

#include "common.h"

namespace dim {

struct WinoGeom {
  int planes, m;  // transform points per tile, output tile edge
  int th, tw;     // tiles per image
  int K, Nout;    // contraction length and output width of the plane GEMMs
  int N;
  int n_slice;    // images per slice, at most N; 0: one image alone exceeds the 32-bit offsets
  long tiles(int n) const { return (long)n * th * tw; }
  // what a workspace must hold; where no slice exists (the run refuses) it is sized as before, for the whole batch
  long workspace_floats() const { return planes * tiles(n_slice ? n_slice : N) * ((long)K + Nout); }
};

// Ho x Wo: the map that is cut into m x m tiles.  Images per slice: tiles * planes * max(K, Nout) floats of one slice stay below 2^32
// bytes (32-bit buffer offsets in the plane GEMMs)
inline WinoGeom wino_geom(int N, int Ho, int Wo, int planes, int m, int K, int Nout) {
  WinoGeom g = {planes, m, (Ho + m - 1) / m, (Wo + m - 1) / m, K, Nout, N, 0};
  const long limit = 1L << 32, per_image = g.tiles(1) * planes * (K > Nout ? K : Nout) * 4;
  const long cap = per_image < limit ? (limit - 1) / per_image : 0;
  g.n_slice = cap < N ? (int)cap : N;
  return g;
}

inline int wino_record_event(void** events4, int i, hipStream_t st) {
  if (!events4 || !events4[i]) return DIM_OK;
  hipError_t e = hipEventRecord(reinterpret_cast<hipEvent_t>(events4[i]), st);
  return e == hipSuccess ? DIM_OK : set_err(DIM_ERR_LAUNCH, "hipEventRecord: %s", hipGetErrorString(e));
}

// For every slice (images n0 .. n0 + n, T = n * th * tw tiles): plan the GEMM with workgroup tile gemm_tile(T),
//   launch_in(n0, n, T, plan, V)   input transform of the slice's images into V; zeroed = its spare blocks (grid + plan.G - 1) zero the M
//                                  tiles that two stream-K workgroups share
//   launch_out(n0, n, T, M)        output transform of M into the slice's images
// both return their check_launch.  events4: optional 4 hipEvent_t recorded around the three steps of the first slice.
// map: optional item-slot table of the layer (wino_balance.hip); a slice whose plan is not the one it was built for runs without it.
template <class Tile, class In, class Out>
int wino_run_slices(const WinoGeom& g, const float* w_packed, float* workspace, Tile&& gemm_tile, int skip5, bool zeroed, void** events4,
                    hipStream_t st, In&& launch_in, Out&& launch_out, const WinoItemMap* map = nullptr) {
  DIM_REQUIRE(g.n_slice > 0, "one image alone exceeds the 32-bit offsets of the plane GEMMs");
  int n_slice = g.n_slice;
  if (const char* e = getenv("DIM_WINO_MAX_SLICE")) {  // test hook: force the slicing path at sizes a unit test can check
    const int cap = atoi(e);
    if (cap > 0 && cap < n_slice) n_slice = cap;
  }
  for (int n0 = 0; n0 < g.N; n0 += n_slice) {
    const int n = g.N - n0 < n_slice ? g.N - n0 : n_slice;
    const long T = g.tiles(n);
    float* V = workspace;
    float* M = workspace + g.planes * T * g.K;
    void** ev = n0 == 0 ? events4 : nullptr;
    WGemmArgs plan;
    int rc = wino_gemm_plan(&plan, V, w_packed, M, (int)T, g.K, g.Nout, g.planes, gemm_tile(T), skip5);
    if (rc == DIM_OK) plan.sigma = wino_item_map_for(map, plan);
    if (rc == DIM_OK) rc = wino_record_event(ev, 0, st);
    if (rc == DIM_OK) rc = launch_in(n0, n, T, plan, V);
    if (rc == DIM_OK) rc = wino_record_event(ev, 1, st);
    if (rc == DIM_OK) rc = wino_gemm_run(plan, zeroed, st);
    if (rc == DIM_OK) rc = wino_record_event(ev, 2, st);
    if (rc == DIM_OK) rc = launch_out(n0, n, T, M);
    if (rc == DIM_OK) rc = wino_record_event(ev, 3, st);
    if (rc != DIM_OK) return rc;
  }
  return DIM_OK;
}

}  // namespace dim
