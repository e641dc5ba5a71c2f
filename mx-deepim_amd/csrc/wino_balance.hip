// Equal live work per stream-K range for the plane GEMMs of the forward 5x5 / stride-2 layers, without moving a cut.
//
// Under WGemmArgs::skip5 a workgroup multiplies only the chunks of its range whose weight block is not zero, and the live share of an
// item depends on its plane alone (wino5_phase_mask): 25 planes are fully live, 10 half, plane 35 a quarter.  The ranges are cut in the
// flat list of the full K (the results must keep their bits, top of the 5x5 / stride-2 code in winograd.hip), a range lies inside one or
// two planes, so about 70 % of the workgroups carry a full range and the others a half or a quarter of one: the heaviest sets the time.
//
// The table built here is a permutation sigma of the item indices: slot s of the flat list holds item sigma(s).  The list, G, per, rem
// and every boundary stay what they are, and every slot with a boundary strictly inside it is a fixed point.  Hence
//   - the same items are cut at the same chunk into the same two partial sums, added with atomics onto a zeroed tile (a + b on zero does
//     not depend on who adds first), and wino_gemm_zero_tile, which decodes cut slots only, zeroes the same tiles;
//   - a whole item is summed in one accumulator in the same chunk order, by another workgroup or at another time;
// the output is bit-identical.  Only which workgroup multiplies a whole item changes.
//
// Builder (host, deterministic, no GPU work), in two steps:
//   1. counts.  Items come in three weights (4 q, 2 q, q live chunks).  Starting from the identity, the heaviest range trades one whole
//      item for a lighter one of the range that brings the pair's maximum lowest, while that is below the heaviest range's load (the sum
//      of squared loads falls with every trade, so this ends).
//   2. dealing.  A range keeps the items it had as far as its new counts allow; what it gives away are the last whole slots of that
//      weight.  The items given away are dealt in item order to the freed slots in slot order: consecutive ranges receive consecutive
//      items of one plane, and since workgroup numbers are XCD-contiguous a plane's U3 still leaves the fabric about once per XCD.
// The result is the identity when nothing is gained (never a worse maximum), when skip5 is off, or when a range spans more than the 64
// slots a workgroup keeps across the lanes of one register (WTab, common.h).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "wino_driver.h"

namespace dim {

namespace {

struct Balance {
  int nch, q, MT, NTN, items, G, per, rem;
  long first(int w) const { return (long)w * per + std::min(w, rem); }
  int plane(int item) const { return item / NTN / MT; }
  // live chunks of an item of plane p among its chunks [lo, hi)
  int live(int p, int lo, int hi) const {
    const int m = wino5_phase_mask(p);
    int n = 0;
    for (int ph = 0; ph < 4; ++ph)
      if ((m >> ph) & 1) n += std::max(0, std::min(hi, (ph + 1) * q) - std::max(lo, ph * q));
    return n;
  }
  // live work of every range under the table
  void loads(const int* sigma, std::vector<int>& out) const {
    out.assign(G, 0);
    for (int w = 0; w < G; ++w)
      for (long v = first(w), e = first(w + 1); v < e;) {
        const long s = v / nch, base = s * nch;
        out[w] += live(plane(sigma[s]), (int)(v - base), (int)std::min<long>(e - base, nch));
        v = base + nch;
      }
  }
};

int weight_class(int p) {
  const int m = wino5_phase_mask(p);
  return m == 0xF ? 0 : (m == 0x1 ? 2 : 1);
}

}  // namespace

// hdr: kMapWords ints; *table: new int[items], the caller's to delete[]
int wino_item_map_build(int T, int K, int Cout, int tile, int G, int skip5, int* hdr, int** table) {
  const int P = 36;
  int BM, BN;
  wino_tile_shape(&tile, Cout, &BM, &BN);
  DIM_REQUIRE(T > 0 && K > 0 && K % 128 == 0 && Cout % BN == 0, "item map: K %% 128 == 0 and Cout %% 64 == 0 required");
  Balance b;
  b.nch = K / 32;
  b.q = b.nch / 4;
  b.MT = (T + BM - 1) / BM;
  b.NTN = Cout / BN;
  const long items = (long)P * b.MT * b.NTN, total = items * b.nch;
  DIM_REQUIRE(total < (1L << 31), "item map: problem too large for 32-bit chunk indices");
  DIM_REQUIRE(G > 0 && G <= items, "item map: 1 <= G <= items required");
  b.items = (int)items;
  b.G = G;
  b.per = (int)(total / G);
  b.rem = (int)(total % G);

  int* sigma = new int[items];
  for (int s = 0; s < b.items; ++s) sigma[s] = s;
  std::vector<int> load;
  b.loads(sigma, load);
  const int before = *std::max_element(load.begin(), load.end());
  int after = before, moved = 0;

  // whole slots of range w: [lo[w], hi[w])
  std::vector<int> lo(G), hi(G);
  bool fits = true;
  for (int w = 0; w < G; ++w) {
    const long f = b.first(w), e = b.first(w + 1);
    lo[w] = (int)((f + b.nch - 1) / b.nch);
    hi[w] = std::max(lo[w], (int)(e / b.nch));
    fits = fits && ((e - 1) / b.nch - f / b.nch + 1 <= 64);
  }
  if (skip5 && fits && G > 1) {
    const int wt[3] = {4 * b.q, 2 * b.q, b.q};
    std::vector<int> cnt0(3 * G, 0);
    for (int w = 0; w < G; ++w)
      for (int s = lo[w]; s < hi[w]; ++s) ++cnt0[3 * w + weight_class(b.plane(s))];
    std::vector<int> cnt(cnt0);
    // 1. counts
    for (;;) {
      const int h = (int)(std::max_element(load.begin(), load.end()) - load.begin());
      int best = load[h], bl = -1, bch = 0, bcl = 0;
      for (int ch = 0; ch < 2; ++ch) {
        if (!cnt[3 * h + ch]) continue;
        for (int l = 0; l < G; ++l)
          for (int cl = ch + 1; cl < 3; ++cl) {
            if (l == h || !cnt[3 * l + cl]) continue;
            const int d = wt[ch] - wt[cl], m = std::max(load[h] - d, load[l] + d);
            if (m < best) best = m, bl = l, bch = ch, bcl = cl;
          }
      }
      if (bl < 0) break;
      const int d = wt[bch] - wt[bcl];
      --cnt[3 * h + bch], ++cnt[3 * h + bcl], load[h] -= d;
      --cnt[3 * bl + bcl], ++cnt[3 * bl + bch], load[bl] += d;
    }
    // 2. dealing: the slots a range frees (the last ones of a weight it keeps fewer of), their items pooled per weight in item order
    std::vector<int> pool[3], freed;
    for (int w = 0; w < G; ++w) {
      int give[3];
      for (int c = 0; c < 3; ++c) give[c] = std::max(0, cnt0[3 * w + c] - cnt[3 * w + c]);
      const size_t mark = freed.size();
      for (int s = hi[w] - 1; s >= lo[w]; --s) {
        const int c = weight_class(b.plane(s));
        if (give[c] > 0) --give[c], freed.push_back(s);
      }
      std::reverse(freed.begin() + mark, freed.end());
      for (size_t i = mark; i < freed.size(); ++i) pool[weight_class(b.plane(freed[i]))].push_back(freed[i]);
    }
    size_t next[3] = {0, 0, 0}, f = 0;
    for (int w = 0; w < G; ++w)
      for (int c = 0; c < 3; ++c)
        for (int n = std::max(0, cnt[3 * w + c] - cnt0[3 * w + c]); n > 0; --n) sigma[freed[f++]] = pool[c][next[c]++];
    b.loads(sigma, load);
    after = *std::max_element(load.begin(), load.end());
    for (int s = 0; s < b.items; ++s) moved += sigma[s] != s;
    if (after >= before) {  // nothing gained: the launch runs as it always did
      for (int s = 0; s < b.items; ++s) sigma[s] = s;
      after = before;
      moved = 0;
    }
  }
  const int h[kMapWords] = {T, K, Cout, tile, G, b.per, b.rem, before, after, moved, b.items, b.nch};
  std::copy(h, h + kMapWords, hdr);
  *table = sigma;
  return DIM_OK;
}

static int copy_out(const int* hdr, const int* table, int* header, int* out, long capacity) {
  DIM_REQUIRE(header, "null header");
  std::copy(hdr, hdr + kMapWords, header);
  if (out) {
    DIM_REQUIRE(capacity >= hdr[kMapItems], "item map: the table has %d entries, room for %ld", hdr[kMapItems], capacity);
    std::copy(table, table + hdr[kMapItems], out);
  }
  return DIM_OK;
}

}  // namespace dim

using namespace dim;

extern "C" {

int dim_wino_item_map_plan(int T, int K, int Cout, int tile, int G, int skip5, int* header, int* table, long capacity) {
  if (G <= 0) {  // the G of the launch: asks the device
    WGemmArgs a;
    const int rc = wino_gemm_plan(&a, nullptr, nullptr, nullptr, T, K, Cout, 36, tile, skip5);
    if (rc != DIM_OK) return rc;
    G = a.G;
  }
  int hdr[kMapWords], *sigma = nullptr;
  int rc = wino_item_map_build(T, K, Cout, tile, G, skip5, hdr, &sigma);
  if (rc == DIM_OK) rc = copy_out(hdr, sigma, header, table, capacity);
  delete[] sigma;
  return rc;
}

int dim_wino_item_map_create(void** map, int N, int H, int W, int Cin, int Cout, int tile) {
  DIM_REQUIRE(map, "null map pointer");
  *map = nullptr;
  DIM_REQUIRE(N > 0 && H > 0 && W > 0 && Cin % 32 == 0 && Cout % 64 == 0, "Cin %% 32 == 0 and Cout %% 64 == 0 required");
  const WinoGeom g = wino_geom(N, (H + 1) / 2, (W + 1) / 2, 36, 4, 4 * Cin, Cout);
  DIM_REQUIRE(g.n_slice > 0, "one image alone exceeds the 32-bit offsets of the plane GEMMs");
  const long T = g.tiles(g.n_slice);  // the plan of a full slice, as wino_run_slices makes it
  if (!tile) tile = (Cout % 128 == 0 && T >= 1024) ? 4 : 3;
  WGemmArgs a;
  int rc = wino_gemm_plan(&a, nullptr, nullptr, nullptr, (int)T, g.K, Cout, 36, tile, 1);
  if (rc != DIM_OK) return rc;
  WinoItemMap* m = new WinoItemMap();
  m->host = m->dev = nullptr;
  rc = wino_item_map_build((int)T, g.K, Cout, tile, a.G, 1, m->hdr, &m->host);
  if (rc == DIM_OK && m->hdr[kMapMoved] > 0) {
    const size_t bytes = sizeof(int) * (size_t)m->hdr[kMapItems];
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->dev), bytes);
    if (e == hipSuccess) e = hipMemcpy(m->dev, m->host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = set_err(DIM_ERR_LAUNCH, "item map upload: %s", hipGetErrorString(e));
  }
  if (rc != DIM_OK) {
    dim_wino_item_map_destroy(m);
    return rc;
  }
  *map = m;
  return DIM_OK;
}

void dim_wino_item_map_destroy(void* map) {
  WinoItemMap* m = static_cast<WinoItemMap*>(map);
  if (!m) return;
  if (m->dev) (void)hipFree(m->dev);
  delete[] m->host;
  delete m;
}

int dim_wino_item_map_query(const void* map, int* header, int* table, long capacity) {
  const WinoItemMap* m = static_cast<const WinoItemMap*>(map);
  DIM_REQUIRE(m, "null map");
  return copy_out(m->hdr, m->host, header, table, capacity);
}

}  // extern "C"
