// CPU check of the lean table kernels' tiles
// (dependence_free_rl_amd/csrc/table_tile_layout.h): the entry <-> (tile, row)
// maps are inverses over all 578 entries, every entry sits in exactly one
// (tile, row), the tail rows are reported as such and have no entry, an entry's
// item and bins are lt::entry's inverse, and the order of the part sum
// (part_slice_sum / part_total) equals a restatement of table_reduce_kernel's
// (wave k sums the parts k, k + 16, ... in double; the 16 sums in wave order, in
// double; one rounding) for nparts in {1, 5, 15, 16, 17, 64, 256}.
// Built for the shipped tile height and, with -DXH_TT_ROWS, for the other one.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "table_tile_layout.h"

using namespace xh;

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);     \
      return 1;                                              \
    }                                                        \
  } while (0)

// table_reduce_kernel, restated: thread (k, lane) of the workgroup that owns
// the entry, then wave 0
static float reduce_restated(const std::vector<double> &part, int nparts, int e) {
  double sc[16];
  for (int k = 0; k < 16; ++k) {
    double v = 0.0;
    for (int p = k; p < nparts; p += 16) v += part[(size_t)p * lt::kEntries + e];
    sc[k] = v;
  }
  double t = 0.0;
  for (int u = 0; u < 16; ++u) t += sc[u];
  return (float)t;
}

int main() {
  CHECK(lt::kEntries == 578);
  CHECK(tt::kR == 16 || tt::kR == 32);
  CHECK(tt::kTiles == (tt::kR == 16 ? 37 : 19));
  CHECK(tt::kRows == (tt::kR == 16 ? 592 : 608));
  CHECK(tt::kSlices == 16);
  std::vector<int> seen(lt::kEntries, 0);
  int tail = 0;
  for (int t = 0; t < tt::kTiles; ++t)
    for (int r = 0; r < tt::kR; ++r) {
      const int e = tt::row_entry(t, r);
      if (tt::is_tail(t, r)) {
        CHECK(e == -1);
        CHECK(t == tt::kTiles - 1);  // the tail is the last tile's
        ++tail;
        continue;
      }
      CHECK(e >= 0 && e < lt::kEntries);
      CHECK(e == t * tt::kR + r);
      CHECK(tt::entry_tile(e) == t && tt::entry_row(e) == r);
      int b0, b1;
      tt::entry_bins(e, b0, b1);
      CHECK(b0 >= -lt::kCap && b0 <= lt::kCap && b1 >= -lt::kCap && b1 <= lt::kCap);
      CHECK(lt::entry(tt::entry_item(e), b0, b1) == e);
      ++seen[e];
    }
  for (int e = 0; e < lt::kEntries; ++e) {
    CHECK(seen[e] == 1);
    CHECK(tt::row_entry(tt::entry_tile(e), tt::entry_row(e)) == e);
    CHECK(!tt::is_tail(tt::entry_tile(e), tt::entry_row(e)));
  }
  CHECK(tail == tt::kRows - lt::kEntries && tail < tt::kR);

  // the part sum: values of mixed sign and widely mixed size, so that another
  // order of the double sums rounds differently
  const int np_list[] = {1, 5, 15, 16, 17, 64, 256};
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  int differs_from_linear = 0;
  for (int nparts : np_list) {
    std::vector<double> part((size_t)nparts * lt::kEntries);
    for (auto &v : part) {
      const uint64_t u = next();
      const double m = (double)(int64_t)(u >> 11) / 9007199254740992.0 - 0.25;
      v = m * (double)(1ull << (u & 31)) / 65536.0;
    }
    for (int e = 0; e < lt::kEntries; ++e) {
      double sl[tt::kSlices];
      for (int k = 0; k < tt::kSlices; ++k) sl[k] = tt::part_slice_sum(part.data(), nparts, e, k);
      // (the kernel keeps the slice sums tt::kR doubles apart: any stride)
      const float got = tt::part_total(sl, 1);
      const float want = reduce_restated(part, nparts, e);
      CHECK(got == want);
      double lin = 0.0;
      for (int p = 0; p < nparts; ++p) lin += part[(size_t)p * lt::kEntries + e];
      differs_from_linear += lin != [&] {
        double t = 0.0;
        for (int k = 0; k < tt::kSlices; ++k) t += sl[k];
        return t;
      }();
    }
    // slices past nparts are empty
    for (int k = nparts; k < tt::kSlices; ++k)
      CHECK(tt::part_slice_sum(part.data(), nparts, 0, k) == 0.0);
  }
  CHECK(differs_from_linear > 0);  // the data does tell the orders apart
  std::printf("table tiles: ok (R = %d, %d tiles, %d tail rows)\n", tt::kR, tt::kTiles, tail);
  return 0;
}
