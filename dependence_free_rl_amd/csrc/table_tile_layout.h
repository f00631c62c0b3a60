// table_tile_layout.h -- the TILES of the 64-bin 2-D [128,128] train epoch's
// lean table kernels (table_mm_kernels.hip; DESIGN.md §3.0e, "the epoch on the
// table"): the lt::kEntries entries of xh_logit_table.h indexed directly, no
// group records.  Plain C++, host + device: compiled by the kernels, by the
// trainer and by the host check (tests/table_tile_check.cc).
//
// Tile t holds the entries [kR t, kR t + kR); rows from lt::kEntries on (the
// last tile's tail) carry no state: they contribute exactly zero to every sum
// and index no entry of logits, G or part.  kR = 16 gives 37 tiles (592 rows),
// kR = 32 gives 19 (608 rows); both build (-DXH_TT_ROWS=16 / 32).
#ifndef XH_TABLE_TILE_LAYOUT_H_
#define XH_TABLE_TILE_LAYOUT_H_

#include "xh_logit_table.h"

#ifndef XH_TT_ROWS
#define XH_TT_ROWS 16
#endif

namespace xh {
namespace tt {

constexpr int kR = XH_TT_ROWS;                        // rows of a tile
constexpr int kTiles = (lt::kEntries + kR - 1) / kR;  // workgroups of a launch
constexpr int kRows = kTiles * kR;                    // rows with the tail
static_assert(kR == 16 || kR == 32, "a tile: one or two 16-row MFMA tiles");

// entry <-> (tile, row); a tail row has no entry (-1)
XH_LT_HD inline int entry_tile(int e) { return e / kR; }
XH_LT_HD inline int entry_row(int e) { return e % kR; }
XH_LT_HD inline int row_entry(int t, int r) {
  const int e = t * kR + r;
  return e < lt::kEntries ? e : -1;
}
XH_LT_HD inline bool is_tail(int t, int r) { return t * kR + r >= lt::kEntries; }

// the item (0: item_a, 1: item_b) and the bins of entry e (lt::entry's inverse)
XH_LT_HD inline int entry_item(int e) { return e / lt::kStates; }
XH_LT_HD inline void entry_bins(int e, int &b0, int &b1) {
  lt::state_bins(e % lt::kStates, b0, b1);
}

// The order of the sum G_e = sum over the stream's workgroups p of part[p][e]
// (spec8_table_kernels.hip: table_reduce_kernel's order): slice k sums the
// parts k, k + kSlices, ... in double; the slices are summed in slice order, in
// double; one rounding to f32.
constexpr int kSlices = 16;
XH_LT_HD inline double part_slice_sum(const double *part, int nparts, int e, int k) {
  const double *q = part + e;
  const long step = (long)kSlices * lt::kEntries;
  double v = 0.0;
  int p = k;
  // (four loads in flight, the adds in the order of the parts)
  for (; p + 3 * kSlices < nparts; p += 4 * kSlices) {
    const double *b = q + (long)p * lt::kEntries;
    const double a0 = b[0], a1 = b[step], a2 = b[2 * step], a3 = b[3 * step];
    v += a0;
    v += a1;
    v += a2;
    v += a3;
  }
  for (; p < nparts; p += kSlices) v += q[(long)p * lt::kEntries];
  return v;
}
// sl: the entry's kSlices slice sums, `stride` doubles apart
XH_LT_HD inline float part_total(const double *sl, int stride) {
  double t = 0.0;
  for (int u = 0; u < kSlices; ++u) t += sl[(long)u * stride];
  return (float)t;
}

}  // namespace tt
}  // namespace xh

#endif  // XH_TABLE_TILE_LAYOUT_H_
