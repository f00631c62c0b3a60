// spec8_table_layout.h -- the TABLE BATCH of the 64-bin 2-D [128,128] train
// epoch ("the epoch on the table"): the per-bin net sees only
// (bin state, item), lt::kEntries points (xh_logit_table.h), so an epoch's
// matrix work runs over one static batch that holds every point once, in the
// group format of spec8_pack_layout.h.  Plain C++, host + device: compiled by
// the kernels, by the trainer (which writes the batch once) and by the host
// check (tests/train_table_batch_check.cc).
//
// kGroups = 10 groups of 64 rows, kGroupsPerItem = 5 per item, item_a's first.
// Row r of group g carries state number (g % 5) * 64 + r of item g / 5, in
// lt::state_index order; numbers from lt::kStates on (the tail of each item's
// last group) carry no state: bins 0, count 0.  Real rows have count 1.  The
// four segment records are the empty one (cu = -1, pold = 1, adv = 0): the
// table build of policy_spec8_kernels.hip reads no record.
#ifndef XH_SPEC8_TABLE_LAYOUT_H_
#define XH_SPEC8_TABLE_LAYOUT_H_

#include <cstdint>
#include <cstring>

#include "spec8_pack_layout.h"
#include "xh_logit_table.h"

namespace xh {
namespace tb {

constexpr int kRows = sp8::kPkSegs * sp8::kPkSegRows;              // rows of a group
constexpr int kGroupsPerItem = (lt::kStates + kRows - 1) / kRows;  // 5
constexpr int kGroups = lt::kItems * kGroupsPerItem;               // 10
constexpr int kBytes = kGroups * sp8::kPkGroupBytes;

// The enumeration: the item of group g, and the table entry of its row r (-1:
// a tail row, no state).
XH_LT_HD inline int group_item(int g) { return g / kGroupsPerItem; }
XH_LT_HD inline int row_entry(int g, int r) {
  const int s = (g % kGroupsPerItem) * kRows + r;
  return s < lt::kStates ? group_item(g) * lt::kStates + s : -1;
}
// Its inverse: the group and the row that carry table entry e.
XH_LT_HD inline int entry_group(int e) {
  return (e / lt::kStates) * kGroupsPerItem + (e % lt::kStates) / kRows;
}
XH_LT_HD inline int entry_row(int e) { return (e % lt::kStates) % kRows; }

// Group g's record (sp8::kPkGroupBytes bytes at rec).
inline void fill_group(int g, uint8_t *rec) {
  std::memset(rec, 0, sp8::kPkGroupBytes);
  for (int r = 0; r < kRows; ++r) {
    const int e = row_entry(g, r);
    if (e < 0) continue;
    int b0, b1;
    lt::state_bins(e % lt::kStates, b0, b1);
    rec[sp8::kPkStates + 2 * r] = (uint8_t)(int8_t)b0;
    rec[sp8::kPkStates + 2 * r + 1] = (uint8_t)(int8_t)b1;
    rec[sp8::kPkCounts + r] = 1;
  }
  const sp8::PkSeg none{-1, 1.0f, 0.0f, -1};
  for (int q = 0; q < sp8::kPkSegs; ++q)
    std::memcpy(rec + sp8::kPkSegRecs + q * sizeof(sp8::PkSeg), &none, sizeof(none));
}

}  // namespace tb
}  // namespace xh

#endif  // XH_SPEC8_TABLE_LAYOUT_H_
