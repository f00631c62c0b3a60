// CPU check of the train epoch's table batch
// (dependence_free_rl_amd/csrc/spec8_table_layout.h): the ten group records
// cover each of the 578 table entries exactly once with count 1, the tail rows
// have count 0, every record is an empty-segment one, and the enumeration
// (row_entry) and lt::entry / entry_group / entry_row are inverses.
#include <cstdio>
#include <cstring>
#include <vector>

#include "spec8_table_layout.h"

using namespace xh;

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);     \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  CHECK(tb::kRows == 64 && tb::kGroupsPerItem == 5 && tb::kGroups == 10);
  CHECK(lt::kEntries == 578);
  std::vector<uint8_t> batch((size_t)tb::kBytes, 0xAB);
  for (int g = 0; g < tb::kGroups; ++g)
    tb::fill_group(g, batch.data() + (size_t)g * sp8::kPkGroupBytes);
  std::vector<int> seen(lt::kEntries, 0);
  int tail = 0;
  for (int g = 0; g < tb::kGroups; ++g) {
    const uint8_t *rec = batch.data() + (size_t)g * sp8::kPkGroupBytes;
    const int item = tb::group_item(g);
    CHECK(item == (g < tb::kGroupsPerItem ? 0 : 1));
    for (int r = 0; r < tb::kRows; ++r) {
      const int e = tb::row_entry(g, r);
      const int b0 = (int8_t)rec[sp8::kPkStates + 2 * r], b1 = (int8_t)rec[sp8::kPkStates + 2 * r + 1];
      const int cnt = rec[sp8::kPkCounts + r];
      if (e < 0) {  // the tail: no state, count 0
        CHECK(cnt == 0 && b0 == 0 && b1 == 0);
        ++tail;
        continue;
      }
      CHECK(cnt == 1);
      CHECK(e >= 0 && e < lt::kEntries);
      CHECK(b0 >= -lt::kCap && b0 <= lt::kCap && b1 >= -lt::kCap && b1 <= lt::kCap);
      // the record's bins are the entry's, and the inverse finds the row
      CHECK(lt::entry(item, b0, b1) == e);
      CHECK(tb::entry_group(e) == g && tb::entry_row(e) == r);
      // states in lt::state_index order within an item
      CHECK(lt::state_index(b0, b1) == (g % tb::kGroupsPerItem) * tb::kRows + r);
      ++seen[e];
    }
    for (int q = 0; q < sp8::kPkSegs; ++q) {
      sp8::PkSeg s;
      std::memcpy(&s, rec + sp8::kPkSegRecs + q * sizeof(s), sizeof(s));
      CHECK(s.cu == -1 && s.pold == 1.0f && s.adv == 0.0f && s.step == -1);
    }
  }
  for (int e = 0; e < lt::kEntries; ++e) CHECK(seen[e] == 1);
  CHECK(tail == tb::kGroups * tb::kRows - lt::kEntries);
  // the inverse on every entry
  for (int e = 0; e < lt::kEntries; ++e)
    CHECK(tb::row_entry(tb::entry_group(e), tb::entry_row(e)) == e);
  std::printf("train table batch: ok (%d entries, %d tail rows)\n", lt::kEntries, tail);
  return 0;
}
