// CPU check of the rollout logit table's index arithmetic
// (dependence_free_rl_amd/csrc/xh_logit_table.h, used by policy_kernels.hip's
// build_logit_table and rollout_split_kernel's table builds): state_index is
// a bijection from [-kCap, kCap]^2 onto 0 .. kStates - 1, the enumeration the
// table is filled by (enum_state / state_bins over kCalls calls of kTile
// rows) is its inverse and names every state exactly once, and every entry a
// reader or the builder can form lies inside the kEntries floats.
#include <cstdio>
#include <vector>

#include "xh_logit_table.h"

using namespace xh::lt;

static int fails = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond) && fails++ < 20)                                  \
      std::printf("FAIL %s (line %d: %d %d)\n", #cond, __LINE__, p, q); \
  } while (0)

int main() {
  static_assert(kSide == 17 && kStates == 289 && kEntries == 578, "D = 2, capacity 8");
  static_assert(kCalls * kTile >= kStates && (kCalls - 1) * kTile < kStates,
                "the calls cover the states with no empty call");
  // the index: a bijection onto 0 .. kStates - 1, its inverse state_bins
  std::vector<int> seen(kStates, 0);
  for (int p = -kCap; p <= kCap; ++p)
    for (int q = -kCap; q <= kCap; ++q) {
      const int s = state_index(p, q);
      EXPECT(s >= 0 && s < kStates);
      if (s >= 0 && s < kStates) ++seen[s];
      int b0, b1;
      state_bins(s, b0, b1);
      EXPECT(b0 == p && b1 == q);
      for (int item = 0; item < kItems; ++item) {
        const int e = entry(item, p, q);
        EXPECT(e >= 0 && e < kEntries);
        EXPECT(e == item * kStates + s);
      }
    }
  for (int p = 0, q = 0; p < kStates; ++p) EXPECT(seen[p] == 1);
  // the enumeration: every state once, nothing else written
  std::vector<int> filled(kEntries, 0);
  long rows = 0, idle = 0;
  for (int p = 0; p < kCalls; ++p)
    for (int q = 0; q < kTile; ++q, ++rows) {
      const int s = enum_state(p, q);
      EXPECT(s >= 0);
      if (s >= kStates) {
        ++idle;
        continue;
      }
      int b0, b1;
      state_bins(s, b0, b1);
      EXPECT(b0 >= -kCap && b0 <= kCap && b1 >= -kCap && b1 <= kCap);
      EXPECT(state_index(b0, b1) == s);
      for (int item = 0; item < kItems; ++item) {
        const int e = entry(item, b0, b1);
        EXPECT(e >= 0 && e < kEntries);
        if (e >= 0 && e < kEntries) ++filled[e];
      }
    }
  for (int p = 0, q = 0; p < kEntries; ++p) EXPECT(filled[p] == 1);
  std::printf("%d states, %d entries, %ld rows enumerated, %ld idle\n", kStates, kEntries,
              rows, idle);
  if (fails) return 1;
  std::printf("rollout table index: ok\n");
  return 0;
}
