// CPU check of the compaction pass's duplicate search on lane masks
// (dependence_free_rl_amd/csrc/spec8_pack_layout.h: pk_mask_index,
// pk_dedup_first, pk_dedup; DESIGN.md §3.0e, "the duplicate search").
//
// A wave's 64 lanes hold one bin state each.  The kernels OR each lane's bit
// into the word of its state in a table of kPkMaskWords words, read the word
// back (m), take one ballot of the first occurrences (F) and derive slot,
// count, first and d from (m, F, lane).  Here the table is an array, the ORs
// run in a shuffled lane order (a bitwise OR ends at the same word in any
// order), and the derivation is held against a direct restatement of
// distinct64's loop (spec8_pack_kernels.hip): equal in slot, count, first and
// min(d, 17) wherever d <= 16, and agreeing on d > 16 otherwise.  The index is
// checked injective on [-8, 8]^2 and the table all zero after every vector.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "spec8_pack_layout.h"

using namespace xh::sp8;

#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #c); \
      return 1;                                          \
    }                                                    \
  } while (0)

typedef std::pair<int, int> State;

// distinct64, restated: the loop over the distinct keys in first-occurrence
// order, capped at kPkSegRows + 1
struct Loop {
  int d;
  int slot[64], count[64];
  bool first[64];
};
static Loop loop_restated(const int *key) {
  Loop r;
  r.d = 0;
  for (int l = 0; l < 64; ++l) {
    r.slot[l] = -1;
    r.count[l] = 0;
    r.first[l] = false;
  }
  unsigned long long left = ~0ull;
  while (left != 0ull && r.d <= kPkSegRows) {
    const int lead = __builtin_ctzll(left);
    unsigned long long m = 0ull;
    for (int l = 0; l < 64; ++l)
      if (key[l] == key[lead]) m |= 1ull << l;
    for (int l = 0; l < 64; ++l)
      if (key[l] == key[lead]) {
        r.slot[l] = r.d;
        r.count[l] = __builtin_popcountll(m);
        r.first[l] = l == lead;
      }
    left &= ~m;
    ++r.d;
  }
  return r;
}

static std::vector<unsigned long long> table(kPkMaskWords, 0ull);
static std::mt19937 rng(20240607u);

// one env-step through the table, as the kernels run it
static int check_vector(const std::vector<State> &st) {
  CHECK(st.size() == 64);
  int key[64], idx[64], order[64];
  std::set<State> distinct(st.begin(), st.end());
  const int dtrue = (int)distinct.size();
  for (int l = 0; l < 64; ++l) {
    CHECK(pk_in_domain(st[l].first, st[l].second));
    // the kernels' key: the int8 pair as one unsigned short
    key[l] = (st[l].first & 0xff) | ((st[l].second & 0xff) << 8);
    idx[l] = pk_mask_index(st[l].first, st[l].second);
    CHECK(idx[l] >= 0 && idx[l] < kPkMaskWords);
    order[l] = l;
  }
  std::shuffle(order, order + 64, rng);
  for (int o = 0; o < 64; ++o) table[idx[order[o]]] |= 1ull << order[o];
  unsigned long long m[64], F = 0ull;
  for (int l = 0; l < 64; ++l) m[l] = table[idx[l]];
  for (int l = 0; l < 64; ++l) table[idx[l]] = 0ull;
  for (int l = 0; l < 64; ++l)
    if (pk_dedup_first(m[l], l)) F |= 1ull << l;
  const Loop ref = loop_restated(key);
  for (int l = 0; l < 64; ++l) {
    const PkDedup r = pk_dedup(m[l], F, l);
    CHECK(r.d == dtrue);
    CHECK(r.first == pk_dedup_first(m[l], l));
    if (dtrue <= kPkSegRows) {
      CHECK(ref.d == dtrue && std::min(r.d, kPkSegRows + 1) == ref.d);
      CHECK(r.slot == ref.slot[l]);
      CHECK(r.count == ref.count[l]);
      CHECK(r.first == ref.first[l]);
    } else {
      CHECK(ref.d == kPkSegRows + 1);  // both say wide
      CHECK(r.d > kPkSegRows);
      // the lanes the capped loop reached agree as well
      if (ref.slot[l] >= 0) {
        CHECK(r.slot == ref.slot[l]);
        CHECK(r.count == ref.count[l]);
        CHECK(r.first == ref.first[l]);
      }
    }
  }
  for (int e = 0; e < kPkMaskWords; ++e) CHECK(table[e] == 0ull);
  return 0;
}

// 64 lanes over d distinct states drawn from `pool`, every state used, in a
// random lane order
static std::vector<State> draw(std::vector<State> pool, int d) {
  std::shuffle(pool.begin(), pool.end(), rng);
  std::vector<State> v;
  for (int l = 0; l < 64; ++l) v.push_back(pool[l < d ? l : (int)(rng() % (unsigned)d)]);
  std::shuffle(v.begin(), v.end(), rng);
  return v;
}

int main() {
  // the index: injective on the domain, xh_logit_table.h's state_index
  CHECK(kPkMaskWords == 289 && kPkSide == 17);
  std::vector<int> seen(kPkMaskWords, 0);
  std::vector<State> legal;
  for (int a = -kPkCap; a <= kPkCap; ++a)
    for (int b = -kPkCap; b <= kPkCap; ++b) {
      const int i = pk_mask_index(a, b);
      CHECK(i >= 0 && i < kPkMaskWords && i == (a + 8) * 17 + (b + 8));
      CHECK(++seen[i] == 1);
      CHECK(pk_in_domain(a, b));
      legal.push_back(State(a, b));
    }
  for (int a = -128; a <= 127; ++a)
    for (int b = -128; b <= 127; ++b)
      CHECK(pk_in_domain(a, b) == (a >= -8 && a <= 8 && b >= -8 && b <= 8));

  int vectors = 0;
  // all lanes equal; 64 distinct; exactly 16 and 17
  for (int rep = 0; rep < 20; ++rep)
    for (int d : {1, 2, 3, 15, 16, 17, 18, 33, 63, 64}) {
      if (check_vector(draw(legal, d))) return 1;
      ++vectors;
    }
  // every d, random
  for (int rep = 0; rep < 8; ++rep)
    for (int d = 1; d <= 64; ++d) {
      if (check_vector(draw(legal, d))) return 1;
      ++vectors;
    }
  // the environment's ten reachable states (tests/test_spec8_pack_states.py)
  const std::vector<State> reach = {{8, 8}, {4, 6}, {7, 6}, {0, 4}, {3, 4},
                                    {6, 4}, {2, 2}, {5, 2}, {1, 0}, {4, 0}};
  for (int rep = 0; rep < 50; ++rep)
    for (int d = 1; d <= 10; ++d) {
      if (check_vector(draw(reach, d))) return 1;
      ++vectors;
    }
  // a state's first occurrence in lane 63: every other lane one state; and
  // 16 / 17 distinct states with the last one in lane 63 only
  {
    std::vector<State> v(64, State(8, 8));
    v[63] = State(-8, 3);
    if (check_vector(v)) return 1;
    for (int d : {16, 17}) {
      for (int l = 0; l < 63; ++l) v[l] = legal[(l % (d - 1)) * 7];
      v[63] = legal[288];
      if (check_vector(v)) return 1;
    }
    // ascending runs: state j in lanes 4 j .. 4 j + 3 (16 states), and one
    // more in lane 63 (17)
    for (int l = 0; l < 64; ++l) v[l] = legal[(l / 4) * 18];
    if (check_vector(v)) return 1;
    v[63] = legal[1];
    if (check_vector(v)) return 1;
    // the corners of the domain
    for (int l = 0; l < 64; ++l)
      v[l] = State((l & 1) ? 8 : -8, (l & 2) ? 8 : -8);
    if (check_vector(v)) return 1;
    vectors += 6;
  }
  std::printf("pack dedup: ok (%d vectors)\n", vectors);
  return 0;
}
