// spec8_pack_layout.h -- the packed batch of the 64-bin 2-D [128,128] train
// epoch ("duplicate rows"): what spec8_pack_kernels.hip
// writes once per learn() and policy_spec8_kernels.hip's packed build
// (XH_SP8_PACK_TU=1) reads in every epoch.  Host + device.
//
// The per-bin policy sees one row per bin, (bin / 8, item / 8), and within an
// env-step all 64 rows share the item: a row is its bin state.  An env-step
// whose 64 bins hold at most kPkSegRows distinct states is PACKABLE: its
// distinct states, in first-occurrence order over the bins, with their
// multiplicities, fill one 16-row segment.  Four segments of env-steps with
// the same item make one 64-row group.  Any other env-step is WIDE: a group of
// its own, all 64 rows with count 1.
//
// Groups in order: item_a's packed groups, item_b's packed groups, item_a's
// wide groups, item_b's wide groups.  Within a class the env-steps keep their
// batch order (slot-major, t N + env), position p of a packed class in
// segment p % 4 of the class's group p / 4: the layout, and with it every
// float sum of the epoch, is a function of the batch alone.
//
// A group's record, kPkGroupBytes:
//   [  0, 128)  64 rows x (b0, b1) int8: row 16 q + k = state k of segment q
//   [128, 192)  64 counts (uint8): 0 = unused slot
//   [192, 256)  4 segments x PkSeg
// A wide group carries the same PkSeg four times (cu = the action).  The empty
// segments of a class's last group have counts 0 and cu = -1, pold = 1, adv =
// 0.
#ifndef XH_SPEC8_PACK_LAYOUT_H_
#define XH_SPEC8_PACK_LAYOUT_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define XH_PK_HD __host__ __device__
#else
#define XH_PK_HD
#endif

namespace xh {
namespace sp8 {

constexpr int kPkSegRows = 16, kPkSegs = 4;
constexpr int kPkGroupBytes = 256;
constexpr int kPkStates = 0, kPkCounts = 128, kPkSegRecs = 192;

struct PkSeg {
  int32_t cu;    // the chosen bin's row in the group (16 q + its slot), -1: empty
  float pold;    // p_old of the env-step
  float adv;     // its advantage
  int32_t step;  // the env-step, t N + env (-1: empty)
};
static_assert(sizeof(PkSeg) == 16 && kPkSegRecs + kPkSegs * sizeof(PkSeg) == kPkGroupBytes,
              "the group record");

// the header (device ints): env-steps per class, groups per class, all groups
enum {
  kPkNA = 0,  // packable env-steps, item_a
  kPkNB,      // packable, item_b
  kPkUA,      // wide, item_a
  kPkUB,      // wide, item_b
  kPkGA,      // packed groups of item_a = ceil(NA / 4)
  kPkGB,      // packed groups of item_b
  kPkGroups,  // GA + GB + UA + UB
  kPkHdrInts = 8
};
// env-step classes, in group order
enum { kPkClsA = 0, kPkClsB, kPkClsWideA, kPkClsWideB, kPkClasses };

// The duplicate search of the compaction pass on lane masks (DESIGN.md §3.0e,
// "the duplicate search"; spec8_pack_kernels.hip, tests/pack_dedup_check.cc).
// Every bin state the environment produces lies in [-kPkCap, kPkCap]^2:
// kPkMaskWords states, one 64-bit word each in a wave's own LDS table.  Each
// lane ORs its lane bit into its state's word; the word read back, m, is the
// set of lanes that hold the lane's state.
constexpr int kPkCap = 8, kPkSide = 2 * kPkCap + 1;
constexpr int kPkMaskWords = kPkSide * kPkSide;
// a bin value the table has a word for
XH_PK_HD inline bool pk_in_domain(int b0, int b1) {
  return (unsigned)(b0 + kPkCap) <= 2u * kPkCap && (unsigned)(b1 + kPkCap) <= 2u * kPkCap;
}
// the word of state (b0, b1), both in [-kPkCap, kPkCap] (xh_logit_table.h's
// state_index)
XH_PK_HD inline int pk_mask_index(int b0, int b1) {
  return (b0 + kPkCap) * kPkSide + (b1 + kPkCap);
}
// the lane is its state's first occurrence
XH_PK_HD inline bool pk_dedup_first(unsigned long long m, int lane) {
  return lane == __builtin_ctzll(m);
}
// From m and F = the set of lanes that are a first occurrence (one ballot):
// the state's index in first-occurrence order, its multiplicity, and the
// number of distinct states (not capped: a wide env-step is d > kPkSegRows).
struct PkDedup {
  int slot, count, d;
  bool first;
};
XH_PK_HD inline PkDedup pk_dedup(unsigned long long m, unsigned long long F, int lane) {
  const int lead = __builtin_ctzll(m);
  PkDedup r;
  r.slot = __builtin_popcountll(F & ((1ull << lead) - 1ull));
  r.count = __builtin_popcountll(m);
  r.d = __builtin_popcountll(F);
  r.first = lane == lead;
  return r;
}

// groups a batch of nt env-steps can need: all wide, or packed with both
// classes' last groups partly filled
constexpr size_t pk_max_groups(size_t nt) { return nt + 2; }
// the pass's scratch ints: counts and offsets per class and chunk of 64 env-steps
constexpr size_t pk_scratch_ints(size_t nt) { return 2 * kPkClasses * ((nt + 63) / 64); }

}  // namespace sp8
}  // namespace xh

#endif  // XH_SPEC8_PACK_LAYOUT_H_
