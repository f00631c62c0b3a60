// xh_logit_table.h -- the index of the 64-bin 2-D rollout's logit table
// (policy_kernels.hip, rollout_split_kernel's table build)
// and the enumeration the table is filled by, compiled by the kernels and by
// the host check (tests/rollout_table_index_check.cc): plain C++, no HIP
// header needed on the host.
//
// The per-bin policy sees (bin state, item); every bin value the environment
// produces lies in [0, kCap], a slot the split rollout starts from holds none
// below -kCap (RolloutArgs::wide) and the item is one of the item table's two
// entries, so the logit is a function on kItems * kStates points.  A bin set
// by hand below -kCap stays where it is until an action takes it, so later
// slots can still hold one: a trainer that has seen such a slot 0 keeps the
// per-row forward (RolloutArgs::wide_seen).
#ifndef XH_LOGIT_TABLE_H_
#define XH_LOGIT_TABLE_H_

#if defined(__HIPCC__)
#define XH_LT_HD __host__ __device__
#else
#define XH_LT_HD
#endif

namespace xh {
namespace lt {

constexpr int kCap = 8;                    // the bin capacity (xh_device.h: kCapacity)
constexpr int kSide = 2 * kCap + 1;        // values of one bin dimension
constexpr int kStates = kSide * kSide;     // bin states at D = 2
constexpr int kItems = 2;                  // item_a, item_b
constexpr int kEntries = kItems * kStates; // floats of the table
constexpr int kTile = 32;                  // rows of one r-tile of the forward
// r-tiles per item; one call of the forward fills r-tile 0 for item_a and
// r-tile 1 for item_b, so this is also the number of calls
constexpr int kCalls = (kStates + kTile - 1) / kTile;

// State (b0, b1), both in [-kCap, kCap] -> 0 .. kStates - 1.
XH_LT_HD inline int state_index(int b0, int b1) {
  return (b0 + kCap) * kSide + (b1 + kCap);
}
// The table entry of a state under item 0 (item_a) or 1 (item_b).
XH_LT_HD inline int entry(int item, int b0, int b1) {
  return item * kStates + state_index(b0, b1);
}

// The enumeration: row `row` (0 .. kTile - 1) of call `call` carries state
// number call * kTile + row; numbers from kStates on (the last call's tail)
// carry no state and write no entry.
XH_LT_HD inline int enum_state(int call, int row) { return call * kTile + row; }
// state_index's inverse: the bin values of state number s < kStates.
XH_LT_HD inline void state_bins(int s, int &b0, int &b1) {
  b0 = s / kSide - kCap;
  b1 = s % kSide - kCap;
}

}  // namespace lt
}  // namespace xh

#endif  // XH_LOGIT_TABLE_H_
