// spec8_l1_layout.h -- the K slots of layer 1's single bf16 MFMA per r-tile in
// the wave-specialised config-3 train kernel (policy_spec8_kernels.hip,
// XH_SP8_L1PK), host + device so that tests/test_spec8_l1pack.py checks the
// map and both fragments on the CPU (tests/l1pack_check.cc).
//
// Layer 1 of the H1 image is pre[i][r] = sum over five inputs of row r
//
//   input 0, 1: x0, x1 (bins / 8)   2: 1   3: item is item_a   4: item is item_b
//
// times the feature's five constants S_H [W1[i][0], W1[i][1], b1[i], W1[i][2..]
// . item_a / cap, W1[i][2..] . item_b / cap], each constant as its three exact
// bf16 parts (xh_split.h, split3: part 0 = hi, 1 = mid, 2 = lo).  A 32x32x16
// MFMA has 16 K slots; the 15 (part, input) products fill them,
//
//   slot k = 5 part + input,   k = 0 .. 14;   slot 15 is zero in both operands
//
// so that one MFMA per r-tile sums what three dependent ones summed (one per
// part, 5 of 16 slots used).  The A fragment holds the matching part of the
// matching constant, the X fragment (B operand) repeats the row's five inputs
// three times.  Lane half h = lane >> 5 holds slots 8 h .. 8 h + 7 in its
// fragment elements e = 0 .. 7 (k = 8 h + e), two per 32-bit word.
#pragma once

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace xh {
namespace sp8 {

constexpr int kL1Inputs = 5, kL1Parts = 3;
constexpr int kL1Slots = kL1Inputs * kL1Parts;  // 15 of the MFMA's 16
constexpr unsigned kL1One = 0x3F80u;            // 1.0 as bf16

constexpr int l1_slot(int part, int input) { return kL1Inputs * part + input; }
constexpr bool l1_used(int k) { return k < kL1Slots; }
constexpr int l1_part(int k) { return k / kL1Inputs; }
constexpr int l1_input(int k) { return k % kL1Inputs; }
// the slot of lane half h's fragment element e
constexpr int l1_k(int h, int e) { return 8 * h + e; }

// A fragment: the bf16 bits of lane half h's element e, from the bits of the
// feature's constants by part, pb[part][input]
__host__ __device__ inline unsigned short l1_a_elem(const unsigned short (&pb)[kL1Parts][kL1Inputs],
                                                    int h, int e) {
  const int k = l1_k(h, e);
  return l1_used(k) ? pb[l1_part(k)][l1_input(k)] : (unsigned short)0;
}

// X fragment: the bf16 bits of slot k of a row whose bins are xx = x0 | x1 <<
// 16 (bf16 bits; bins / 8 are exact in bf16) and whose item is item_a (ia) or
// item_b
__host__ __device__ inline unsigned l1_x_bits(int k, unsigned xx, bool ia) {
  if (!l1_used(k)) return 0u;
  switch (l1_input(k)) {
    case 0: return xx & 0xffffu;
    case 1: return xx >> 16;
    case 2: return kL1One;
    case 3: return ia ? kL1One : 0u;
    default: return ia ? 0u : kL1One;
  }
}
// word j (elements 2 j, 2 j + 1) of lane half h's X fragment
__host__ __device__ inline unsigned l1_x_word(int h, int j, unsigned xx, bool ia) {
  return l1_x_bits(l1_k(h, 2 * j), xx, ia) | (l1_x_bits(l1_k(h, 2 * j + 1), xx, ia) << 16);
}

}  // namespace sp8
}  // namespace xh
