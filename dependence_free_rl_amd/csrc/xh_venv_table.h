// xh_venv_table.h -- the domain of a venv's logit table (xh_venv_table_*,
// include/xylo_hip.h; venv_table_kernels.hip) and the
// fixed-point quantiser of its gradient sum, compiled by the kernels, by the
// host API (venv_api.cpp) and by the host check (tests/venv_table_check.cc):
// plain C++, no HIP header needed on the host.
//
// The per-bin policy sees (bins[b][0..D), item[0..D)).  Every bin value a venv
// stores lies in [0, capacity[d]] -- the launch that takes a bin below zero
// resets the env -- and the item is one of the set's K shapes, so a per-bin
// logit is a function on E = K * prod_d (capacity[d] + 1) points:
//   side[d] = capacity[d] + 1            S = prod_d side[d]
//   s = (b0 * side[1] + b1) * side[2] + b2     (the unused dims dropped)
//   e = k * S + s, k the FIRST shape of the set equal to the item
// The table is laid out as R = ceil(E / B) observation rows of B per-bin rows
// each, so a per-bin network evaluates it as R rows; the tail from E on is
// padding (zero observations, no entry).
#ifndef XH_VENV_TABLE_H_
#define XH_VENV_TABLE_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define XH_VT_HD __host__ __device__
#else
#define XH_VT_HD
#endif

#define XH_VTAB_MAX_ENTRIES 16384

namespace xh {
namespace vt {

constexpr int kMaxItems = 16;  // XH_ITEMS_MAX

// The domain of one item set at D dims.  E is a long: 16 items at capacity 64
// in three dims are 4.4 M points, far past the limit but inside the type.
struct Domain {
  int D, K;
  int side[4];   // capacity[d] + 1; 1 past D
  int states;    // S
  long entries;  // E = K * S
};

XH_VT_HD inline Domain domain(const int *capacity, int D, int K) {
  Domain m{};
  m.D = D;
  m.K = K;
  long s = 1;
  for (int d = 0; d < 4; ++d) {
    m.side[d] = d < D ? capacity[d] + 1 : 1;
    s *= m.side[d];
  }
  m.states = (int)s;
  m.entries = (long)K * s;
  return m;
}

// padded observation rows: R = ceil(E / B)
XH_VT_HD inline long rows(long entries, int B) { return (entries + B - 1) / B; }

// bin value v of dim d is inside the domain
XH_VT_HD inline bool bin_ok(int v, int side) { return v >= 0 && v < side; }

// s of D bin values that passed bin_ok
XH_VT_HD inline int state_index(const int *side, int D, const int *b) {
  int s = b[0];
  for (int d = 1; d < D; ++d) s = s * side[d] + b[d];
  return s;
}

// the bytes of an ITEMS word that carry a shape at D dims
XH_VT_HD inline uint32_t item_mask(int D) {
  return D >= 4 ? 0xffffffffu : (1u << (8 * D)) - 1u;
}

// k: the first of the K shape words equal to the item word (its D bytes), or
// -1 where the item is none of them.  16 compares whatever K is.
XH_VT_HD inline int item_index(const uint32_t *shape, int K, int D,
                               uint32_t item_word) {
  const uint32_t w = item_word & item_mask(D);
  int k = -1;
  for (int i = kMaxItems - 1; i >= 0; --i)
    k = i < K && (shape[i] & item_mask(D)) == w ? i : k;
  return k;
}

XH_VT_HD inline int entry(int k, int states, int s) { return k * states + s; }

// The inverse enumeration: entry e < E -> item k and the D bin values.
XH_VT_HD inline void entry_decode(const Domain &m, int e, int *k, int *b) {
  *k = e / m.states;
  int s = e % m.states;
  for (int d = m.D - 1; d >= 0; --d) {
    b[d] = s % m.side[d];
    s /= m.side[d];
  }
}

// ------------------------------------------------------------ quantiser --
// The entry sums of xh_venv_table_grad are exact integer sums, so any grid and
// any order give the same bits.  With n addends, L the least integer with
// 2^L >= n, m = max |g| > 0 (finite) and ex the integer with 2^(ex-1) <= m <
// 2^ex:
//   s = 62 - L - ex
//   q(g) = llrint((double)g * 2^s)      the product is exact (a power of two
//                                       times a float, far inside double's
//                                       range), the rounding to nearest even
//   |q| <= 2^(62-L), so a sum of n of them stays below 2^62 in an int64
//   G = (float)((double)sum * 2^-s)     both conversions to nearest even
// Error of one entry with n_e addends: at most n_e * 2^(-s-1) from the
// roundings of q (an addend whose lowest set bit is at or above 2^-s rounds
// to itself), then the two final roundings (2^-53 and 2^-24 relative).

// L: the least integer with 2^L >= n (n >= 1)
XH_VT_HD inline int quant_log2(long n) {
  int L = 0;
  while (((long)1 << L) < n) ++L;
  return L;
}

// ex of m given as its f32 bit pattern with the sign cleared; bits != 0 and
// below 0x7f800000 (finite).  Normal: exponent field - 126; denormal: the
// highest set bit p of the mantissa gives m in [2^(p-149), 2^(p-148)).
XH_VT_HD inline int quant_exponent(uint32_t bits) {
  const int be = (int)(bits >> 23);
  if (be) return be - 126;
  int p = 0;
  while (bits >> (p + 1)) ++p;
  return p - 148;
}

// s, from the addend count and the maximum's bits (see quant_exponent)
XH_VT_HD inline int quant_shift(long n, uint32_t max_bits) {
  return 62 - quant_log2(n) - quant_exponent(max_bits);
}

XH_VT_HD inline bool quant_finite(uint32_t max_bits) {
  return max_bits < 0x7f800000u;
}

XH_VT_HD inline long long quantise(float g, int s) {
  return llrint(ldexp((double)g, s));
}

XH_VT_HD inline float dequantise(long long sum, int s) {
  return (float)ldexp((double)sum, -s);
}

}  // namespace vt
}  // namespace xh

#endif  // XH_VENV_TABLE_H_
