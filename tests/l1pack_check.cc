// Host check (tests/test_spec8_l1pack.py) of
//   * spec8_l1_layout.h: the K slots of layer 1's single bf16 MFMA per r-tile
//     in policy_spec8_kernels.hip (XH_SP8_L1PK) -- the slot map, and both
//     fragments built by the helpers the kernel uses;
//   * the two-scale f16 pair split (xh_split.h, split2h_x2g), restated here on
//     doubles: a product of two f32 values is exact in double, and so is its
//     difference from an f16 value within half an f16 ulp of it.
// The 32x32x16 MFMA operand layout is restated from the kernel's comments
// (lane half h = lane >> 5 holds k = 8 h + e in fragment element e), bf16 and
// f16 rounding (to nearest even) on bit patterns / by nearbyint: the host
// compiler need not have either type.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "spec8_l1_layout.h"

using namespace xh::sp8;

static uint32_t f2u(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float u2f(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// f32 -> bf16 bits, round to nearest even (finite inputs)
static uint16_t bf16_bits(float f) {
  const uint32_t u = f2u(f);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static float bf16_val(uint16_t b) { return u2f((uint32_t)b << 16); }
// xh_split.h's split3 on bits: hi, mid, lo (the differences are exact in f32)
static void split3_bits(float x, uint16_t (&p)[3]) {
  p[0] = bf16_bits(x);
  const float r1 = x - bf16_val(p[0]);
  p[1] = bf16_bits(r1);
  const float r2 = r1 - bf16_val(p[1]);
  p[2] = bf16_bits(r2);
}
// the nearest f16 (11 significant bits, exponents from -14, subnormals with
// spacing 2^-24; |x| < 65504) of a double, round to nearest even
static double f16_round(double x) {
  if (x == 0.0) return 0.0;
  const int e = std::max(std::ilogb(x), -14);
  return std::ldexp(std::nearbyint(std::ldexp(x, 10 - e)), e - 10);
}

static int check_slots() {
  int bad = 0;
  bool seen[16] = {};
  for (int part = 0; part < kL1Parts; ++part)
    for (int input = 0; input < kL1Inputs; ++input) {
      const int k = l1_slot(part, input);
      if (k < 0 || k >= kL1Slots || seen[k]) {
        ++bad;
        continue;
      }
      seen[k] = true;
      if (!l1_used(k) || l1_part(k) != part || l1_input(k) != input) ++bad;
    }
  for (int k = 0; k < kL1Slots; ++k)
    if (!seen[k]) ++bad;
  if (kL1Slots != 15 || l1_used(15)) ++bad;
  // slot 15 = lane half 1's element 7: zero in both operands whatever the data
  unsigned short ones[kL1Parts][kL1Inputs];
  for (auto &row : ones)
    for (auto &v : row) v = 0x3F80;
  if (l1_a_elem(ones, 1, 7) != 0) ++bad;
  for (int ia = 0; ia < 2; ++ia) {
    if (l1_x_bits(15, 0xC000BF80u, ia != 0) != 0u) ++bad;
    if ((l1_x_word(1, 3, 0xC000BF80u, ia != 0) >> 16) != 0u) ++bad;
  }
  std::printf("slots: %s (15 (part, input) pairs, slot 15 zero)\n", bad ? "FAILED" : "ok");
  return bad;
}

// the per-half view: element e of lane half h is slot 8 h + e, elements 2 j
// and 2 j + 1 share word j (low / high half)
static int check_halves() {
  int bad = 0;
  unsigned short pb[kL1Parts][kL1Inputs];
  for (int p = 0; p < kL1Parts; ++p)
    for (int i = 0; i < kL1Inputs; ++i) pb[p][i] = (unsigned short)(0x100 * (p + 1) + i + 1);
  const unsigned xx = 0xBFC03E80u;  // x0 = 0.25, x1 = -1.5
  for (int h = 0; h < 2; ++h)
    for (int e = 0; e < 8; ++e) {
      const int k = 8 * h + e;  // the MFMA's K index of this element
      if (l1_k(h, e) != k) ++bad;
      const unsigned short want_a = k < 15 ? pb[k / 5][k % 5] : 0;
      if (l1_a_elem(pb, h, e) != want_a) ++bad;
      for (int ia = 0; ia < 2; ++ia) {
        const unsigned in[5] = {xx & 0xffffu, xx >> 16, 0x3F80u, ia ? 0x3F80u : 0u,
                                ia ? 0u : 0x3F80u};
        const unsigned want_x = k < 15 ? in[k % 5] : 0u;
        const unsigned w = l1_x_word(h, e >> 1, xx, ia != 0);
        if (((e & 1) ? w >> 16 : w & 0xffffu) != want_x) ++bad;
      }
    }
  std::printf("halves: %s (k = 8 h + e)\n", bad ? "FAILED" : "ok");
  return bad;
}

// sum_k A[k] B[k] over the fragments against sum_parts part . input, in
// double; the lists of products compared as sorted lists too (no order of
// summation enters)
static int check_fragments() {
  int bad = 0;
  long cases = 0;
  std::mt19937 rng(20240607);
  std::uniform_real_distribution<float> mant(1.0f, 2.0f);
  std::uniform_int_distribution<int> expo(-30, 30), kind(0, 9);
  for (int rep = 0; rep < 400; ++rep) {
    // a W1 row's five constants: wide exponents, negatives, zeros
    float cst[kL1Inputs];
    for (float &c : cst) {
      const int kd = kind(rng);
      c = kd == 0 ? 0.0f : std::ldexp(mant(rng), expo(rng)) * (kd & 1 ? -1.0f : 1.0f);
    }
    if (rep == 0)
      for (float &c : cst) c = 0.0f;
    unsigned short pb[kL1Parts][kL1Inputs];
    double part_val[kL1Parts][kL1Inputs];
    for (int i = 0; i < kL1Inputs; ++i) {
      uint16_t p[3];
      split3_bits(cst[i], p);
      for (int q = 0; q < kL1Parts; ++q) {
        pb[q][i] = p[q];
        part_val[q][i] = (double)bf16_val(p[q]);
      }
    }
    for (int ia = 0; ia < 2; ++ia)
      for (int b0 = -16; b0 <= 16; ++b0)
        for (int b1 = -16; b1 <= 16; b1 += (rep < 8 ? 1 : 7)) {
          const float x0 = (float)b0 / 8.0f, x1 = (float)b1 / 8.0f;
          if (bf16_val(bf16_bits(x0)) != x0 || bf16_val(bf16_bits(x1)) != x1) ++bad;
          const unsigned xx = (unsigned)bf16_bits(x0) | ((unsigned)bf16_bits(x1) << 16);
          const double in[kL1Inputs] = {x0, x1, 1.0, ia ? 1.0 : 0.0, ia ? 0.0 : 1.0};
          double ref = 0.0, got = 0.0;
          std::vector<double> pr, pg;
          for (int q = 0; q < kL1Parts; ++q)
            for (int i = 0; i < kL1Inputs; ++i) {
              const double t = part_val[q][i] * in[i];
              ref += t;
              if (t != 0.0) pr.push_back(t);
            }
          for (int h = 0; h < 2; ++h)
            for (int e = 0; e < 8; ++e) {
              const double av = (double)bf16_val(l1_a_elem(pb, h, e));
              const unsigned w = l1_x_word(h, e >> 1, xx, ia != 0);
              const double bv = (double)bf16_val((uint16_t)((e & 1) ? w >> 16 : w & 0xffffu));
              const double t = av * bv;
              got += t;
              if (t != 0.0) pg.push_back(t);
            }
          std::sort(pr.begin(), pr.end());
          std::sort(pg.begin(), pg.end());
          if (got != ref || pr != pg) ++bad;
          ++cases;
        }
  }
  std::printf("fragments: %s (%ld rows)\n", bad ? "FAILED" : "ok", cases);
  return bad;
}

// the two-scale pair split: hi = f16(h g), the exact product rounded once; lo
// = f16(h g - hi), the exact difference rounded once.  That v_fma_mixlo /
// mixhi_f16 round the exact fused result ONCE to f16 (and not first to f32)
// is ASSUMED here, from the instruction's description; this host check
// states what the split computes under that assumption and cannot verify the
// hardware's rounding (restated on doubles, where product and difference are
// exact, because the host compiler has no _Float16; fmaf followed by a
// conversion would itself round twice).  The form it replaces: x = f32(h g),
// hi = f16(x), lo = f16(x - hi).
static int check_split() {
  int bad = 0;
  long n = 0, bound_cases = 0, hi_moved = 0, closer = 0, farther = 0;
  double worst_new = 0.0, worst_old = 0.0;
  std::mt19937 rng(977);
  std::uniform_real_distribution<float> mant(1.0f, 2.0f);
  std::uniform_int_distribution<int> eh(-20, 6), ep(-24, 13), sg(0, 1);
  for (int it = 0; it < 400000; ++it) {
    // h >= 0 (a relu output, or exactly zero), g of either sign, |h g| < 2^14
    const int e_h = eh(rng), e_p = ep(rng);
    const float h = it % 97 == 0 ? 0.0f : std::ldexp(mant(rng), e_h);
    float g = std::ldexp(mant(rng), e_p - e_h - 1) * (sg(rng) ? -1.0f : 1.0f);
    if (it % 89 == 0) g = 0.0f;
    const double P = (double)h * (double)g;  // exact: 24 x 24 bits
    // new form
    const double hi = f16_round(P), lo = f16_round(P - hi);
    // old form
    const float x = h * g;
    const double hi_o = f16_round((double)x), lo_o = f16_round((double)x - hi_o);
    // (the differences are exact in double)
    if ((P - hi) + hi != P || ((double)x - hi_o) + hi_o != (double)x) ++bad;
    const double tol = std::ldexp(std::fabs(P), -22);
    const double err = std::fabs((hi + lo) - P), err_o = std::fabs((hi_o + lo_o) - P);
    if (err_o <= tol) {
      ++bound_cases;
      if (err > tol) ++bad;
      if (P != 0.0) {
        worst_new = std::max(worst_new, err / std::fabs(P));
        worst_old = std::max(worst_old, err_o / std::fabs(P));
      }
    }
    // hi is the once-rounded exact product: no f16 lies closer to P, and on
    // a tie its last bit is even
    const int e = std::max(std::ilogb(hi == 0.0 ? P : hi), -14);
    const double ulp = std::ldexp(1.0, e - 10);
    if (std::fabs(hi - P) > 0.5 * ulp) ++bad;
    if (std::fabs(hi - P) == 0.5 * ulp && std::fmod(hi / ulp, 2.0) != 0.0) ++bad;
    if (hi != hi_o) ++hi_moved;
    if (err < err_o) ++closer;
    if (err > err_o) ++farther;
    ++n;
  }
  std::printf("split: %s (%ld pairs, %ld where the old form holds 2^-22; worst relative error "
              "new %.3g old %.3g; hi differs from the twice-rounded one in %ld, sum closer in "
              "%ld, farther in %ld)\n",
              bad ? "FAILED" : "ok", n, bound_cases, worst_new, worst_old, hi_moved, closer,
              farther);
  return bad;
}

int main() {
  const int bad = check_slots() + check_halves() + check_fragments() + check_split();
  return bad ? 1 : 0;
}
