// Host check of rollout_pack_layout.h (tests/test_rollout_pack_layout.py
// builds and runs it with contraction off): for every lane count the packed
// rollout is built with,
//  * lane -> (env, bins) is a bijection of the wave's 64 lanes onto G x 64
//    bins, and lane_of / reg_of is its inverse;
//  * the packed order of the softmax sum -- lane_tree inside the lane, then
//    the xor butterfly over the segment's lanes, which is what seg_sum<L>'s
//    DPP stages add -- gives in every lane the bits of the 64-lane order of
//    seg_sum<64> (xor 1, 2, 4, 8 inside a row of 16, then (r0 + r1) + (r2 + r3)
//    of the four row sums), over random vectors, vectors with denormals and
//    vectors with one dominant term;
//  * a tail wave's lanes are active exactly for the envs below N, whole
//    segments at a time.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rollout_pack_layout.h"

using namespace xh::rp;

static int failures = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      if (++failures <= 20) {          \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// seg_sum<64> over lane = bin, lane by lane: the four in-row xor stages, then
// the row sums of lanes 0, 16, 32, 48.
static float wave_order(const float *v) {
  float t[64], n[64];
  for (int i = 0; i < 64; ++i) t[i] = v[i];
  for (int o = 1; o < 16; o <<= 1) {
    for (int i = 0; i < 64; ++i) n[i] = t[i] + t[i ^ o];
    for (int i = 0; i < 64; ++i) t[i] = n[i];
  }
  return (t[0] + t[16]) + (t[32] + t[48]);
}

template <int L>
static void mapping() {
  using P = Pack<L>;
  static_assert(P::kG * L == kWaveLanes && P::kBpl * L == kBins, "sizes");
  std::vector<int> seen(P::kG * kBins, 0);
  for (int lane = 0; lane < kWaveLanes; ++lane) {
    const int e = P::env_of(lane), b0 = P::bin0_of(lane);
    CHECK(e >= 0 && e < P::kG, "L=%d lane %d env %d", L, lane, e);
    CHECK(b0 >= 0 && b0 + P::kBpl <= kBins, "L=%d lane %d bin0 %d", L, lane, b0);
    CHECK(lane - P::pos_of(lane) == e * L, "L=%d lane %d: segment not aligned", L, lane);
    for (int r = 0; r < P::kBpl; ++r) {
      ++seen[e * kBins + b0 + r];
      CHECK(P::lane_of(e, b0 + r) == lane && P::reg_of(b0 + r) == r,
            "L=%d lane %d reg %d: inverse", L, lane, r);
    }
  }
  for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "L=%d slot %zu seen %d", L, i, seen[i]);
  // a segment lies inside one row of 16 lanes (the DPP patterns' reach)
  for (int lane = 0; lane < kWaveLanes; ++lane)
    CHECK((lane - P::pos_of(lane)) / 16 == (lane - P::pos_of(lane) + L - 1) / 16,
          "L=%d lane %d: segment crosses a row", L, lane);
}

template <int L>
static void tails() {
  using P = Pack<L>;
  const int Ns[] = {1, 3, P::kG - 1, P::kG, P::kG + 1, 48, 300, 32768};
  for (int N : Ns) {
    if (N < 1) continue;
    const int ng = P::groups(N);
    CHECK(ng * P::kG >= N && (ng - 1) * P::kG < N, "L=%d N=%d groups %d", L, N, ng);
    std::vector<int> lanes_of_env(N, 0);
    for (int g = 0; g < ng; ++g)
      for (int lane = 0; lane < kWaveLanes; ++lane) {
        const int env = g * P::kG + P::env_of(lane);
        const bool act = P::active(g, lane, N);
        CHECK(act == (env < N), "L=%d N=%d g %d lane %d", L, N, g, lane);
        if (act) ++lanes_of_env[env];
        // whole segments: a lane is active iff its segment's first lane is
        CHECK(act == P::active(g, lane - P::pos_of(lane), N), "L=%d N=%d: split segment", L, N);
      }
    for (int e = 0; e < N; ++e) CHECK(lanes_of_env[e] == L, "L=%d N=%d env %d lanes %d", L, N, e, lanes_of_env[e]);
  }
}

template <int L>
static float packed_order(const float *v, int lane_in_seg) {
  using P = Pack<L>;
  float t[L], n[L];
  for (int l = 0; l < L; ++l) {
    float regs[P::kBpl];
    for (int r = 0; r < P::kBpl; ++r) regs[r] = v[l * P::kBpl + r];
    t[l] = lane_tree<P::kBpl>(regs);
  }
  for (int o = 1; o < L; o <<= 1) {
    for (int l = 0; l < L; ++l) n[l] = t[l] + t[l ^ o];
    for (int l = 0; l < L; ++l) t[l] = n[l];
  }
  return t[lane_in_seg];
}

template <int L>
static void sums(int count) {
  std::mt19937 gen(1234 + L);
  std::uniform_real_distribution<float> u01(0.0f, 1.0f), ulog(-40.0f, 10.0f);
  float v[64];
  for (int it = 0; it < count; ++it) {
    const int kind = it % 4;
    for (int i = 0; i < 64; ++i) {
      if (kind == 0) v[i] = u01(gen);                     // like probabilities
      if (kind == 1) v[i] = std::exp(ulog(gen));          // like exp(logit)
      if (kind == 2) v[i] = (i % 3 == 0) ? 1e-41f * u01(gen) : 1e-38f * u01(gen);  // denormals
      if (kind == 3) v[i] = 1e-6f * u01(gen);             // one dominant term, below
    }
    if (kind == 3) v[gen() % 64] = 1.0e3f * (1.0f + u01(gen));
    const float want = wave_order(v);
    for (int l = 0; l < L; ++l) {
      const float got = packed_order<L>(v, l);
      CHECK(bits(got) == bits(want), "L=%d vector %d lane %d: %a vs %a", L, it, l, got, want);
    }
  }
}

template <int L>
static void all() {
  mapping<L>();
  tails<L>();
  sums<L>(4000);
}

int main() {
  all<16>();
  all<8>();
  all<4>();
  if (failures) {
    std::printf("rollout pack layout: %d failures\n", failures);
    return 1;
  }
  std::printf("rollout pack layout: ok\n");
  return 0;
}
