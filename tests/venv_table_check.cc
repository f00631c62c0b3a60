// venv_table_check.cc -- xh_venv_table.h on the host, driven by
// tests/test_venv_table_cpu.py, which compares every printed number with
// tests/venv_table_ref.py's.  Commands on stdin, one per line:
//   I D K B cap[D] shape[K][D]
//       prints "dom E S R", then for every e < E "e k b0 .. b(D-1) back",
//       back = the entry formed again from the decoded values
//   X D K cap[D] shape[K][D] item[D] bin[D]
//       prints "ent e", e = -1 outside the domain
//   Q n count bits[count]   (f32 bit patterns, hex; n the addend count)
//       prints "max bits", and unless the maximum is 0 or not finite
//       "shift s", "q v" per addend, "sum v" and "G bits"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "xh_venv_table.h"

using namespace xh::vt;

static uint32_t shape_word(const int *it, int D) {
  uint32_t w = 0;
  for (int d = 0; d < D; ++d) w |= (uint32_t)(it[d] & 0xff) << (8 * d);
  return w;
}

int main() {
  char cmd;
  while (std::scanf(" %c", &cmd) == 1) {
    if (cmd == 'I' || cmd == 'X') {
      int D, K, B = 0, cap[4] = {0, 0, 0, 0};
      if (std::scanf("%d %d", &D, &K) != 2) return 2;
      if (cmd == 'I' && std::scanf("%d", &B) != 1) return 2;
      if (D < 1 || D > 3 || K < 1 || K > kMaxItems) return 2;
      for (int d = 0; d < D; ++d)
        if (std::scanf("%d", &cap[d]) != 1) return 2;
      uint32_t shape[kMaxItems] = {};
      for (int k = 0; k < K; ++k) {
        int it[4] = {0, 0, 0, 0};
        for (int d = 0; d < D; ++d)
          if (std::scanf("%d", &it[d]) != 1) return 2;
        shape[k] = shape_word(it, D);
      }
      const Domain m = domain(cap, D, K);
      if (cmd == 'I') {
        std::printf("dom %ld %d %ld\n", m.entries, m.states,
                    rows(m.entries, B));
        for (long e = 0; e < m.entries; ++e) {
          int k, b[4] = {0, 0, 0, 0};
          entry_decode(m, (int)e, &k, b);
          std::printf("%ld %d", e, k);
          bool ok = true;
          for (int d = 0; d < D; ++d) {
            std::printf(" %d", b[d]);
            ok &= bin_ok(b[d], m.side[d]);
          }
          // the decoded item through the lookup: the first equal shape
          const int kk = item_index(shape, K, D, shape[k]);
          const int back =
              ok && kk >= 0 ? entry(kk, m.states, state_index(m.side, D, b))
                            : -1;
          std::printf(" %d\n", back);
        }
      } else {
        int it[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        for (int d = 0; d < D; ++d)
          if (std::scanf("%d", &it[d]) != 1) return 2;
        for (int d = 0; d < D; ++d)
          if (std::scanf("%d", &b[d]) != 1) return 2;
        // bytes past D set: the lookup reads the item's D bytes only
        const uint32_t w = shape_word(it, D) | ~item_mask(D);
        const int k = item_index(shape, K, D, w);
        bool ok = k >= 0;
        for (int d = 0; d < D; ++d) ok &= bin_ok(b[d], m.side[d]);
        std::printf("ent %d\n",
                    ok ? entry(k, m.states, state_index(m.side, D, b)) : -1);
      }
    } else if (cmd == 'Q') {
      long n;
      int count;
      if (std::scanf("%ld %d", &n, &count) != 2) return 2;
      std::vector<uint32_t> bits(count);
      uint32_t mb = 0;
      for (int i = 0; i < count; ++i) {
        if (std::scanf("%" SCNx32, &bits[i]) != 1) return 2;
        const uint32_t a = bits[i] & 0x7fffffffu;
        mb = a > mb ? a : mb;
      }
      std::printf("max %08" PRIx32 "\n", mb);
      if (mb == 0 || !quant_finite(mb)) continue;
      const int s = quant_shift(n, mb);
      std::printf("shift %d\n", s);
      unsigned long long sum = 0;  // the kernels' wrapping 64-bit adds
      for (int i = 0; i < count; ++i) {
        float g;
        std::memcpy(&g, &bits[i], 4);
        const long long q = quantise(g, s);
        std::printf("q %lld\n", q);
        sum += (unsigned long long)q;
      }
      const float G = dequantise((long long)sum, s);
      uint32_t gb;
      std::memcpy(&gb, &G, 4);
      std::printf("sum %lld\nG %08" PRIx32 "\n", (long long)sum, gb);
    } else {
      return 2;
    }
  }
  std::printf("venv table check: done\n");
  return 0;
}
