// Host check of spec8_e0_layout.h (tests/test_e0_layout.py): the relu-mask
// record that rollout_split_kernel writes and policy_train_spec8_e0_kernel
// reads.  The 32x32 MFMA C layout is restated here from the kernels' comments
// (lane row r = 32 t + (lane & 31); register e = 4 q + u of o-tile ot holds
// o = 32 ot + 8 q + 4 (lane >> 5) + u), not taken from the header.
#include <cstdio>
#include <set>
#include <vector>

#include "spec8_e0_layout.h"

using namespace xh::sp8;

static int c_row(int t, int lane) { return 32 * t + (lane & 31); }
static int c_out(int ot, int lane, int e) {
  return 32 * ot + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
}

int main() {
  int bad = 0;
  // (r, o) <-> (word, bit): a bijection over 64 x 128 onto 256 x 32
  std::set<int> seen;
  for (int r = 0; r < kE0Rows; ++r)
    for (int o = 0; o < kE0Outs; ++o) {
      const int w = e0_word_of(r, o), b = e0_bit_of(r, o);
      if (w < 0 || w >= kE0Words || b < 0 || b >= 32) ++bad;
      seen.insert(32 * w + b);
      // and back through the accumulator coordinates
      const int ot = w / 64, lane = w % 64, t = b / 16, e = b % 16;
      if (e0_row(t, lane) != r || e0_out(ot, lane >> 5, e) != o) ++bad;
    }
  if ((int)seen.size() != kE0Rows * kE0Outs || kE0RecordBytes != 1024) ++bad;
  std::printf("bijection: %s (%zu bits)\n", bad ? "FAILED" : "ok", seen.size());

  // the rollout lane's view: r-tile rt in turn, the row of its lane, the 64
  // outputs of its lane half (4 o-tiles x 16 registers) -> its own four words
  int bad_r = 0;
  std::vector<int> owner(kE0Words, -1);
  for (int lane = 0; lane < 64; ++lane)
    for (int rt = 0; rt < 2; ++rt)
      for (int ot = 0; ot < 4; ++ot)
        for (int e = 0; e < 16; ++e) {
          const int r = c_row(rt, lane), o = c_out(ot, lane, e);
          if (e0_word_of(r, o) != e0_word(ot, lane) || e0_bit_of(r, o) != e0_bit(rt, e))
            ++bad_r;
          int &ow = owner[e0_word(ot, lane)];
          if (ow != -1 && ow != lane) ++bad_r;  // a word has one writing lane
          ow = lane;
        }
  // each of the four stores covers 64 consecutive words (256 bytes)
  for (int ot = 0; ot < 4; ++ot)
    for (int lane = 0; lane < 64; ++lane)
      if (e0_word(ot, lane) != 64 * ot + lane) ++bad_r;
  std::printf("rollout view: %s\n", bad_r ? "FAILED" : "ok");

  // the train kernel's matrix wave m: its 32 outputs, both r-tiles -> one
  // aligned dword per lane, the wave's 64 dwords contiguous
  int bad_t = 0;
  for (int m = 0; m < 4; ++m)
    for (int lane = 0; lane < 64; ++lane) {
      std::set<int> words;
      for (int t = 0; t < 2; ++t)
        for (int e = 0; e < 16; ++e) {
          const int r = c_row(t, lane), o = c_out(m, lane, e);
          if (o < 32 * m || o >= 32 * m + 32) ++bad_t;
          words.insert(e0_word_of(r, o));
          if (e0_bit_of(r, o) != 16 * t + e) ++bad_t;
        }
      if (words.size() != 1 || *words.begin() != 64 * m + lane) ++bad_t;
    }
  std::printf("train view: %s\n", bad_t ? "FAILED" : "ok");

  // both views address the same bits: every bit written by exactly one
  // (rollout lane, rt, ot, e) and read by exactly one (wave, lane, t, e)
  std::vector<int> wr(kE0Words * 32, 0), rd(kE0Words * 32, 0);
  for (int lane = 0; lane < 64; ++lane)
    for (int t = 0; t < 2; ++t)
      for (int ot = 0; ot < 4; ++ot)
        for (int e = 0; e < 16; ++e) {
          ++wr[32 * e0_word(ot, lane) + e0_bit(t, e)];
          ++rd[32 * (64 * ot + lane) + 16 * t + e];
        }
  int bad_b = 0;
  for (int i = 0; i < kE0Words * 32; ++i)
    if (wr[i] != 1 || rd[i] != 1) ++bad_b;
  std::printf("same bits: %s\n", bad_b ? "FAILED" : "ok");
  return bad || bad_r || bad_t || bad_b;
}
