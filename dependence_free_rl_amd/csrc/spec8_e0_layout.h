// spec8_e0_layout.h -- the relu-mask record that rollout_split_kernel writes
// per transition for PPO's first policy epoch (policy_train_spec8_e0_kernel,
// policy_spec8_kernels.hip with XH_SP8_E0_TU=1), host + device so that
// tests/test_e0_layout.py checks it exhaustively on the CPU
// (tests/e0_layout_check.cc).
//
// A record holds the bits M[r][o] = [A2[r][o] > 0] of one transition's layer-2
// pre-activations, 64 rows r (bins) x 128 outputs o: 256 words of 32 bits,
// 1 KB.  Both kernels hold A2 in the 32x32 MFMA C layout with the rows in the
// lanes:
//
//   r = 32 t + l31         r-tile t, lane row l31 = lane & 31
//   o = 32 ot + 8 q + 4 h + u   o-tile ot, lane half h = lane >> 5,
//                               accumulator register e = 4 q + u (0 .. 15)
//
// and the record is indexed by exactly these coordinates:
//
//   word = 64 ot + lane     (lane = 32 h + l31)
//   bit  = 16 t + e
//
// The rollout lane (one env per wave, both r-tiles in turn, all four o-tiles)
// owns words 64 ot + lane, ot = 0 .. 3: four dword stores, each coalesced over
// the wave (256 contiguous bytes).  The train kernel's matrix wave m (o-tile
// ot = m) reads word 64 m + lane: one aligned dword per lane, 256 contiguous
// bytes per wave, whose bit 16 t + e is the mask of its accumulator register
// e of r-tile t.  No lane needs another lane's bits on either side.
#pragma once

namespace xh {
namespace sp8 {

constexpr int kE0Rows = 64, kE0Outs = 128;
constexpr int kE0Words = kE0Rows * kE0Outs / 32;  // per record
constexpr int kE0RecordBytes = 4 * kE0Words;      // 1 KB
constexpr int kE0PBytes = 4 * kE0Rows;            // the record of p: 64 floats

// by accumulator position: o-tile ot, lane; r-tile t, register e
constexpr int e0_word(int ot, int lane) { return 64 * ot + lane; }
constexpr int e0_bit(int t, int e) { return 16 * t + e; }

// the accumulator position of (r, o)
constexpr int e0_rtile(int r) { return r >> 5; }
constexpr int e0_otile(int o) { return o >> 5; }
constexpr int e0_lane(int r, int o) { return 32 * ((o >> 2) & 1) + (r & 31); }
constexpr int e0_reg(int o) { return 4 * ((o >> 3) & 3) + (o & 3); }
// and back: the output of o-tile ot, lane half h, register e; the row of
// r-tile t, lane
constexpr int e0_out(int ot, int h, int e) { return 32 * ot + 8 * (e >> 2) + 4 * h + (e & 3); }
constexpr int e0_row(int t, int lane) { return 32 * t + (lane & 31); }

// by matrix coordinates
constexpr int e0_word_of(int r, int o) { return e0_word(e0_otile(o), e0_lane(r, o)); }
constexpr int e0_bit_of(int r, int o) { return e0_bit(e0_rtile(r), e0_reg(o)); }

}  // namespace sp8
}  // namespace xh
