// xh_vstore.h -- the store of a wave's block of rows in the venv kernels'
// layout (a lane owns 16 consecutive floats of a row -- all 8 at 8 bins -- and
// the wave's rows are consecutive, so its [rows][B] output is one contiguous
// block): venv_policy_loss_kernel's grad / probs_out (venv_loss_kernels.hip)
// and venv_act_kernel's distribution record (venv_kernels.hip).
// A lane's 16 floats are one 64-byte run, and stored from the lane that made
// them every instruction would touch 64 lines; exchanged through LDS the block
// goes out as whole lines, nontemporal (it is read once, later).  OWNER = true
// stores from the owning lanes instead (16-byte stores, no LDS, no barrier);
// each kernel has a -D switch that picks it for `make variant`, and both
// times are in DESIGN.md 3.2.
#pragma once
#include "xh_device.h"

namespace xh {

typedef float vl_f4 __attribute__((ext_vector_type(4)));

template <int B>
struct VLossShape {
  static constexpr int BPL = 16 < B ? 16 : B;  // bins per lane
  static constexpr int LPE = B / BPL;          // lanes per row
  static constexpr int RPW = 64 / LPE;         // rows per wave
  static constexpr int F4 = BPL / 4;           // 16-byte pieces per lane
};

// The wave's [RPW][B] block at `ob` from the lanes' f[BPL]: lane l holds the
// pieces l F4 .. l F4 + F4 - 1 of the block; instruction i stores piece 64 i +
// l from lane l.  rows_live bit l: lane l's row is stored.  stage: the wave's
// 64 F4 pieces of LDS (unused with OWNER).  Without OWNER every lane of the
// workgroup reaches the barriers.
template <int B, bool OWNER>
__device__ __forceinline__ void vloss_store(const float *f, vl_f4 *stage,
                                            int lane,
                                            unsigned long long rows_live,
                                            vl_f4 *ob) {
  constexpr int G = VLossShape<B>::F4;
  if constexpr (OWNER) {
    if ((rows_live >> lane) & 1)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const vl_f4 x = {f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]};
        ob[lane * G + g] = x;
      }
  } else {
    __syncthreads();  // the previous block's pieces have been read
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const vl_f4 x = {f[4 * g], f[4 * g + 1], f[4 * g + 2], f[4 * g + 3]};
      stage[lane * G + (g + lane) % G] = x;  // rotated: LDS banks
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int p = i * 64 + lane, lp = p / G, gg = p % G;
      if ((rows_live >> lp) & 1) {
        const vl_f4 x = stage[lp * G + (gg + lp) % G];
        __builtin_nontemporal_store(x, ob + p);
      }
    }
  }
}

}  // namespace xh
