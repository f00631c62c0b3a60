// xh_seg.h -- reductions over the aligned lane segments that share one row in
// the venv kernels' layout (a lane owns 16 consecutive bins, B / 16 lanes a
// row): one text for venv_act_kernel (venv_kernels.hip), which defines the f32
// softmax whose p[choice] goes into the record, and venv_policy_loss_kernel
// (venv_loss_kernels.hip), which restates that softmax bit for bit.
// seg_sum<S> (f32, the xor butterfly with partners 1, 2, 4 as DPP adds) is
// xh_device.h's; its max and integer counterparts are here.
#pragma once
#include "xh_device.h"

namespace xh {

template <int S>
__device__ __forceinline__ float seg_max(float v) {
#pragma unroll
  for (int o = 1; o < S; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
template <int S>
__device__ __forceinline__ int seg_sum_i(int v) {
#pragma unroll
  for (int o = 1; o < S; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// p_k = e_k / se of a row of logits held NB per lane by S lanes: e_k = expf(z_k
// - m), m the row's maximum; se adds the lane's e_k in bin order, then the
// row's lanes' sums by seg_sum.  All f32, one rounding per operation.
template <int S, int NB>
__device__ __forceinline__ void seg_softmax(const float (&z)[NB],
                                            float (&p)[NB]) {
#pragma clang fp contract(off)
  float m = z[0];
#pragma unroll
  for (int k = 1; k < NB; ++k) m = fmaxf(m, z[k]);
  m = seg_max<S>(m);
  float se = 0.0f;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    p[k] = expf(z[k] - m);
    se += p[k];
  }
  se = seg_sum<S>(se);
#pragma unroll
  for (int k = 0; k < NB; ++k) p[k] = p[k] / se;
}

}  // namespace xh
