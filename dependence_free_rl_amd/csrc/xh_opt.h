// xh_opt.h -- the per-parameter optimizer update shared by the optimizer
// kernels (value_kernels.hip: sgd / opt / slab_reduce_opt; clip_kernels.hip:
// clip_step), so every path to a parameter runs the same arithmetic.
#ifndef XH_OPT_H_
#define XH_OPT_H_

#include "xh_device.h"
#include "xh_kernels.h"

namespace xh {

// One parameter's update, the reference's operation order:
//   sgd_optimizer::next_parameters (nn.h:622-625): p * (1 - wd) - g * lr
//   momentum_optimizer::next_parameters (nn.h:637-651): v = rho v + g;
//     p - v * lr
//   adam_optimizer::next_parameters (nn.h:666-691): m, v moments,
//     bias-corrected by c1 = 1 - beta1^t, c2 = 1 - beta2^t;
//     p - m^ lr / (sqrt(v^) + 1e-7)
__device__ __forceinline__ void opt_update(float *p, float *m, float *v, int i,
                                           float gi, const OptStep &o) {
#pragma clang fp contract(off)
  if (o.kind == 0) {
    p[i] = p[i] * (1.0f - o.wd) - gi * o.lr;
  } else if (o.kind == 1) {
    const float vel = 0.9f * m[i] + gi;
    m[i] = vel;
    p[i] = p[i] - vel * o.lr;
  } else {
    const float m1 = m[i] * o.beta1 + gi * (1.0f - o.beta1);
    const float m2 = v[i] * o.beta2 + gi * gi * (1.0f - o.beta2);
    m[i] = m1;
    v[i] = m2;
    const float mu = m1 / o.c1, vu = m2 / o.c2;
    p[i] = p[i] - mu * o.lr / (sqrtf(vu) + 1e-7f);
  }
}

}  // namespace xh

#endif  // XH_OPT_H_
