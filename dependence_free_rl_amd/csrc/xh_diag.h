// xh_diag.h -- the per-row terms of the PPO update diagnostics
// (xh_trainer_set_update_diag), one function compiled by the sum kernel
// (diag_kernels.hip) and by the host check (tests/update_diag_check.cc):
// plain C++, no HIP header needed on the host.
#ifndef XH_DIAG_H_
#define XH_DIAG_H_

#include <cmath>

#if defined(__HIPCC__)
#define XH_DIAG_HD __host__ __device__
#else
#define XH_DIAG_HD
#endif

namespace xh {

struct DiagTerms {
  float r32;       // p_new / p_old in f32 (rl.h:54-74)
  double clipped;  // 1 where r32 left [1 - eps, 1 + eps], else 0
  double surr;     // min(clamp(r32) * A, r32 * A): the surrogate objective
  double logr;     // log p_new - log p_old
  double logr2;    // its square
  double k3;       // (p_new / p_old - 1) - logr, in double: >= 0 up to rounding
};

// p_new: the updated policy's probability of the taken action; p_old: the
// sampling policy's (XH_BUF_POLD); A: the advantage the epochs read; eps:
// clip_eps.  The ratio, its clamp and the two products are f32 operations in
// the order of the clipped loss (1.0f + eps and 1.0f - eps rounded to f32
// first); the logs are double.  Nothing is masked: p_new == 0 gives logr =
// -inf and k3 = +inf, p_old == 0 gives r32 = inf (or NaN for 0 / 0), and a NaN
// input stays a NaN in every floating term (a NaN ratio compares false, so
// `clipped` is 0 for it).  A non-finite sum in the ring is the signal that the
// policy collapsed.
XH_DIAG_HD inline DiagTerms diag_terms(float p_new, float p_old, float A,
                                       float eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  DiagTerms d;
  const float hi = 1.0f + eps, lo = 1.0f - eps;
  const float r = p_new / p_old;
  float c = r;
  bool cl = false;
  if (r > hi) {
    c = hi;
    cl = true;
  } else if (r < lo) {
    c = lo;
    cl = true;
  }
  const float x = c * A, y = r * A;
  d.r32 = r;
  d.clipped = cl ? 1.0 : 0.0;
  d.surr = (double)(y < x ? y : x);
  d.logr = log((double)p_new) - log((double)p_old);
  d.logr2 = d.logr * d.logr;
  d.k3 = ((double)p_new / (double)p_old - 1.0) - d.logr;
  return d;
}

}  // namespace xh

#endif  // XH_DIAG_H_
