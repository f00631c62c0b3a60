// xh_clip.h -- the scale of global-norm gradient clipping
// (xh_trainer_set_grad_clip, xh_clip_grad_norm), one function compiled by the
// clip-and-step kernel (clip_kernels.hip) and by the host check
// (tests/clip_scale_check.cc): plain C++, no HIP header needed on the host.
#ifndef XH_CLIP_H_
#define XH_CLIP_H_

#include <cmath>

#if defined(__HIPCC__)
#define XH_CLIP_HD __host__ __device__
#else
#define XH_CLIP_HD
#endif

namespace xh {

struct ClipScale {
  double norm;  // sqrt(ss) * r
  float scale;  // max_norm / norm where norm > max_norm, else 1
};

// ss: the sum of the squared gradient entries, in double.  r: what the
// optimizer multiplies the summed gradient by before it steps (1 / rows with
// lr_scale_rows, else exactly 1), so the norm is that of the gradient the
// step works on.  A zero or NaN norm compares false and leaves scale 1 (the
// NaN stays in `norm`); an infinite norm gives scale 0.  One square root, one
// product, one comparison, one quotient and one rounding to float: nothing a
// compiler could contract.
XH_CLIP_HD inline ClipScale clip_scale(double ss, double r, float max_norm) {
  ClipScale c;
  c.norm = sqrt(ss) * r;
  c.scale = (float)(c.norm > (double)max_norm ? (double)max_norm / c.norm : 1.0);
  return c;
}

}  // namespace xh

#endif  // XH_CLIP_H_
