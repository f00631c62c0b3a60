// Host check of the gradient-clipping scale (dependence_free_rl_amd/csrc/
// xh_clip.h, the function the clip-and-step kernel compiles) against a long
// double restatement of its definition:
//   norm  = sqrt(ss) * r
//   scale = (float)(norm > max_norm ? max_norm / norm : 1)
// Bounds: norm takes two double roundings (the root, the product), each
// within 2^-53 relative, so |norm - sqrtl(ss) r| <= 2^-52 sqrtl(ss) r (exact
// where r == 1 and ss is a perfect square); the branch is decided on the
// function's own double norm; scale takes a double quotient and one rounding
// to float, within one float ulp (2^-23 relative) of max_norm / norm.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "xh_clip.h"

static int failures = 0;

#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      ++failures;                                  \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                    \
      std::printf("\n");                           \
    }                                              \
  } while (0)

// the generic comparison for finite, positive ss
static void check(double ss, double r, float max_norm, const char *what) {
  const xh::ClipScale c = xh::clip_scale(ss, r, max_norm);
  const long double want = sqrtl((long double)ss) * (long double)r;
  const long double nerr = fabsl((long double)c.norm - want);
  EXPECT(nerr <= ldexpl(want, -52) + (long double)DBL_TRUE_MIN,
         "%s: norm %.17g, want %.21Lg", what, c.norm, want);
  if (c.norm > (double)max_norm) {
    const long double q = (long double)max_norm / (long double)c.norm;
    EXPECT(fabsl((long double)c.scale - q) <= ldexpl(q, -23),
           "%s: scale %.9g, want %.21Lg", what, (double)c.scale, q);
    EXPECT(c.scale <= 1.0f, "%s: scale %.9g above 1", what, (double)c.scale);
  } else {
    EXPECT(c.scale == 1.0f, "%s: scale %.9g, not clipped", what,
           (double)c.scale);
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {  // ss = 0: norm 0, scale 1
    const xh::ClipScale c = xh::clip_scale(0.0, 1.0, 1.0f);
    EXPECT(c.norm == 0.0 && c.scale == 1.0f, "zero: %g %g", c.norm,
           (double)c.scale);
  }
  {  // a subnormal ss: a tiny positive norm, below every float max_norm
    const double sub = std::numeric_limits<double>::denorm_min();
    const xh::ClipScale c = xh::clip_scale(sub, 1.0, FLT_TRUE_MIN);
    EXPECT(c.norm > 0.0 && c.norm == std::sqrt(sub) && c.scale == 1.0f,
           "subnormal: %g %g", c.norm, (double)c.scale);
    check(sub, 1.0, 1.0f, "subnormal");
    check(sub * 1024, 0.5, 1.0f, "subnormal r");
  }
  {  // ss = inf: norm inf, scale 0
    const xh::ClipScale c = xh::clip_scale(inf, 1.0, 3.0f);
    EXPECT(c.norm == inf && c.scale == 0.0f, "inf: %g %g", c.norm,
           (double)c.scale);
    const xh::ClipScale d = xh::clip_scale(inf, 1.0 / 512, FLT_MAX);
    EXPECT(d.norm == inf && d.scale == 0.0f, "inf r: %g %g", d.norm,
           (double)d.scale);
  }
  {  // ss = NaN: the comparison is false, scale 1, the NaN stays in norm
    const xh::ClipScale c = xh::clip_scale(nan, 1.0, 3.0f);
    EXPECT(std::isnan(c.norm) && c.scale == 1.0f, "nan: %g %g", c.norm,
           (double)c.scale);
  }
  const float maxes[] = {3.0f, 0.1f, 1e-3f, 0.5f, 123.456f, 1e20f};
  for (float mx : maxes) {
    const double m = (double)mx;
    // norm exactly max_norm: m has 24 significant bits, so m * m is exact in
    // double and its root is m again -> not clipped
    {
      const xh::ClipScale c = xh::clip_scale(m * m, 1.0, mx);
      EXPECT(c.norm == m && c.scale == 1.0f, "equal %g: norm %.17g scale %.9g",
             m, c.norm, (double)c.scale);
    }
    // one ulp above through r: sqrt(1) * r = r
    const double up = std::nextafter(m, inf);
    {
      const xh::ClipScale c = xh::clip_scale(1.0, up, mx);
      EXPECT(c.norm == up, "ulp above (r) %g: norm %.17g", m, c.norm);
      const float want = (float)(m / up);
      EXPECT(c.scale == want && c.scale <= 1.0f,
             "ulp above (r) %g: scale %.9g want %.9g", m, (double)c.scale,
             (double)want);
      check(1.0, up, mx, "ulp above (r)");
    }
    // one ulp above with r = 1: an ss whose double root is `up`
    {
      double ss = up * up;
      bool found = false;
      for (int k = 0; k < 8 && !found; ++k) {
        if (std::sqrt(ss) == up) found = true;
        else ss = std::nextafter(ss, std::sqrt(ss) < up ? inf : 0.0);
      }
      EXPECT(found, "no ss with root one ulp above %g", m);
      if (found) {
        const xh::ClipScale c = xh::clip_scale(ss, 1.0, mx);
        EXPECT(c.norm == up && c.scale == (float)(m / up) && c.scale <= 1.0f,
               "ulp above %g: norm %.17g scale %.9g", m, c.norm,
               (double)c.scale);
      }
    }
    // one ulp below: not clipped
    {
      const xh::ClipScale c = xh::clip_scale(1.0, std::nextafter(m, 0.0), mx);
      EXPECT(c.scale == 1.0f, "ulp below %g: scale %.9g", m, (double)c.scale);
    }
    // clipped to half and not clipped at twice, r = 1 and r = 1 / rows
    check(4.0 * m * m, 1.0, mx, "half");
    {
      const xh::ClipScale c = xh::clip_scale(4.0 * m * m, 1.0, mx);
      EXPECT(c.scale == 0.5f, "half %g: scale %.9g", m, (double)c.scale);
    }
    check(0.25 * m * m, 1.0, mx, "twice");
    const double r = 1.0 / (4.0 * 131072.0);
    check(4.0 * m * m / (r * r), r, mx, "half, r");
    check(0.25 * m * m / (r * r), r, mx, "twice, r");
    check(4.0 * m * m, 1.0 / 96.0, mx, "r = 1/96");
    check(4.0 * m * m * 96.0 * 96.0, 1.0 / 96.0, mx, "r = 1/96, clipped");
  }
  // a sweep of pseudo-random ss / r / max_norm (a fixed LCG)
  unsigned long long x = 88172645463325252ull;
  auto next = [&x]() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
  };
  for (int k = 0; k < 20000; ++k) {
    const double ss = std::exp(80.0 * next() - 40.0);
    const double r = (k & 1) ? 1.0 : 1.0 / (1.0 + std::floor(1e6 * next()));
    const float mx = (float)std::exp(40.0 * next() - 20.0);
    check(ss, r, mx, "sweep");
  }
  if (failures) {
    std::printf("clip scale: %d failures\n", failures);
    return 1;
  }
  std::printf("clip scale: ok\n");
  return 0;
}
