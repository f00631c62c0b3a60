// Host check of the per-row terms of the PPO update diagnostics
// (dependence_free_rl_amd/csrc/xh_diag.h, the function the sum kernel
// compiles) against a long double restatement of their definition:
//   r32     = p_new / p_old                          (one f32 quotient)
//   clipped = r32 > 1.0f + eps || r32 < 1.0f - eps   (f32 bounds)
//   surr    = min(clamp(r32) * A, r32 * A)           (f32 products)
//   logr    = log((double)p_new) - log((double)p_old)
//   logr2   = logr * logr
//   k3      = ((double)p_new / (double)p_old - 1) - logr
// Bounds.  r32: a correctly rounded f32 quotient, within 2^-24 relative of
// the exact one (plus half a subnormal step).  The branch and the clamp are
// decided on the function's own r32 against the f32 sums 1.0f +- eps.  The two
// products of floats are exact in long double, so rounding them to float once
// restates the f32 products exactly: surr must be equal.  Each double log is
// within one ulp (2^-52 relative), the difference adds 2^-53 of itself; logr2
// is one double product of the function's own logr; k3 takes a double
// quotient, a difference and another difference, each within 2^-53 relative
// of its result, on top of logr's error.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "xh_diag.h"

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

static float f32_sum(float a, float b) {
  volatile float s = a + b;
  return s;
}

// the f32 part, for any inputs without a NaN: the clip decision, the clamp
// and the surrogate, from the function's own r32
static void check_f32(const xh::DiagTerms &d, float A, float eps,
                      const char *what) {
  const float hi = f32_sum(1.0f, eps), lo = f32_sum(1.0f, -eps);
  const bool above = (long double)d.r32 > (long double)hi;
  const bool below = (long double)d.r32 < (long double)lo;
  EXPECT(d.clipped == ((above || below) ? 1.0 : 0.0), "%s: clipped %g at r %.9g",
         what, d.clipped, (double)d.r32);
  const float c = above ? hi : below ? lo : d.r32;
  const float x = (float)((long double)c * (long double)A);
  const float y = (float)((long double)d.r32 * (long double)A);
  const float m = y < x ? y : x;
  EXPECT(d.surr == (double)m || (std::isnan(d.surr) && std::isnan(m)),
         "%s: surr %.17g, want %.9g (r %.9g A %.9g)", what, d.surr, (double)m,
         (double)d.r32, (double)A);
}

// the generic comparison for finite positive p_new, p_old and finite A
static void check(float pn, float po, float A, float eps, const char *what) {
  const xh::DiagTerms d = xh::diag_terms(pn, po, A, eps);
  const long double q = (long double)pn / (long double)po;
  if (q <= (long double)FLT_MAX)
    EXPECT(fabsl((long double)d.r32 - q) <=
               ldexpl(q, -24) * (1.0L + ldexpl(1.0L, -30)) + (long double)FLT_TRUE_MIN,
           "%s: r32 %.9g, want %.21Lg", what, (double)d.r32, q);
  else
    EXPECT(std::isinf(d.r32) || d.r32 == FLT_MAX, "%s: r32 %.9g, want overflow",
           what, (double)d.r32);
  check_f32(d, A, eps, what);
  const long double ln = logl((long double)pn), lo = logl((long double)po);
  const long double lr = ln - lo;
  const long double lerr = ldexpl(fabsl(ln) + fabsl(lo), -52) +
                           ldexpl(fabsl(lr), -53) + (long double)DBL_TRUE_MIN;
  EXPECT(fabsl((long double)d.logr - lr) <= lerr, "%s: logr %.17g, want %.21Lg",
         what, d.logr, lr);
  const long double l2 = (long double)d.logr * (long double)d.logr;
  EXPECT(fabsl((long double)d.logr2 - l2) <=
             ldexpl(l2, -53) + (long double)DBL_TRUE_MIN,
         "%s: logr2 %.17g, want %.21Lg", what, d.logr2, l2);
  const long double k3 = (q - 1.0L) - lr;
  const long double kerr =
      ldexpl(fabsl(q) + fabsl(q - 1.0L) + fabsl(k3), -52) + lerr;
  EXPECT(fabsl((long double)d.k3 - k3) <= kerr, "%s: k3 %.17g, want %.21Lg",
         what, d.k3, k3);
  // k3 >= 0 in exact arithmetic: below zero only by rounding
  EXPECT((long double)d.k3 >= -kerr, "%s: k3 %.17g negative", what, d.k3);
}

int main() {
  const float inff = std::numeric_limits<float>::infinity();
  const float nanf_ = std::numeric_limits<float>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  const float epss[] = {0.2f, 0.1f, 0.3f, 0.05f};
  for (float eps : epss) {
    const float hi = f32_sum(1.0f, eps), lo = f32_sum(1.0f, -eps);
    const float advs[] = {1.0f, -1.0f, 0.37f, -2.5f, 0.0f};
    for (float A : advs) {
      {  // p_new == p_old: ratio 1, every KL term exactly 0, surr = A
        const xh::DiagTerms d = xh::diag_terms(0.3f, 0.3f, A, eps);
        EXPECT(d.r32 == 1.0f && d.clipped == 0.0 && d.logr == 0.0 &&
                   d.logr2 == 0.0 && d.k3 == 0.0 && d.surr == (double)A,
               "equal: r %.9g clipped %g logr %g k3 %g surr %g", (double)d.r32,
               d.clipped, d.logr, d.k3, d.surr);
        check(0.3f, 0.3f, A, eps, "equal");
      }
      // r32 exactly 1 + eps (p_old = 0.5: the quotient is exact), one ulp
      // either side of it; the same at 1 - eps
      const float pts[6] = {hi, std::nextafterf(hi, 2.0f), std::nextafterf(hi, 0.0f),
                            lo, std::nextafterf(lo, 2.0f), std::nextafterf(lo, 0.0f)};
      const double want[6] = {0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
      for (int k = 0; k < 6; ++k) {
        const xh::DiagTerms d = xh::diag_terms(pts[k] * 0.5f, 0.5f, A, eps);
        EXPECT(d.r32 == pts[k] && d.clipped == want[k],
               "edge %d eps %g: r %.9g (want %.9g) clipped %g (want %g)", k,
               (double)eps, (double)d.r32, (double)pts[k], d.clipped, want[k]);
        check(pts[k] * 0.5f, 0.5f, A, eps, "edge");
        // on the clipped side the surrogate is the bound times A where that is
        // the smaller product, else r A
        if (want[k] == 1.0) {
          const float b = k == 1 ? hi : lo;
          const float x = b * A, y = pts[k] * A;
          EXPECT(d.surr == (double)(y < x ? y : x), "edge %d: surr %g", k, d.surr);
        }
      }
      {  // p_new = 0: ratio 0 (clipped), logr -inf, logr2 and k3 +inf
        const xh::DiagTerms d = xh::diag_terms(0.0f, 0.25f, A, eps);
        EXPECT(d.r32 == 0.0f && d.clipped == 1.0 && d.logr == -inf &&
                   d.logr2 == inf && d.k3 == inf,
               "p_new 0: r %g clipped %g logr %g logr2 %g k3 %g", (double)d.r32,
               d.clipped, d.logr, d.logr2, d.k3);
        check_f32(d, A, eps, "p_new 0");
      }
      {  // a subnormal p_old: the f32 ratio overflows, the double terms do not
        const float sub = 5.0f * FLT_TRUE_MIN;
        const xh::DiagTerms d = xh::diag_terms(0.3f, sub, A, eps);
        EXPECT(d.r32 == inff && d.clipped == 1.0 && std::isfinite(d.logr) &&
                   std::isfinite(d.k3) && d.logr > 0.0,
               "subnormal p_old: r %g clipped %g logr %g k3 %g", (double)d.r32,
               d.clipped, d.logr, d.k3);
        check(0.3f, sub, A, eps, "subnormal p_old");
        // both subnormal: the quotient of two small integers
        check(7.0f * FLT_TRUE_MIN, sub, A, eps, "subnormal both");
        const xh::DiagTerms e = xh::diag_terms(7.0f * FLT_TRUE_MIN, sub, A, eps);
        EXPECT(e.r32 == 1.4f, "subnormal both: r %.9g", (double)e.r32);
      }
    }
    {  // A < 0 with the ratio above the range: min picks r A, not the bound
      const xh::DiagTerms d = xh::diag_terms(0.75f, 0.5f, -2.0f, eps);
      EXPECT(d.r32 == 1.5f && d.clipped == 1.0 && d.surr == -3.0,
             "A < 0 above: surr %g", d.surr);
      // ... and below the range: the bound times A
      const xh::DiagTerms e = xh::diag_terms(0.25f, 0.5f, -2.0f, eps);
      EXPECT(e.r32 == 0.5f && e.clipped == 1.0 && e.surr == (double)(lo * -2.0f),
             "A < 0 below: surr %g", e.surr);
      // A > 0 mirrors it
      const xh::DiagTerms f = xh::diag_terms(0.75f, 0.5f, 2.0f, eps);
      EXPECT(f.surr == (double)(hi * 2.0f), "A > 0 above: surr %g", f.surr);
      const xh::DiagTerms g = xh::diag_terms(0.25f, 0.5f, 2.0f, eps);
      EXPECT(g.surr == 1.0, "A > 0 below: surr %g", g.surr);
    }
    {  // NaN stays NaN in every floating term; a NaN ratio is not "clipped"
      const xh::DiagTerms a = xh::diag_terms(nanf_, 0.5f, 1.0f, eps);
      EXPECT(std::isnan(a.r32) && a.clipped == 0.0 && std::isnan(a.surr) &&
                 std::isnan(a.logr) && std::isnan(a.logr2) && std::isnan(a.k3),
             "NaN p_new: %g %g %g %g", a.surr, a.logr, a.logr2, a.k3);
      const xh::DiagTerms b = xh::diag_terms(0.5f, nanf_, 1.0f, eps);
      EXPECT(std::isnan(b.r32) && b.clipped == 0.0 && std::isnan(b.surr) &&
                 std::isnan(b.logr) && std::isnan(b.logr2) && std::isnan(b.k3),
             "NaN p_old: %g %g %g %g", b.surr, b.logr, b.logr2, b.k3);
      const xh::DiagTerms c = xh::diag_terms(0.5f, 0.5f, nanf_, eps);
      EXPECT(c.r32 == 1.0f && c.clipped == 0.0 && std::isnan(c.surr) &&
                 c.logr == 0.0 && c.k3 == 0.0,
             "NaN A: %g %g", c.surr, c.logr);
      // 0 / 0
      const xh::DiagTerms z = xh::diag_terms(0.0f, 0.0f, 1.0f, eps);
      EXPECT(std::isnan(z.r32) && std::isnan(z.logr) && std::isnan(z.k3) &&
                 std::isnan(z.surr), "0/0: %g %g", z.logr, z.k3);
    }
  }
  // a sweep of pseudo-random rows (a fixed LCG)
  unsigned long long x = 88172645463325252ull;
  auto next = [&x]() {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
  };
  for (int k = 0; k < 20000; ++k) {
    const float po = (float)std::exp(-14.0 * next());
    float pn = (float)((double)po * std::exp(2.0 * next() - 1.0));
    if (k % 7 == 0) pn = (float)((double)po * (1.0 + 1e-6 * (next() - 0.5)));
    const float A = (float)(6.0 * next() - 3.0);
    check(pn, po, A, epss[k & 3], "sweep");
  }
  if (failures) {
    std::printf("update diag terms: %d failures\n", failures);
    return 1;
  }
  std::printf("update diag terms: ok\n");
  return 0;
}
