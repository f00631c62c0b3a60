// The on-policy training curve of PPO on 2-D bin packing with 64 bins
// (BASELINE config 3's shape), written against the C ABI (xylo_hip.h): the
// trainer keeps one row of statistics per iteration on the device
// (xh_trainer_set_stats), xh_trainer_iterate runs blocks of 100 iterations
// asynchronously, and one synchronising xh_trainer_get_stats per block reads
// its 100 rows.
//
//   build/compat/ppo_training_curve [iterations=1000] [workers=32768]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include <xylo_hip.h>

#define CHECK(x)                                                       \
  do {                                                                 \
    if ((x) != XH_OK) {                                                \
      std::fprintf(stderr, "%s: %s\n", #x, xh_last_error());           \
      return 1;                                                        \
    }                                                                  \
  } while (0)

namespace {

// [A(out x in) ~ N(0, sigma), b = 0] per dense layer, the flat
// model::parameters() layout (nn.h:499-508)
std::vector<float> init(std::mt19937 &gen, const std::vector<int> &w,
                        bool he) {
  std::vector<float> p;
  for (size_t l = 0; l + 1 < w.size(); ++l) {
    // he_initialize (nn.h:16-18) / normal_initialize (nn.h:12-14)
    std::normal_distribution<float> d(
        0.0f, he ? std::sqrt(2.0f / (float)w[l]) : 0.01f);
    for (int i = 0; i < w[l + 1] * w[l]; ++i) p.push_back(d(gen));
    p.insert(p.end(), (size_t)w[l + 1], 0.0f);
  }
  return p;
}

}  // namespace

int main(int argc, char **argv) {
  const int iterations = argc > 1 ? std::atoi(argv[1]) : 1000;
  const int workers = argc > 2 ? std::atoi(argv[2]) : 32768;
  constexpr int kBins = 64, kDims = 2, kSteps = 4, kBlock = 100;

  xh_ctx *ctx = nullptr;
  CHECK(xh_ctx_create(0, 0, 1, nullptr, &ctx));
  xh_config cfg;
  xh_config_default(&cfg, XH_PPO, kBins, kDims, workers, kSteps);
  cfg.policy_h1 = cfg.policy_h2 = 128;
  // SGD on the mean instead of the reference's row sum, which diverges at
  // this batch size (xh_config.lr_scale_rows)
  cfg.lr_scale_rows = 1;
  xh_trainer *t = nullptr;
  CHECK(xh_trainer_create(ctx, &cfg, &t));
  std::mt19937 gen(1);
  const std::vector<float> pp = init(gen, {2 * kDims, 128, 128, 1}, true);
  const std::vector<float> vp =
      init(gen, {kBins * 2 * kDims, cfg.value_h1, cfg.value_h2, 1}, false);
  CHECK(xh_trainer_set_params(t, XH_POLICY, pp.data(), pp.size()));
  CHECK(xh_trainer_set_params(t, XH_VALUE, vp.data(), vp.size()));

  CHECK(xh_trainer_set_stats(t, kBlock));
  std::vector<double> rows((size_t)kBlock * XH_STAT_COUNT);
  for (int done = 0; done < iterations;) {
    const int n = iterations - done < kBlock ? iterations - done : kBlock;
    CHECK(xh_trainer_iterate(t, n));  // asynchronous
    long total = 0;
    CHECK(xh_trainer_stats_count(t, &total));
    CHECK(xh_trainer_get_stats(t, total - n, n, rows.data()));  // waits
    done += n;
    // the block's curve point: sums over its rows
    double s[XH_STAT_COUNT] = {0};
    for (int r = 0; r < n; ++r)
      for (int k = 0; k < XH_STAT_COUNT; ++k)
        s[k] += rows[(size_t)r * XH_STAT_COUNT + k];
    const double rows_n = s[XH_STAT_TRANSITIONS];
    const double verr = s[XH_STAT_VERR_SUM] / rows_n,
                 mse = s[XH_STAT_VERR_SQSUM] / rows_n,
                 tmean = s[XH_STAT_TARGET_SUM] / rows_n,
                 tvar = s[XH_STAT_TARGET_SQSUM] / rows_n - tmean * tmean;
    const double *last = &rows[(size_t)(n - 1) * XH_STAT_COUNT];
    std::printf("iteration %d episodes %.0f mean_return %.3f entropy %.4f "
                "value_loss %.4g explained_variance %.3f "
                "policy_grad_norm %.4g value_grad_norm %.4g\n",
                done, s[XH_STAT_EPISODES],
                s[XH_STAT_EPLEN_SUM] / s[XH_STAT_EPISODES] - 1.0,
                s[XH_STAT_NEGLOGP_SUM] / rows_n, mse,
                1.0 - (mse - verr * verr) / tvar,
                std::sqrt(last[XH_STAT_PGRAD_SQ_FIRST]),
                std::sqrt(last[XH_STAT_VGRAD_SQ]));
  }
  CHECK(xh_trainer_destroy(t));
  CHECK(xh_ctx_destroy(ctx));
  return 0;
}
