// Stopping and resuming a PPO run on 2-D bin packing with 64 bins, written
// against the C ABI (xylo_hip.h): train, save the trainer's state to a file,
// destroy the trainer, restore the file into a new one and continue.  The
// continued run ends on the same parameter digest as a run that was never
// interrupted, bit for bit (every sum of rollout() and learn() is formed in a
// fixed order; xh_trainer_state_digest compares 80 bytes instead of the nets).
//
//   build/compat/ppo_resume [iterations=20] [workers=4096] [file=ppo_resume.state]
#include <cinttypes>
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

constexpr int kBins = 64, kDims = 2, kSteps = 4;

std::vector<float> init(std::mt19937 &gen, const std::vector<int> &w, bool he) {
  std::vector<float> p;
  for (size_t l = 0; l + 1 < w.size(); ++l) {
    std::normal_distribution<float> d(
        0.0f, he ? std::sqrt(2.0f / (float)w[l]) : 0.01f);
    for (int i = 0; i < w[l + 1] * w[l]; ++i) p.push_back(d(gen));
    p.insert(p.end(), (size_t)w[l + 1], 0.0f);
  }
  return p;
}

// A trainer as the run configures it.  `fresh`: seeded nets and adam on both;
// otherwise the nets stay zero and the optimizers sgd -- a restore brings
// both along.
int make(xh_ctx *ctx, int workers, bool fresh, xh_trainer **out) {
  xh_config cfg;
  xh_config_default(&cfg, XH_PPO, kBins, kDims, workers, kSteps);
  cfg.policy_h1 = cfg.policy_h2 = 128;
  cfg.lr_scale_rows = 1;  // a setting: every trainer of the run sets it itself
  cfg.rng_state = fresh ? 20241008u : 1u;
  CHECK(xh_trainer_create(ctx, &cfg, out));
  if (!fresh) return 0;
  std::mt19937 gen(1);
  const std::vector<float> pp = init(gen, {2 * kDims, 128, 128, 1}, true);
  const std::vector<float> vp =
      init(gen, {kBins * 2 * kDims, cfg.value_h1, cfg.value_h2, 1}, false);
  CHECK(xh_trainer_set_params(*out, XH_POLICY, pp.data(), pp.size()));
  CHECK(xh_trainer_set_params(*out, XH_VALUE, vp.data(), vp.size()));
  CHECK(xh_trainer_set_optimizer(*out, XH_POLICY, XH_OPT_ADAM, 3e-4f, 0, 0.9f, 0.999f));
  CHECK(xh_trainer_set_optimizer(*out, XH_VALUE, XH_OPT_ADAM, 1e-3f, 0, 0.9f, 0.999f));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const int iterations = argc > 1 ? std::atoi(argv[1]) : 20;
  const int workers = argc > 2 ? std::atoi(argv[2]) : 4096;
  const char *path = argc > 3 ? argv[3] : "ppo_resume.state";
  const int half = iterations / 2;

  xh_ctx *ctx = nullptr;
  CHECK(xh_ctx_create(0, 0, 1, nullptr, &ctx));
  uint64_t whole[XH_DIG_COUNT], resumed[XH_DIG_COUNT];

  // the run that is never interrupted
  xh_trainer *t = nullptr;
  if (make(ctx, workers, true, &t)) return 1;
  CHECK(xh_trainer_iterate(t, iterations));
  CHECK(xh_trainer_state_digest(t, whole));
  CHECK(xh_trainer_destroy(t));

  // the same run, stopped half way: its state goes to a file
  if (make(ctx, workers, true, &t)) return 1;
  CHECK(xh_trainer_iterate(t, half));
  std::vector<unsigned char> blob(xh_trainer_state_bytes(t));
  size_t n = 0;
  CHECK(xh_trainer_save_state(t, blob.data(), blob.size(), &n));
  CHECK(xh_trainer_destroy(t));
  std::FILE *f = std::fopen(path, "wb");
  if (!f || std::fwrite(blob.data(), 1, n, f) != n || std::fclose(f) != 0) {
    std::perror(path);
    return 1;
  }

  // ... and continued from the file by a trainer that knows nothing else
  std::vector<unsigned char> back(n);
  f = std::fopen(path, "rb");
  if (!f || std::fread(back.data(), 1, n, f) != n) {
    std::perror(path);
    return 1;
  }
  std::fclose(f);
  char what[4096];
  CHECK(xh_state_describe(back.data(), back.size(), what, sizeof what));
  std::printf("%s: %zu bytes\n%s\n", path, n, what);
  if (make(ctx, workers, false, &t)) return 1;
  CHECK(xh_trainer_load_state(t, back.data(), back.size(), XH_STATE_ALL));
  CHECK(xh_trainer_iterate(t, iterations - half));
  CHECK(xh_trainer_state_digest(t, resumed));
  CHECK(xh_trainer_destroy(t));
  CHECK(xh_ctx_destroy(ctx));

  bool same = true;
  for (int k = 0; k < XH_DIG_COUNT; ++k) same &= whole[k] == resumed[k];
  std::printf("policy parameters after %d iterations: uninterrupted %016" PRIx64
              ", resumed at %d %016" PRIx64 "\nvalue parameters: %016" PRIx64
              " / %016" PRIx64 "\n%s\n",
              iterations, whole[XH_DIG_POLICY_PARAMS], half,
              resumed[XH_DIG_POLICY_PARAMS], whole[XH_DIG_VALUE_PARAMS],
              resumed[XH_DIG_VALUE_PARAMS],
              same ? "every state digest is equal" : "DIGESTS DIFFER");
  return same ? 0 : 2;
}
