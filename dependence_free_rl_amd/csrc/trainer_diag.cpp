// trainer_diag.cpp -- the trainer's opt-in diagnostics with their C ABI:
// per-iteration statistics, PPO update diagnostics, global-norm gradient
// clipping's log, and launch timing / kernel info.  Their hooks in rollout()
// and learn() (stats_rollout, stats_learn, upd_learn) are declared in
// xh_trainer.h; nothing here runs while a diagnostic is off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/xylo_hip.h"
#include "spec8_pack_layout.h"
#include "spec8_table_layout.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

namespace xh {
namespace host {

// ---------------------------------------------------------- statistics ----
// xh_trainer_set_stats: one row per iteration in the device ring.  The summed
// entries of each part are contiguous in the row, so with a communicator one
// all-reduce per phase runs in place on the row between the kernels' partial
// sums and any read of it; without a communicator none is launched.
void stats_free(xh_trainer *t) {
  auto &st = t->stats;
  if (st.ring.dev) (void)hipFree(st.ring.dev);
  if (st.part) (void)hipFree(st.part);
  if (st.norms) (void)hipFree(st.norms);
  if (st.ep_len) (void)hipFree(st.ep_len);
  st = xh_trainer::stats_state{};
}

// After the rollout launches: open row `rows` with the episode part.
int stats_rollout(xh_trainer *t) {
  auto &st = t->stats;
  hipStream_t s = t->ctx->stream;
  const int N = (int)t->N(), T = (int)t->T();
  double *row = ring_row(st.ring, st.ring.rows);
  CHK(timed(t, "stats", [&]() {
    return xh::launch_episode_stats(t->done, t->pold, N, T, st.ep_len, st.part,
                                    s);
  }));
  CHK(timed(t, "stats", [&]() {
    return xh::launch_episode_row(st.part, xh::gae_grid(N),
                                  (double)st.ring.rows,
                                  (double)T * t->cfg.num_envs_global,
                                  (double)T * N, row, s);
  }));
  CHK(allreduce_d(t, row + XH_STAT_EPISODES, xh::kStatEpisodeSummed));
  ++st.ring.rows;
  st.open = true;
  return XH_OK;
}

// At the end of learn(): the learner part of the open row (none is open when
// statistics were switched on after this window's rollout).
int stats_learn(xh_trainer *t) {
  auto &st = t->stats;
  if (!st.open) return XH_OK;
  hipStream_t s = t->ctx->stream;
  const int N = (int)t->N(), T = (int)t->T();
  double *row = ring_row(st.ring, st.ring.rows - 1);
  CHK(timed(t, "stats", [&]() {
    return xh::launch_learner_stats(t->v_state0, t->targets, t->adv, N, T,
                                    st.part, s);
  }));
  CHK(timed(t, "stats", [&]() {
    return xh::launch_grad_norms(
        t->pgrads, t->pgrads + (size_t)(t->cfg.epochs - 1) * t->np, t->np,
        t->vgrad, t->nv, st.norms, s);
  }));
  CHK(timed(t, "stats", [&]() {
    return xh::launch_learner_row(
        st.part, xh::gae_grid(N), st.norms,
        t->kl_log ? t->kl_log + 3 * (size_t)(t->cfg.epochs - 1) : nullptr,
        t->clip[XH_POLICY].log, t->cfg.epochs, t->clip[XH_VALUE].log, row, s);
  }));
  CHK(allreduce_d(t, row + XH_STAT_VERR_SUM, xh::kStatLearnerSums));
  st.open = false;
  return XH_OK;
}

// ---------------------------------------------------- update diagnostics ----
// xh_trainer_set_update_diag: after the last epoch of every `every`-th
// learn(), a forward of the updated policy over the batch, its records summed
// into the next ring row; with a communicator one all-reduce on the row's
// summed entries.  Nothing here synchronises the host.
void upd_free(xh_trainer *t) {
  if (t->upd.ring.dev) (void)hipFree(t->upd.ring.dev);
  t->upd = xh_trainer::upd_state{};
}

// e0_at_entry: PPO's epoch-0 distributions (e0_p) were this window's when the
// learn() began (its own optimizer steps have cleared e0_valid since).
int upd_learn(xh_trainer *t, bool e0_at_entry) {
  auto &u = t->upd;
  const long learn = u.learns++;
  if (learn % u.every) return XH_OK;
  hipStream_t s = t->ctx->stream;
  const int N = (int)t->N(), T = (int)t->T();
  xh::DiagArgs a{};
  a.env = t->env;
  a.b = t->batch();
  a.params = t->pp;
  a.q = t->qold ? t->qold : (e0_at_entry && t->e0_p ? t->e0_p : nullptr);
  u.kl_source = t->qold ? "qold" : (a.q ? "e0_p" : nullptr);
  a.p_new = u.p_new;
  a.ent = u.ent;
  a.kl = u.kl;
  const int wide = batch_wide(t);
  double *row = ring_row(u.ring, u.ring.rows);
  CHK(timed(t, "probe", [&]() {
    return xh::launch_policy_diag(a, t->cfg.policy_h1, t->cfg.policy_h2, wide,
                                  t->rgrid, s, &u.info);
  }));
  CHK(timed(t, "probe", [&]() {
    return xh::launch_update_diag_sum(u.p_new, t->pold, t->adv, u.ent, u.kl, N,
                                      T, t->cfg.clip_eps, u.part, s);
  }));
  CHK(timed(t, "probe", [&]() {
    return xh::launch_update_diag_row(u.part, xh::gae_grid(N), (double)learn,
                                      (double)T * t->cfg.num_envs_global, row,
                                      s);
  }));
  CHK(allreduce_d(t, row + XH_UPD_LOGR_SUM, xh::kUpdSums));
  ++u.ring.rows;
  return XH_OK;
}

// ------------------------------------------------------ gradient clipping ----
void clip_free(xh_trainer *t, int which) {
  auto &c = t->clip[which];
  if (c.part) (void)hipFree(c.part);
  c = xh_trainer::clip_state{};
}

namespace {

constexpr int kMaxStatsRows = 1 << 20;      // xh_trainer_set_stats: 151 MB
constexpr int kMaxUpdRows = 1 << 20;        // xh_trainer_set_update_diag: 75 MB

// The update diagnostics are on and, for a read of what a probed learn() left
// (probed), one has run; `who` prefixes the messages.
int upd_ready(const xh_trainer *t, const char *who, bool probed) {
  if (!t->upd.ring.history)
    return fail(XH_ERR_STATE, "%s: the diagnostics are off "
                "(xh_trainer_set_update_diag)", who);
  if (probed && !t->upd.ring.rows)
    return fail(XH_ERR_STATE, "%s: no probed learn() since "
                "xh_trainer_set_update_diag", who);
  return XH_OK;
}

// Optimizer steps of net `which` in one learn(): the rows of its clip log.
int clip_log_rows(const xh_trainer *t, int which) {
  return which == XH_POLICY && t->cfg.algo != XH_PG ? t->cfg.epochs : 1;
}

// ------------------------------------------------- timing and kernel info ----
constexpr double kBf16DensePeakTflops = 2500.0;  // MI355X_MICROARCH.md
constexpr double kF32MfmaPeakTflops = 157.3;

std::string kernel_json(const xh::KernelInfo &k) {
  char buf[640];
  if (!k.name) return "{\"kernel\": null}";
  // MFMA products per f32 product of the kernel's arithmetic (equal FLOPs
  // per GEMM): bf16 / f16 run at the same dense rate (MI355X_MICROARCH.md)
  const double prod = k.math == xh::kMathSplitTrain      ? 4.0
                      : k.math == xh::kMathSplitRollout  ? 3.0
                      : k.math == xh::kMathSplitTrainF16 ||
                                k.math == xh::kMathSplitTrainF16Pair
                          ? 8.0 / 3.0
                          : 0.0;
  const bool bf16 = k.math == xh::kMathSplitTrain;  // the others: f16 pairs
  const char *math = prod == 0.0                         ? "f32_mfma"
                     : bf16                              ? "bf16_split"
                     : k.math == xh::kMathSplitRollout   ? "f16_pair"
                                                         : "f16_pair_bf16_split";
  char products[32] = "null";
  if (prod > 0) std::snprintf(products, sizeof products, "%.6g", prod);
  int n = std::snprintf(buf, sizeof buf,
                        "{\"kernel\": \"%s\", \"math\": \"%s\", "
                        "\"bf16_products_per_f32_product\": %s, "
                        "\"products_per_f32_product\": %s, \"peak_tflops\": %.6g",
                        k.name, math, bf16 ? products : "null", products,
                        prod > 0 ? kBf16DensePeakTflops / prod
                                 : kF32MfmaPeakTflops);
  if (k.math == xh::kMathSplitTrainF16Pair) {
    // dW2 on f16 pairs as well: 7 MFMA products issued per 3 f32 products.
    // The entries every report and test has read so far (math, products,
    // peak) keep the 8/3 yardstick of the f16-pair train kernels, so `frac`
    // stays comparable across them; what is issued is reported beside them.
    const double issued = 7.0 / 3.0;
    std::snprintf(buf + n, sizeof buf - n,
                  ", \"dw2_math\": \"f16_pair_per_feature_scale\", "
                  "\"issued_math\": \"f16_pair_train\", "
                  "\"issued_products_per_f32_product\": %.6g, "
                  "\"issued_peak_tflops\": %.6g",
                  issued, kBf16DensePeakTflops / issued);
  }
  return std::string(buf) + "}";
}

std::string env_json(const char *name) {
  const char *v = std::getenv(name);
  if (!v) return std::string("\"") + name + "\": null";
  std::string out = std::string("\"") + name + "\": \"";
  for (const char *p = v; *p; ++p)
    if (*p != '"' && *p != '\\' && (unsigned char)*p >= 32) out += *p;
  return out + "\"";
}

}  // namespace
}  // namespace host
}  // namespace xh

using namespace xh::host;

extern "C" {

int xh_trainer_set_stats(xh_trainer *t, int history_rows) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (t->cfg.algo == XH_PG)
      return fail(XH_ERR_INVALID, "set_stats: not for XH_PG trainers (REINFORCE "
                  "plays whole episodes: XH_BUF_LEN)");
    if (history_rows < 0 || history_rows > kMaxStatsRows)
      return fail(XH_ERR_INVALID, "set_stats: history_rows %d not in [0, %d]",
                  history_rows, kMaxStatsRows);
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));
    stats_free(t);
    if (history_rows == 0) return XH_OK;
    auto &st = t->stats;
    const size_t ring = (size_t)history_rows * XH_STAT_COUNT * 8,
                 part = (size_t)xh::gae_grid((int)t->N()) *
                        xh::kStatLearnerSums * 8;
    hipError_t e = hipMalloc((void **)&st.ring.dev, ring);
    if (e == hipSuccess) e = hipMalloc((void **)&st.part, part);
    if (e == hipSuccess) e = hipMalloc((void **)&st.norms, 3 * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&st.ep_len, t->N() * 4);
    // unwritten rows read as NaN (all-ones bytes); running lengths from zero
    if (e == hipSuccess) e = hipMemsetAsync(st.ring.dev, 0xFF, ring, s);
    if (e == hipSuccess) e = hipMemsetAsync(st.ep_len, 0, t->N() * 4, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      stats_free(t);
      return fail(XH_ERR_HIP, "set_stats(%d): %s", history_rows,
                  hipGetErrorString(e));
    }
    st.ring.history = history_rows;
    return XH_OK;
  });
}

int xh_trainer_stats_count(xh_trainer *t, long *total_rows) {
  return guard([&]() -> int {
    if (!t || !total_rows) return fail(XH_ERR_INVALID, "null arg");
    if (!t->stats.ring.history)
      return fail(XH_ERR_STATE, "stats_count: statistics are off "
                  "(xh_trainer_set_stats)");
    *total_rows = t->stats.ring.rows;
    return XH_OK;
  });
}

int xh_trainer_get_stats(xh_trainer *t, long first, int count, double *out) {
  return guard([&]() -> int {
    if (!t || (count > 0 && !out)) return fail(XH_ERR_INVALID, "null arg");
    if (!t->stats.ring.history)
      return fail(XH_ERR_STATE, "get_stats: statistics are off "
                  "(xh_trainer_set_stats)");
    return ring_read(t->stats.ring, t->ctx, first, count, out, "get_stats");
  });
}

int xh_trainer_set_update_diag(xh_trainer *t, int history_rows, int every) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (t->cfg.algo == XH_PG)
      return fail(XH_ERR_INVALID, "set_update_diag: not for XH_PG trainers "
                  "(REINFORCE has no old policy to compare with)");
    if (history_rows < 0 || history_rows > kMaxUpdRows)
      return fail(XH_ERR_INVALID, "set_update_diag: history_rows %d not in "
                  "[0, %d]", history_rows, kMaxUpdRows);
    if (history_rows > 0 && every < 1)
      return fail(XH_ERR_INVALID, "set_update_diag: every %d (>= 1)", every);
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    // launches of an earlier learn() may still write the buffers
    HIPCHK(hipStreamSynchronize(s));
    upd_free(t);
    if (history_rows == 0) return XH_OK;
    auto &u = t->upd;
    const size_t rows = t->T() * t->N();
    const size_t ring = (size_t)history_rows * XH_UPD_COUNT,
                 part = (size_t)xh::gae_grid((int)t->N()) * xh::kUpdSums;
    // doubles first (ring, partials, entropy, KL), then the f32 p_new
    const size_t bytes = (ring + part + 2 * rows) * 8 + rows * 4;
    hipError_t e = hipMalloc((void **)&u.ring.dev, bytes);
    // unwritten rows and records read as NaN (all-ones bytes)
    if (e == hipSuccess) e = hipMemsetAsync(u.ring.dev, 0xFF, bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      upd_free(t);
      return fail(XH_ERR_HIP, "set_update_diag(%d, %d): %s", history_rows, every,
                  hipGetErrorString(e));
    }
    u.part = u.ring.dev + ring;
    u.ent = u.part + part;
    u.kl = u.ent + rows;
    u.p_new = reinterpret_cast<float *>(u.kl + rows);
    u.ring.history = history_rows;
    u.every = every;
    return XH_OK;
  });
}

int xh_trainer_update_diag_count(xh_trainer *t, long *total_rows) {
  return guard([&]() -> int {
    if (!t || !total_rows) return fail(XH_ERR_INVALID, "null arg");
    CHK(upd_ready(t, "update_diag_count", false));
    *total_rows = t->upd.ring.rows;
    return XH_OK;
  });
}

int xh_trainer_get_update_diag(xh_trainer *t, long first, int count, double *out) {
  return guard([&]() -> int {
    if (!t || (count > 0 && !out)) return fail(XH_ERR_INVALID, "null arg");
    CHK(upd_ready(t, "get_update_diag", true));
    return ring_read(t->upd.ring, t->ctx, first, count, out, "get_update_diag");
  });
}

int xh_trainer_get_update_diag_rows(xh_trainer *t, float *p_new, double *entropy,
                                    double *kl, size_t n) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    const auto &u = t->upd;
    CHK(upd_ready(t, "get_update_diag_rows", true));
    const size_t rows = t->T() * t->N();
    if (n != rows)
      return fail(XH_ERR_INVALID, "get_update_diag_rows: n %zu, the batch has "
                  "%zu transitions", n, rows);
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));
    if (p_new) HIPCHK(copy_to_host(p_new, u.p_new, rows * 4, s));
    if (entropy) HIPCHK(copy_to_host(entropy, u.ent, rows * 8, s));
    if (kl) HIPCHK(copy_to_host(kl, u.kl, rows * 8, s));
    return XH_OK;
  });
}

int xh_trainer_update_diag_info(xh_trainer *t, char *buf, size_t cap) {
  return guard([&]() -> int {
    if (!t || !buf || cap == 0) return fail(XH_ERR_INVALID, "null arg");
    const auto &u = t->upd;
    CHK(upd_ready(t, "update_diag_info", false));
    auto quoted = [](const char *v) {
      return v ? "\"" + std::string(v) + "\"" : std::string("null");
    };
    const std::string js =
        "{\"kernel\": " + quoted(u.info.name) + ", \"math\": " +
        quoted(u.info.math == xh::kMathSplitRollout ? "f16_pair" : "f32_mfma") +
        ", \"kl_source\": " + quoted(u.kl_source) + ", \"history_rows\": " +
        std::to_string(u.ring.history) + ", \"every\": " +
        std::to_string(u.every) + "}";
    if (js.size() + 1 > cap)
      return fail(XH_ERR_INVALID, "update_diag_info: %zu bytes needed",
                  js.size() + 1);
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return XH_OK;
  });
}

int xh_trainer_set_grad_clip(xh_trainer *t, int which, float max_norm) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (which != XH_POLICY && which != XH_VALUE)
      return fail(XH_ERR_INVALID, "grad clip: which %d", which);
    if (which == XH_VALUE && t->cfg.algo == XH_PG)
      return fail(XH_ERR_INVALID, "grad clip: REINFORCE has no value net");
    if (!(max_norm >= 0.0f) || std::isinf(max_norm))
      return fail(XH_ERR_INVALID, "grad clip: max_norm %g (a finite norm > 0, "
                  "or 0 for off)", (double)max_norm);
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    // launches of an earlier learn() may still read the workspace
    HIPCHK(hipStreamSynchronize(s));
    auto &c = t->clip[which];
    if (max_norm == 0.0f) {
      clip_free(t, which);
      return XH_OK;
    }
    if (!c.part) {
      const size_t bytes =
          ((size_t)xh::kClipMaxParts + 2 * (size_t)clip_log_rows(t, which)) * 8;
      hipError_t e = hipMalloc((void **)&c.part, bytes);
      if (e == hipSuccess) e = hipMemsetAsync(c.part, 0, bytes, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        clip_free(t, which);
        return fail(XH_ERR_HIP, "grad clip: %s", hipGetErrorString(e));
      }
      c.log = c.part + xh::kClipMaxParts;
    }
    c.max_norm = max_norm;
    c.learned = false;
    return XH_OK;
  });
}

int xh_trainer_get_grad_clip_log(xh_trainer *t, int which, double *out,
                                 int cap_rows, int *rows) {
  return guard([&]() -> int {
    if (!t || !out || !rows) return fail(XH_ERR_INVALID, "null arg");
    if (which != XH_POLICY && which != XH_VALUE)
      return fail(XH_ERR_INVALID, "grad clip log: which %d", which);
    const auto &c = t->clip[which];
    if (!c.part)
      return fail(XH_ERR_STATE, "grad clip log: clipping is off for net %d "
                  "(xh_trainer_set_grad_clip)", which);
    if (!c.learned)
      return fail(XH_ERR_STATE, "grad clip log: no learn() since "
                  "xh_trainer_set_grad_clip");
    const int n = clip_log_rows(t, which);
    if (cap_rows < n)
      return fail(XH_ERR_INVALID, "grad clip log: room for %d rows, the log has "
                  "%d", cap_rows, n);
    HIPCHK(hipSetDevice(t->ctx->device));
    HIPCHK(copy_to_host(out, c.log, (size_t)n * 16, t->ctx->stream));
    *rows = n;
    return XH_OK;
  });
}

int xh_trainer_set_timing(xh_trainer *t, int on) {
  if (!t) return fail(XH_ERR_INVALID, "null trainer");
  if (on < 0 || on > XH_TIMING_TRAIN)
    return fail(XH_ERR_INVALID, "set_timing: mode %d (0, 1 or XH_TIMING_TRAIN)", on);
  t->timing = on;
  return XH_OK;
}

int xh_trainer_reset_timing(xh_trainer *t) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    for (auto &ev : t->events) {
      t->event_pool.push_back(ev.start);
      t->event_pool.push_back(ev.stop);
    }
    t->events.clear();
    return XH_OK;
  });
}

int xh_trainer_kernel_info(xh_trainer *t, char *buf, size_t cap) {
  return guard([&]() -> int {
    if (!t || !buf || cap == 0) return fail(XH_ERR_INVALID, "null arg");
    std::string roll = kernel_json(t->last_rollout);
    roll.insert(roll.size() - 1, std::string(", \"logit_table\": ") +
                                     (t->last_rollout.logit_table ? "true" : "false") +
                                     ", \"envs_per_wave\": " +
                                     std::to_string(t->last_rollout.envs_per_wave));
    const std::string js = "{\"rollout_step\": " + roll +
                           ", \"policy_train\": " + kernel_json(t->last_train) +
                           ", \"value\": \"" +
                           std::string(t->cfg.algo != XH_PG
                                           ? xh::value_kernel_name(value_mlp(t, 0, nullptr))
                                           : "gemm") +
                           "\", \"train_grid\": " + std::to_string(t->pslab_n) +
                           ", \"train_grid_cap\": " +
                           std::to_string(t->cfg.train_grid_cap) +
                           ", \"overrides\": {" + env_json("XH_TRAIN_KERNEL") +
                           ", " + env_json("XH_ROLLOUT_KERNEL") + ", " +
                           env_json("XH_VALUE_KERNEL") + "}}";
    if (js.size() + 1 > cap)
      return fail(XH_ERR_INVALID, "kernel_info: %zu bytes needed", js.size() + 1);
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return XH_OK;
  });
}

int xh_trainer_pack_stats(xh_trainer *t, long *packed, long *unpacked, long *groups) {
  return guard([&]() -> int {
    if (!t || !packed || !unpacked || !groups) return fail(XH_ERR_INVALID, "null arg");
    *packed = *unpacked = *groups = 0;
    if (!t->pk_hdr || !t->pk_learned) return XH_OK;
    int h[xh::sp8::kPkHdrInts];
    HIPCHK(hipMemcpyAsync(h, t->pk_hdr, sizeof(h), hipMemcpyDeviceToHost, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    *packed = (long)h[xh::sp8::kPkNA] + h[xh::sp8::kPkNB];
    *unpacked = (long)h[xh::sp8::kPkUA] + h[xh::sp8::kPkUB];
    *groups = h[xh::sp8::kPkGroups];
    return XH_OK;
  });
}

int xh_trainer_pack_read(xh_trainer *t, int *hdr, void *records, size_t cap) {
  return guard([&]() -> int {
    if (!t || !hdr) return fail(XH_ERR_INVALID, "null arg");
    if (!t->pk || !t->pk_hdr || !t->pk_learned)
      return fail(XH_ERR_STATE, "pack_read: the last learn() did not run packed");
    HIPCHK(hipMemcpyAsync(hdr, t->pk_hdr, xh::sp8::kPkHdrInts * sizeof(int),
                          hipMemcpyDeviceToHost, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    if (!records) return XH_OK;
    const size_t groups = (size_t)hdr[xh::sp8::kPkGroups];
    const size_t bytes = groups * xh::sp8::kPkGroupBytes;
    if (hdr[xh::sp8::kPkGroups] < 0 ||
        groups > xh::sp8::pk_max_groups((size_t)(t->T() * t->N())))
      return fail(XH_ERR_STATE, "pack_read: a header of %d groups", hdr[xh::sp8::kPkGroups]);
    if (bytes > cap) return fail(XH_ERR_INVALID, "pack_read: %zu bytes needed", bytes);
    HIPCHK(hipMemcpyAsync(records, t->pk, bytes, hipMemcpyDeviceToHost, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_table_stats(xh_trainer *t, int *ran, long *out_of_domain, long *groups) {
  return guard([&]() -> int {
    if (!t || !ran || !out_of_domain || !groups) return fail(XH_ERR_INVALID, "null arg");
    *ran = 0;
    *out_of_domain = *groups = 0;
    if (!t->tab_ood || !t->tab_learned) return XH_OK;
    int ood = 0;
    HIPCHK(hipMemcpyAsync(&ood, t->tab_ood, sizeof(ood), hipMemcpyDeviceToHost, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    *ran = 1;
    *out_of_domain = ood;
    *groups = xh::tb::kGroups;
    return XH_OK;
  });
}

int xh_trainer_kernel_time(xh_trainer *t, const char *name, double *ms,
                           long *launches) {
  return guard([&]() -> int {
    if (!t || !name || !ms || !launches) return fail(XH_ERR_INVALID, "null arg");
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    double total = 0;
    long n = 0;
    for (auto &ev : t->events) {
      if (ev.name != name) continue;
      float e = 0;
      HIPCHK(hipEventElapsedTime(&e, ev.start, ev.stop));
      total += e;
      ++n;
    }
    *ms = total;
    *launches = n;
    return XH_OK;
  });
}

}  // extern "C"
