// eval_api.cpp -- the episode evaluators of the C ABI: a trainer's policy
// (xh_trainer_evaluate) and the packing heuristics (xh_heuristic_evaluate)
// played over whole episodes by one kernel launch each.
#include <hip/hip_runtime.h>

#include "../../include/xylo_hip.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

using namespace xh::host;

namespace {

struct EvalBuffers {
  uint32_t x0;
  long max_steps;
  const int *init_items;
  double *total;
  long *steps;
  uint32_t *rng_out;
  int *final_items;
  int *trace;
  long trace_cap;
  // the fields xh::EvalArgs and xh::HeuristicArgs share
  template <class Args>
  void fill(Args &a, const xh_eval *e) const {
    a.n_envs = e->n_envs;
    a.episodes = e->episodes;
    a.x0 = x0;
    a.stream_stride = kEvalStride;
    a.max_steps = max_steps;
    a.init_items = init_items;
    a.total = total;
    a.steps = steps;
    a.rng_out = rng_out;
    a.final_items = final_items;
    a.trace = trace;
    a.trace_cap = trace_cap;
  }
};

// Shared host side of the episode evaluators (xh_trainer_evaluate,
// xh_heuristic_evaluate): one device scratch block for the per-env outputs,
// the launch bracketed by HIP events (e->elapsed_ms), copies back, sync.
template <class Launch>
int eval_common(xh_ctx *ctx, const xh::EnvDesc &env, int G, xh_eval *e,
                Launch launch) {
  const int n = e->n_envs, D = env.D;
  if (n <= 0 || n % G || e->episodes < 0 || e->trace_cap < 0)
    return fail(XH_ERR_INVALID, "evaluate: n_envs %d (multiple of %d), "
                "episodes %d", n, G, e->episodes);
  if (e->init_items)
    for (long i = 0; i < (long)n * D; ++i)
      if (e->init_items[i] != env.item_a[i % D] &&
          e->init_items[i] != env.item_b[i % D])
        return fail(XH_ERR_INVALID, "evaluate: init_items[%ld] = %d is not "
                    "an item of the table", i, e->init_items[i]);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_steps = up(sizeof(double) * n),
               o_rng = o_steps + up(8 * (size_t)n),
               o_init = o_rng + up(4 * (size_t)n),
               o_fin = o_init + up(4 * (size_t)n * D),
               o_trace = o_fin + up(4 * (size_t)n * D),
               bytes = o_trace + up(4 * (size_t)(e->trace ? e->trace_cap : 0));
  // a plain device allocation, each region on its own 256-byte boundary
  // (the stream-ordered allocator returned trace bytes that read back wrong
  // for some sizes on ROCm 7.2: measured at trace_cap 2049 and 10000)
  char *scratch = nullptr;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMalloc((void **)&scratch, bytes));
  EvalBuffers eb{};
  const uint32_t x0 = e->rng_state % 2147483647u;
  eb.x0 = x0 ? x0 : 1u;
  // an episode lasts at most B * capacity * D + 1 steps (every step puts at
  // least one unit into some bin)
  eb.max_steps = (long)(e->episodes + 1) * (env.B * 8 * D + 2);
  eb.total = (double *)scratch;
  eb.steps = (long *)(scratch + o_steps);
  eb.rng_out = (uint32_t *)(scratch + o_rng);
  eb.final_items = (int *)(scratch + o_fin);
  eb.trace = e->trace ? (int *)(scratch + o_trace) : nullptr;
  eb.trace_cap = e->trace ? e->trace_cap : 0;
  int st = XH_OK;
  if (e->init_items) {
    eb.init_items = (const int *)(scratch + o_init);
    st = copy_ok(copy_to_device(scratch + o_init, e->init_items,
                                4 * (size_t)n * D, s));
  }
  // from here on a failure is recorded in `st` and the scratch block, the
  // events and the stream are still released / drained below
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  auto hip_ok = [&](hipError_t e, const char *what) {
    if (st == XH_OK && e != hipSuccess)
      st = fail(XH_ERR_HIP, "evaluate %s: %s", what, hipGetErrorString(e));
    return st == XH_OK;
  };
  if (st == XH_OK && hip_ok(hipEventCreate(&ev0), "event") &&
      hip_ok(hipEventCreate(&ev1), "event") &&
      hip_ok(hipEventRecord(ev0, s), "event record")) {
    if (hip_ok(launch(eb), "launch")) hip_ok(hipEventRecord(ev1, s), "event record");
  }
  auto out = [&](void *host, size_t off, size_t nb) {
    if (st == XH_OK && host)
      st = copy_ok(copy_to_host(host, scratch + off, nb, s));
  };
  out(e->totals, 0, sizeof(double) * n);
  out(e->steps, o_steps, 8 * (size_t)n);
  out(e->rng_out, o_rng, 4 * (size_t)n);
  out(e->final_items, o_fin, 4 * (size_t)n * D);
  out(e->trace, o_trace, 4 * (size_t)eb.trace_cap);
  (void)hipStreamSynchronize(s);
  (void)hipFree(scratch);
  hip_ok(hipStreamSynchronize(s), "synchronize");
  float ms = 0.0f;
  if (st == XH_OK && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess)
    e->elapsed_ms = ms;
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  return st;
}

}  // namespace

extern "C" {

int xh_trainer_evaluate(xh_trainer *t, xh_eval *e) {
  return guard([&]() -> int {
    if (!t || !e) return fail(XH_ERR_INVALID, "null trainer / eval");
    const int G = t->cfg.bins <= 64 ? 64 / t->cfg.bins : 0;
    if (G == 0)
      return fail(XH_ERR_INVALID, "evaluate: bins %d > 64 not supported",
                  t->cfg.bins);
    return eval_common(t->ctx, t->env, G, e, [&](const EvalBuffers &eb) {
      xh::EvalArgs a{};
      a.env = t->env;
      a.params = t->pp;
      a.argmax_probs = e->argmax_probs ? 1 : 0;
      eb.fill(a, e);
      return xh::launch_eval_argmax(a, t->cfg.policy_h1, t->cfg.policy_h2,
                                    t->ctx->stream);
    });
  });
}

int xh_heuristic_evaluate(xh_ctx *ctx, int policy, int bins, int dims,
                          xh_eval *e) {
  return guard([&]() -> int {
    if (!ctx || !e) return fail(XH_ERR_INVALID, "null ctx / eval");
    if (policy < XH_HEUR_RANDOM || policy > XH_HEUR_MINWASTE)
      return fail(XH_ERR_INVALID, "heuristic policy %d", policy);
    if (!xh::heuristic_shape_supported(bins, dims))
      return fail(XH_ERR_INVALID, "heuristic: bins %d dims %d not supported",
                  bins, dims);
    const xh::EnvDesc env = make_env(bins, dims);
    return eval_common(ctx, env, 64 / bins, e, [&](const EvalBuffers &eb) {
      xh::HeuristicArgs a{};
      a.env = env;
      eb.fill(a, e);
      return xh::launch_heuristic(a, policy, ctx->stream);
    });
  });
}

}  // extern "C"
