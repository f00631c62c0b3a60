// trainer_pg.cpp -- the REINFORCE trainer (XH_PG) behind xh_trainer_create /
// rollout / learn: policy_gradient_learner (policy_gradient.h:88-147) with a
// full-MLP softmax-xent policy (pg_training.cc:10-20), each env playing
// cfg.steps whole episodes per iteration.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/xylo_hip.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

namespace xh {
namespace host {
namespace {

// Upper bound of an episode's length: every non-final step puts an item into
// a bin, and a bin takes at most min_d floor(8 / smallest item extent in d)
// items before some extent would go negative.
int pg_episode_bound(const xh::EnvDesc &E) {
  int per_bin = 8;  // capacity per dim (bin_packing.h:48)
  for (int d = 0; d < E.D; ++d) {
    const int m = std::min(E.item_a[d], E.item_b[d]);
    per_bin = std::min(per_bin, 8 / m);
  }
  return E.B * per_bin + 1;
}

xh::MlpArgs pg_mlp(const xh_trainer *t, bool learn, int slot) {
  xh::MlpArgs m{};
  m.env = t->env;
  m.bins = t->bins;
  m.items = t->items;
  m.N = (int)t->N();
  m.nlayers = t->pg.nlayers;
  for (int i = 0; i < 4; ++i) m.w[i] = t->pg.w[i];
  m.params = t->pp;
  for (int i = 0; i < 3; ++i) {
    m.act[i] = t->pg.act[i];
    m.grad[i] = t->pg.grad[i];
  }
  if (learn) {
    m.list = t->pg.list;
    m.rows = t->pg.nrows;
    m.max_rows = (int)(t->T() * t->N());
  } else {
    m.slot = slot;
    m.max_rows = (int)t->N();
  }
  return m;
}

}  // namespace

int create_pg(xh_ctx *ctx, const xh_config &c, xh_trainer **out) {
  if (c.adv_normalize || c.lr_scale_rows)
    return fail(XH_ERR_INVALID, "REINFORCE: adv_normalize / lr_scale_rows are "
                "actor-critic / PPO options (REINFORCE has its own mean-return "
                "baseline, policy_gradient.h:125-147)");
  if (c.bins < 2 || c.bins > 128 || c.dims < 1 || c.dims > 3)
    return fail(XH_ERR_INVALID, "REINFORCE: bins %d (2..128), dims %d (1..3)",
                c.bins, c.dims);
  if (c.policy_h1 < 1 || c.policy_h2 < 0 || c.policy_h1 > 1024 ||
      c.policy_h2 > 1024)
    return fail(XH_ERR_INVALID, "REINFORCE: widths [%d,%d]", c.policy_h1,
                c.policy_h2);
  if (c.steps < 1 || c.steps > 64)
    return fail(XH_ERR_INVALID, "REINFORCE: episodes per env %d not in [1,64]",
                c.steps);
  if (c.num_envs < 1 || c.num_envs_global < c.num_envs || c.env_offset < 0 ||
      c.env_offset + c.num_envs > c.num_envs_global)
    return fail(XH_ERR_INVALID, "env partition offset %d + %d > global %d",
                c.env_offset, c.num_envs, c.num_envs_global);
  HIPCHK(hipSetDevice(ctx->device));
  auto *t = new xh_trainer;
  t->ctx = ctx;
  t->cfg = c;
  t->cfg.epochs = 1;
  t->cfg.rng_state = c.rng_state % 2147483647u;
  if (t->cfg.rng_state == 0) t->cfg.rng_state = 1;
  t->env = make_env(c.bins, c.dims);
  t->Tb = c.steps * pg_episode_bound(t->env);
  auto &pg = t->pg;
  pg.w[0] = c.bins * 2 * c.dims;
  pg.w[1] = c.policy_h1;
  pg.nlayers = 2;
  if (c.policy_h2 > 0) {
    pg.w[2] = c.policy_h2;
    pg.nlayers = 3;
  }
  pg.w[pg.nlayers] = c.bins;
  t->np = 0;
  for (int l = 0; l < pg.nlayers; ++l) t->np += pg.w[l + 1] * pg.w[l] + pg.w[l + 1];
  t->nv = 0;
  const size_t N = t->N(), T = t->T(), R = T * N;
  int st = XH_OK;
  auto A = [&](auto **p, size_t bytes) {
    if (st == XH_OK) st = dalloc(t, p, bytes);
  };
  A(&t->bins, (T + 1) * N * t->BD());
  A(&t->items, (T + 1) * N * 4);
  A(&t->action, T * N * 4);
  A(&t->forced, T * N * 4);
  A(&t->pold, T * N * 4);
  A(&t->done, T * N);
  A(&t->rng, N * 4);
  A(&t->pp, (size_t)t->np * 4);
  A(&t->adv, T * N * 4);
  for (int l = 0; l < pg.nlayers; ++l) {
    A(&pg.act[l], R * pg.w[l + 1] * 4);
    A(&pg.grad[l], R * pg.w[l + 1] * 4);
  }
  A(&pg.ep_done, N * 4);
  A(&pg.len, N * 4);
  A(&pg.active, 4);
  A(&pg.row_off, N * 4);
  A(&pg.list, R * 4);
  A(&pg.nrows, 4);
  A(&pg.rtg, R * 4);
  A(&pg.ep_part, N * 8);
  A(&pg.stats, 2 * 8);
  t->pslab_n = 64;
  t->pslab_stride = (t->np + 63) & ~63;
  A(&t->pslab, (size_t)t->pslab_n * t->pslab_stride * 4);
  A(&t->pgrads, (size_t)t->np * 4);
  A(&t->logits, N * c.bins * 4);
  A(&t->probs, N * c.bins * 4);
  if (st == XH_OK && hipHostMalloc((void **)&pg.host_active, 4) != hipSuccess)
    st = fail(XH_ERR_HIP, "hipHostMalloc");
  t->opt[XH_POLICY].lr = c.lr_policy;
  t->opt[XH_POLICY].wd = c.wd_policy;
  hipError_t e = hipSuccess;
  if (st == XH_OK) {
    e = xh::launch_pg_env_init(t->env, t->batch(), t->cfg.rng_state,
                               c.env_offset, kEvalStride, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) st = fail(XH_ERR_HIP, "env init: %s", hipGetErrorString(e));
  }
  t->counted = true;
  ++ctx->trainers;
  if (st != XH_OK) return fail_after(st, [&] { xh_trainer_destroy(t); });
  *out = t;
  return XH_OK;
}

// agent::play_one_episode x cfg.steps for every env (rl.h:325-354): one
// forward + one step kernel per env step, until every env has finished its
// episodes (checked every 8 steps through a pinned flag).
int do_pg_rollout(xh_trainer *t) {
  hipStream_t s = t->ctx->stream;
  const size_t N = t->N();
  auto &pg = t->pg;
  if (t->need_shift) {  // the envs' current states -> slot 0
    HIPCHK(hipMemcpyAsync(t->bins, t->bins + (size_t)pg.slot_end * N * t->BD(),
                          N * t->BD(), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t->items, t->items + (size_t)pg.slot_end * N * 4,
                          N * 4, hipMemcpyDeviceToDevice, s));
    t->need_shift = false;
  }
  CHK(timed(t, "rollout_step", [&]() {
    return xh::launch_pg_begin((int)N, pg.active, pg.ep_done, pg.len, s);
  }));
  xh::PgStepArgs a{};
  a.env = t->env;
  a.b = t->batch();
  a.episodes = t->cfg.steps;
  a.logits = pg.act[pg.nlayers - 1];
  a.forced = t->use_forced ? t->forced : nullptr;
  a.ep_done = pg.ep_done;
  a.len = pg.len;
  a.active = pg.active;
  int steps = 0;
  for (int step = 0; step < t->Tb; ++step) {
    xh::MlpArgs m = pg_mlp(t, false, step);
    CHK(timed(t, "rollout_step", [&]() { return xh::mlp_forward(m, s); }));
    a.t = step;
    CHK(timed(t, "rollout_step", [&]() { return xh::launch_pg_step(a, s); }));
    steps = step + 1;
    if (steps % 8 == 0 || steps == t->Tb) {
      HIPCHK(hipMemcpyAsync(pg.host_active, pg.active, 4,
                            hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (*pg.host_active == 0) break;
    }
  }
  if (*pg.host_active != 0)
    return fail(XH_ERR_STATE, "REINFORCE rollout: %d envs still playing after "
                "the step bound %d", *pg.host_active, t->Tb);
  pg.slot_end = steps;
  t->rolled = true;
  return XH_OK;
}

// policy_gradient_learner::learn (policy_gradient.h:95-123): rows = every
// transition in replay-buffer order, advantages = reversed rewards-to-go minus
// the mean trajectory return, one optimizer step on policy_loss.
int do_pg_learn(xh_trainer *t) {
  hipStream_t s = t->ctx->stream;
  auto &pg = t->pg;
  xh::PgLearnArgs L{};
  L.N = (int)t->N();
  L.B = t->cfg.bins;
  L.episodes = t->cfg.steps;
  L.gamma = t->cfg.gamma;
  L.len = pg.len;
  L.row_off = pg.row_off;
  L.list = pg.list;
  L.nrows = pg.nrows;
  L.done = t->done;
  L.action = t->action;
  L.rtg = pg.rtg;
  L.ep_part = pg.ep_part;
  L.stats = pg.stats;
  L.logits = pg.act[pg.nlayers - 1];
  L.dlogits = pg.grad[pg.nlayers - 1];
  L.adv_grid = t->adv;
  CHK(timed(t, "policy_train", [&]() { return xh::launch_pg_rows(L, s); }));
  CHK(timed(t, "policy_train", [&]() { return xh::launch_pg_adv(L, s); }));
  CHK(allreduce_d(t, pg.stats, 2));  // baseline over the job's trajectories
  const xh::MlpArgs m = pg_mlp(t, true, 0);
  CHK(timed(t, "policy_train", [&]() { return xh::mlp_forward(m, s); }));
  CHK(timed(t, "policy_train", [&]() {
    return xh::launch_pg_loss(L, m.max_rows, s);
  }));
  CHK(timed(t, "policy_train", [&]() {
    return xh::mlp_backward(m, t->pslab, t->pslab_stride, t->pslab_n, s);
  }));
  CHK(reduce_and_step(t, XH_POLICY, 0, t->pslab, t->pslab_n,
                      t->pslab_stride, t->np, t->pgrads, t->pp));
  t->clip[XH_POLICY].learned = t->clip[XH_POLICY].part != nullptr;
  t->need_shift = true;
  t->rolled = false;
  return XH_OK;
}

}  // namespace host
}  // namespace xh
