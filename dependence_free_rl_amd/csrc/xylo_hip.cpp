// xylo_hip.cpp -- the trainer's lifecycle and data ABI (include/xylo_hip.h).
//
// One xh_trainer owns every device buffer of the vectorised PPO / AC path and
// drives it on one HIP stream: T rollout-step kernels (do_rollout, here), then
// learn() in the reference order (trainer_learn.cpp).  This unit creates and
// destroys the trainer, moves parameters, optimizer settings, buffers and env
// states in and out, and holds the rollout / learn / forget / iterate entry
// points.  The rest of the trainer's ABI: trainer_pg.cpp (REINFORCE),
// trainer_diag.cpp (opt-in diagnostics, timing), eval_api.cpp (evaluators),
// state_api.cpp (checkpoints); the context's: ctx_api.cpp.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/xylo_hip.h"
#include "spec8_e0_layout.h"
#include "spec8_pack_layout.h"
#include "spec8_table_layout.h"
#include "table_tile_layout.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

using namespace xh::host;

namespace {

// XH_BUF_* -> the device buffer (null: this trainer has none) and its bytes
struct buffer_view {
  void *ptr;
  size_t bytes;
};
buffer_view buffer_of(const xh_trainer *t, int which) {
  const size_t N = t->N(), T = t->T();
  switch (which) {
    case XH_BUF_BINS: return {t->bins, (T + 1) * N * t->BD()};
    case XH_BUF_ITEMS: return {t->items, (T + 1) * N * 4};
    case XH_BUF_ACTION: return {t->action, T * N * 4};
    case XH_BUF_POLD: return {t->pold, T * N * 4};
    case XH_BUF_DONE: return {t->done, T * N};
    case XH_BUF_RNG: return {t->rng, N * 4};
    case XH_BUF_V_STATE: return {t->v_state, (T + 1) * N * 4};
    case XH_BUF_V_STATE0: return {t->v_state0, (T + 1) * N * 4};
    case XH_BUF_V_TERM: return {t->v_term, T * N * 4};
    case XH_BUF_TARGETS: return {t->targets, T * N * 4};
    case XH_BUF_ADV: return {t->adv, T * N * 4};
    case XH_BUF_VALUE_GRAD: return {t->vgrad, (size_t)t->nv * 4};
    case XH_BUF_POLICY_GRADS:
      return {t->pgrads, (size_t)t->cfg.epochs * t->np * 4};
    case XH_BUF_LOGITS: return {t->logits, N * t->cfg.bins * 4};
    case XH_BUF_PROBS: return {t->probs, N * t->cfg.bins * 4};
    case XH_BUF_QOLD: return {t->qold, T * N * t->cfg.bins * 4};
    case XH_BUF_KL: return {t->kl_log, (size_t)t->cfg.epochs * 12};
    case XH_BUF_LEN: return {t->pg.len, N * 4};
  }
  return {nullptr, 0};
}

// an env's item (D of 4 bytes) is one of the two item-table entries
bool table_item(const xh::EnvDesc &env, const int8_t *item) {
  bool is_a = true, is_b = true;
  for (int d = 0; d < env.D; ++d) {
    is_a &= item[d] == env.item_a[d];
    is_b &= item[d] == env.item_b[d];
  }
  return is_a || is_b;
}

// xh_trainer_get / set_env_state: a PPO-family trainer and envs it has
int check_env_range(const xh_trainer *t, int first, int count,
                    const int8_t *bins, const int8_t *items) {
  if (!t || (count && (!bins || !items)))
    return fail(XH_ERR_INVALID, "null arg");
  if (t->cfg.algo == XH_PG)
    return fail(XH_ERR_INVALID, "env state access: not for XH_PG trainers");
  if (first < 0 || count < 0 || first + count > t->cfg.num_envs)
    return fail(XH_ERR_INVALID, "envs [%d, %d) of %d", first, first + count,
                t->cfg.num_envs);
  return XH_OK;
}

// row groups one policy-train workgroup sums into its gradient slab at most
// (= BASELINE configs 3 and 5 per GPU: 131072 groups over 256 workgroups)
constexpr int kMaxTrainDepth = 512;

// items_ok[0] / bins_wide[0] from the device's slot 0 (after host writes that
// replaced part of it)
int rescan_slot0(xh_trainer *t) {
  const size_t N = t->N(), BD = t->BD();
  std::vector<int8_t> b(N * BD), it(N * 4);
  HIPCHK(copy_to_host(b.data(), t->bins, b.size(), t->ctx->stream));
  HIPCHK(copy_to_host(it.data(), t->items, it.size(), t->ctx->stream));
  HIPCHK(hipStreamSynchronize(t->ctx->stream));
  char ok = 1, wide = 0;
  for (size_t e = 0; e < N; ++e)
    if (!table_item(t->env, &it[e * 4])) ok = 0;
  for (int8_t v : b) wide |= v < -kBinCapacity;
  t->items_ok[0] = ok;
  t->bins_wide[0] = wide;
  return XH_OK;
}

// Pending xh_trainer_set_env_state writes -> slot 0 (the rollout's S_0).  The
// host vectors stay alive until the stream has consumed them (synchronised
// before the map is cleared).
int apply_env_overrides(xh_trainer *t) {
  if (t->env_override.empty()) return XH_OK;
  hipStream_t s = t->ctx->stream;
  const size_t BD = t->BD(), D = (size_t)t->cfg.dims;
  // runs of consecutive env ids (the map is ordered): one bins copy and one
  // items copy per run from host staging that lives until the single stream
  // synchronisation at the end (pageable sources)
  std::vector<std::vector<int8_t>> stage;
  auto it = t->env_override.begin();
  while (it != t->env_override.end()) {
    const size_t first = (size_t)it->first;
    std::vector<int8_t> rb, ri;
    size_t next = first;
    for (; it != t->env_override.end() && (size_t)it->first == next; ++it, ++next) {
      rb.insert(rb.end(), it->second.begin(), it->second.begin() + BD);
      int8_t item[4] = {0, 0, 0, 0};
      for (size_t d = 0; d < D; ++d) item[d] = it->second[BD + d];
      ri.insert(ri.end(), item, item + 4);
    }
    stage.push_back(std::move(rb));
    stage.push_back(std::move(ri));
    const std::vector<int8_t> &sb = stage[stage.size() - 2], &si = stage.back();
    hipError_t e = hipMemcpyAsync(t->bins + first * BD, sb.data(), sb.size(),
                                  hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(t->items + first * 4, si.data(), si.size(),
                         hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s);  // nothing in flight reads `stage` after this
      return fail(XH_ERR_HIP, "env override upload: %s", hipGetErrorString(e));
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  bool wide = false;
  for (const auto &kv : t->env_override)
    for (size_t i = 0; i < BD; ++i) wide |= kv.second[i] < -kBinCapacity;
  t->env_override.clear();
  // slot 0's flags: the overrides are whole item-table entries, but envs they
  // did not touch keep what an earlier set_buffer left -> re-read the slot
  // when either flag was off its default
  if (!t->items_ok[0] || t->bins_wide[0]) return rescan_slot0(t);
  if (wide) t->bins_wide[0] = 1;
  return XH_OK;
}

int do_rollout(xh_trainer *t) {
  if (t->cfg.algo == XH_PG) return do_pg_rollout(t);
  hipStream_t s = t->ctx->stream;
  const size_t N = t->N(), T = t->T();
  if (t->items_ok.size() != T + 1) {  // constructed envs in slot 0 only
    t->items_ok.assign(T + 1, 0);
    t->items_ok[0] = 1;
  }
  if (t->bins_wide.size() != T + 1) t->bins_wide.assign(T + 1, 0);
  // replay_buffer::forget(): open trajectories continue from slot T.  With
  // no host overrides pending the rollout launch moves slot T to slot 0
  // itself (the register-stepping kernels as they fetch; copies otherwise)
  int src_slot = -1;
  if (t->need_shift) {
    if (t->env_override.empty()) {
      src_slot = (int)T;
    } else {
      HIPCHK(hipMemcpyAsync(t->bins, t->bins + T * N * t->BD(), N * t->BD(),
                            hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(t->items, t->items + T * N * 4, N * 4,
                            hipMemcpyDeviceToDevice, s));
    }
    t->need_shift = false;
    t->items_ok[0] = t->items_ok[T];
    t->bins_wide[0] = t->bins_wide[T];
  }
  CHK(apply_env_overrides(t));  // whole item-table entries only
  xh::RolloutArgs a{};
  a.src_slot = src_slot;
  a.env = t->env;
  a.b = t->batch();
  a.jump_mul = t->jump_mul;
  a.params = t->pp;
  a.forced = t->use_forced ? t->forced : nullptr;
  a.qold_out = t->qold;  // KL-PPO only (nullptr otherwise)
  // PPO's epoch 0 reuses this window's masks and distributions
  // (where a learn() reads them: rollout_wants_e0)
  const bool e0w = t->e0_mask && rollout_wants_e0(t);
  a.e0_p = e0w ? t->e0_p : nullptr;
  a.e0_mask = e0w ? t->e0_mask : nullptr;
  t->e0_valid = false;
  // all T slots in one call (one launch where the kernel steps in registers);
  // only slot 0 can hold a wide state
  a.t = 0;
  a.nsteps = (int)T;
  // the f32 kernels for a slot 0 the split rollouts cannot take: a bin below
  // -capacity, or an item outside the item table (set_buffer; the split
  // rollouts fold the item into per-entry biases)
  a.wide = t->bins_wide[0] || !t->items_ok[0];
  if (t->bins_wide[0]) t->wide_seen = true;
  a.wide_seen = t->wide_seen;
  // diagnostics only (tests, health checks): off in the product path
  a.logits_out = t->cfg.record_last_step ? t->logits : nullptr;
  a.probs_out = t->cfg.record_last_step ? t->probs : nullptr;
  // cleared as well: a rollout without recording leaves no current logits
  t->last_step_recorded = t->cfg.record_last_step != 0;
  CHK(timed(t, "rollout_step", [&]() {
    return xh::launch_rollout_step(a, t->cfg.policy_h1, t->cfg.policy_h2,
                                   t->rgrid, s, &t->last_rollout);
  }));
  for (size_t step = 0; step < T; ++step) {
    t->items_ok[step + 1] = 1;  // items drawn from the table (get_item)
    t->bins_wide[step + 1] = 0;  // apply + reset on game over: bins >= 0
  }
  t->rolled = true;
  // valid only from the one kernel that writes both outputs for all T slots:
  // not after a wide slot 0 (the f32 kernel ran it), the f32 rollouts or
  // XH_ROLLOUT_KERNEL
  t->e0_valid = a.e0_mask && !a.wide && t->last_rollout.name &&
                std::strcmp(t->last_rollout.name, "rollout_split_kernel") == 0;
  if (t->stats.ring.history) CHK(stats_rollout(t));
  return XH_OK;
}

}  // namespace

// ================================================================= C ABI ==
extern "C" {

int xh_trainer_create(xh_ctx *ctx, const xh_config *cfg, xh_trainer **out) {
  return guard([&]() -> int {
    if (!ctx || !cfg || !out) return fail(XH_ERR_INVALID, "null arg");
    const xh_config &c = *cfg;
    if (c.algo == XH_PG) return create_pg(ctx, c, out);
    if (c.algo != XH_PPO && c.algo != XH_AC && c.algo != XH_KLPPO)
      return fail(XH_ERR_INVALID, "algo %d", c.algo);
    // KL-PPO beyond 64 bins: the 128-bin 3-D [128,128] shape's split train
    // kernel only (the f32 KL kernel is written for <= 64 bins)
    if (c.algo == XH_KLPPO && c.bins > 64 &&
        !(c.bins == 128 && c.dims == 3 && c.policy_h1 == 128 && c.policy_h2 == 128))
      return fail(XH_ERR_INVALID,
                  "KL-PPO: bins %d > 64 supported at 128 bins, 3-D, [128,128] only",
                  c.bins);
    if (!xh::policy_shape_supported(c.bins, c.dims, c.policy_h1, c.policy_h2))
      return fail(XH_ERR_INVALID,
                  "unsupported policy shape B=%d D=%d widths=[%d,%d]", c.bins,
                  c.dims, c.policy_h1, c.policy_h2);
    if (!xh::value_shape_supported(c.value_h1, c.value_h2))
      return fail(XH_ERR_INVALID, "unsupported value widths [%d,%d]",
                  c.value_h1, c.value_h2);
    const int G = c.bins <= 64 ? 64 / c.bins : 1;  // envs per 64-row group
    if (c.num_envs <= 0 || c.num_envs % G)
      return fail(XH_ERR_INVALID, "num_envs %d must be a positive multiple of %d",
                  c.num_envs, G);
    if (c.steps < 1 || c.steps > 1024)
      return fail(XH_ERR_INVALID, "steps %d not in [1,1024]", c.steps);
    if (c.epochs < 1 || c.epochs > 64)
      return fail(XH_ERR_INVALID, "epochs %d", c.epochs);
    if (c.num_envs_global < c.num_envs || c.env_offset < 0 ||
        c.env_offset + c.num_envs > c.num_envs_global)
      return fail(XH_ERR_INVALID, "env partition offset %d + %d > global %d",
                  c.env_offset, c.num_envs, c.num_envs_global);
    if (c.bins * 2 * c.dims > 768)
      return fail(XH_ERR_INVALID, "value input %d > 768", c.bins * 2 * c.dims);
    if (c.train_grid_cap < 0)
      return fail(XH_ERR_INVALID, "train_grid_cap %d < 0", c.train_grid_cap);
    HIPCHK(hipSetDevice(ctx->device));

    auto *t = new xh_trainer;
    t->ctx = ctx;
    t->cfg = c;
    t->Tb = c.steps;
    // minstd_rand0 seeding rule: s mod m, 0 -> 1
    t->cfg.rng_state = c.rng_state % 2147483647u;
    if (t->cfg.rng_state == 0) t->cfg.rng_state = 1;
    t->env = make_env(c.bins, c.dims);
    t->pl = xh::PolicyLayout{2 * c.dims, c.policy_h1, c.policy_h2};
    t->vl = xh::ValueLayout{c.bins * 2 * c.dims, c.value_h1, c.value_h2};
    t->np = t->pl.size();
    t->nv = t->vl.size();
    const size_t N = t->N(), T = t->T();
    int st = XH_OK;
    auto A = [&](auto **p, size_t bytes) {
      if (st == XH_OK) st = dalloc(t, p, bytes);
    };
    // + 64 B: the value forward's 8-byte loads may read past a row's last
    // byte (vnet_forward_kernel; the bytes meet zero weights)
    A(&t->bins, (T + 1) * N * t->BD() + 64);
    A(&t->items, (T + 1) * N * 4 + 64);
    A(&t->action, T * N * 4);
    A(&t->forced, T * N * 4);
    A(&t->pold, T * N * 4);
    A(&t->done, T * N);
    A(&t->rng, N * 4);
    A(&t->pp, (size_t)t->np * 4);
    A(&t->vp, (size_t)t->nv * 4);
    A(&t->v_state, (T + 1) * N * 4);
    // V(S_0..S_T) then V(E_t) of the terminal transitions only (end_list
    // order, n_end rows): one forward batch; v_term receives them by row
    A(&t->v_state0, (2 * T + 1) * N * 4);
    A(&t->v_term, T * N * 4);
    A(&t->end_list, T * N * 4);
    A(&t->n_end, 4);
    A(&t->n_open, 4);
    A(&t->vrows, 4);
    A(&t->end_scratch, (size_t)xh::end_list_scratch_ints((int)N) * 4);
    A(&t->targets, T * N * 4);
    A(&t->adv, T * N * 4);
    A(&t->row_g, T * N * 4);
    A(&t->vact[0], (2 * T + 1) * N * c.value_h1 * 4);
    A(&t->vact[1], (2 * T + 1) * N * c.value_h2 * 4);
    A(&t->vgr[0], T * N * c.value_h1 * 4);
    A(&t->vgr[1], T * N * c.value_h2 * 4);
    t->rgrid = xh::rollout_grid(c.bins, c.dims, c.policy_h1, c.policy_h2);
    t->pslab_n = xh::policy_train_grid(c.bins, c.dims, c.policy_h1, c.policy_h2,
                                       c.algo == XH_KLPPO);
    const int groups = (int)(T * N / (size_t)G);
    if (c.train_grid_cap > 0) {
      if (t->pslab_n > c.train_grid_cap)
        t->pslab_n = c.train_grid_cap;  // test-only depth control (xylo_hip.h)
    } else if (groups > t->pslab_n * kMaxTrainDepth) {
      // a batch beyond one GPU's BASELINE share (the 8-GPU jobs' whole
      // batches on one device): more workgroups than the one-per-CU grid, so
      // that no f32 gradient slab accumulates more than kMaxTrainDepth row
      // groups -- the depth the bench configurations run at, where the
      // tests hold the gradient error flat (tests/test_gpu_depth.py).  A
      // multiple of 8 keeps the kernels' XCD-aware work order.
      const int want = (groups + kMaxTrainDepth - 1) / kMaxTrainDepth;
      t->pslab_n = (want + 7) & ~7;
    }
    if (t->pslab_n > groups) t->pslab_n = groups;
    t->pslab_stride = (t->np + 63) & ~63;
    t->vslab_n = 256;
    const long vrows = (long)T * N;
    if (t->vslab_n > vrows) t->vslab_n = (int)vrows;
    t->vslab_stride = (t->nv + 63) & ~63;
    A(&t->pslab, (size_t)t->pslab_n * t->pslab_stride * 4);
    A(&t->vslab, (size_t)t->vslab_n * t->vslab_stride * 4);
    A(&t->vw0red, (size_t)c.value_h1 * (c.bins * c.dims + c.dims) * 4);
    A(&t->vw0frag, xh::vnet_frag_bytes(t->env));
    A(&t->pgrads, (size_t)c.epochs * t->np * 4);
    A(&t->vgrad, (size_t)t->nv * 4);
    A(&t->logits, N * c.bins * 4);
    A(&t->probs, N * c.bins * 4);
    A(&t->g_bound, 4);
    if (c.adv_normalize) {
      A(&t->adv_part, (size_t)xh::gae_grid((int)N) * 2 * 8);
      A(&t->adv_stats, 2 * 8);
    }
    if (c.algo == XH_KLPPO || c.record_distrib)
      A(&t->qold, T * N * c.bins * 4);
    {
      // epoch 0's inputs from the rollout: N T (1024 + 256) bytes (134 MB +
      // 33.5 MB at config 3), only where the e0 kernel can run
      const char *rk = std::getenv("XH_ROLLOUT_KERNEL"), *tk = std::getenv("XH_TRAIN_KERNEL");
      if (c.algo == XH_PPO && c.epochs >= 2 && c.bins == 64 && c.dims == 2 &&
          c.policy_h1 == 128 && c.policy_h2 == 128 && !(rk && *rk) && !(tk && *tk)) {
        A(&t->e0_mask, T * N * (size_t)xh::sp8::kE0RecordBytes);
        if (t->qold)
          t->e0_p = t->qold;
        else
          A(&t->e0_p, T * N * (size_t)xh::sp8::kE0PBytes);
      }
    }
    if ((c.algo == XH_PPO || c.algo == XH_AC) && c.bins == 64 && c.dims == 2 &&
        c.policy_h1 == 128 && c.policy_h2 == 128) {
      // the packed batch (256 B per group: a quarter of the env-steps' count
      // when every env-step packs, one group per env-step at worst)
      A(&t->pk, xh::sp8::pk_max_groups(T * N) * (size_t)xh::sp8::kPkGroupBytes);
      A(&t->pk_hdr, (size_t)xh::sp8::kPkHdrInts * 4);
      A(&t->pk_cls, T * N);
      A(&t->pk_blk, xh::sp8::pk_scratch_ints(T * N) * 4);
      // the epoch on the table: the table batch, the logits, G and its bound,
      // the streaming pass's sums per workgroup
      A(&t->tab_pk, (size_t)xh::tb::kBytes);
      A(&t->tab_logits, (size_t)xh::lt::kEntries * 4);
      A(&t->tab_G, (size_t)xh::lt::kEntries * 4);
      A(&t->tab_gmax, 4);
      A(&t->tab_part, (size_t)t->pslab_n * xh::lt::kEntries * 8);
      A(&t->tab_ood, 4);
      // the lean table kernels' H2 (tail rows included) and their own slabs
      A(&t->tab_h2, (size_t)xh::tt::kRows * c.policy_h2 * 4);
      A(&t->tab_slab, (size_t)xh::tt::kTiles * t->pslab_stride * 4);
      if (st == XH_OK) {
        std::vector<uint8_t> tbh((size_t)xh::tb::kBytes);
        for (int g = 0; g < xh::tb::kGroups; ++g)
          xh::tb::fill_group(g, tbh.data() + (size_t)g * xh::sp8::kPkGroupBytes);
        st = copy_ok(copy_to_device(t->tab_pk, tbh.data(), tbh.size(), ctx->stream));
      }
    }
    if (c.algo == XH_KLPPO) {
      A(&t->beta, 4);
      A(&t->kl_log, (size_t)c.epochs * 3 * 4);
      A(&t->kl_part, (size_t)t->pslab_n * 8);
      A(&t->kl_sum, 2 * 8);
    }
    if (st == XH_OK && t->beta)
      st = copy_ok(copy_to_device(t->beta, &c.kl_beta, 4, ctx->stream));
    t->opt[XH_POLICY].lr = c.lr_policy;
    t->opt[XH_POLICY].wd = c.wd_policy;
    t->opt[XH_VALUE].lr = c.lr_value;
    t->opt[XH_VALUE].wd = c.wd_value;
    if (st != XH_OK) return fail_after(st, [&] { xh_trainer_destroy(t); });
    // a^(4T(Ng-1)): from this env's last draw of an iteration to its next.
    t->jump_mul = mstd_pow(4ull * T * (uint64_t)(c.num_envs_global - 1));
    hipError_t e = xh::launch_env_init(t->env, t->batch(), t->cfg.rng_state,
                                       c.env_offset, c.num_envs_global,
                                       ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      xh_trainer_destroy(t);
      return fail(XH_ERR_HIP, "env init: %s", hipGetErrorString(e));
    }
    t->counted = true;
    ++ctx->trainers;
    *out = t;
    return XH_OK;
  });
}

int xh_trainer_destroy(xh_trainer *t) {
  return guard([&]() -> int {
    if (!t) return XH_OK;
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    for (auto &ev : t->events) {
      (void)hipEventDestroy(ev.start);
      (void)hipEventDestroy(ev.stop);
    }
    for (hipEvent_t e : t->event_pool) (void)hipEventDestroy(e);
    for (void *p : t->allocs) (void)hipFree(p);
    stats_free(t);
    upd_free(t);
    clip_free(t, XH_POLICY);
    clip_free(t, XH_VALUE);
    if (t->pg.host_active) (void)hipHostFree(t->pg.host_active);
    xh_ctx *c = t->ctx;
    const bool counted = t->counted;
    delete t;
    ctx_release(c, counted);
    return XH_OK;
  });
}

size_t xh_trainer_num_params(const xh_trainer *t, int which) {
  if (!t) return 0;
  return which == XH_POLICY ? (size_t)t->np : (size_t)t->nv;
}

int xh_trainer_set_params(xh_trainer *t, int which, const float *host,
                          size_t n) {
  return guard([&]() -> int {
    if (!t || !host) return fail(XH_ERR_INVALID, "null arg");
    const size_t want = xh_trainer_num_params(t, which);
    if (n != want)
      return fail(XH_ERR_INVALID, "params: got %zu floats, model has %zu", n,
                  want);
    HIPCHK(hipSetDevice(t->ctx->device));
    wrote(t, wrote_net(which));
    float *dst = which == XH_POLICY ? t->pp : t->vp;
    HIPCHK(copy_to_device(dst, host, n * 4, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_get_params(xh_trainer *t, int which, float *host, size_t n) {
  return guard([&]() -> int {
    if (!t || !host) return fail(XH_ERR_INVALID, "null arg");
    const size_t want = xh_trainer_num_params(t, which);
    if (n != want)
      return fail(XH_ERR_INVALID, "params: got %zu floats, model has %zu", n,
                  want);
    HIPCHK(hipSetDevice(t->ctx->device));
    HIPCHK(copy_to_host(host, which == XH_POLICY ? t->pp : t->vp, n * 4,
                        t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_set_optimizer(xh_trainer *t, int which, int kind, float lr,
                             float weight_decay, float beta1, float beta2) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (which != XH_POLICY && which != XH_VALUE)
      return fail(XH_ERR_INVALID, "optimizer: which %d", which);
    if (kind != XH_OPT_SGD && kind != XH_OPT_MOMENTUM && kind != XH_OPT_ADAM)
      return fail(XH_ERR_INVALID, "optimizer: kind %d", kind);
    if (kind != XH_OPT_SGD && weight_decay != 0.0f)
      return fail(XH_ERR_INVALID, "optimizer: weight decay is an "
                  "sgd_optimizer parameter only (nn.h:616-628)");
    HIPCHK(hipSetDevice(t->ctx->device));
    auto &o = t->opt[which];
    const int n = which == XH_POLICY ? t->np : t->nv;
    if (kind != XH_OPT_SGD && !o.m) {
      CHK(dalloc(t, &o.m, (size_t)n * 4));
      CHK(dalloc(t, &o.v, (size_t)n * 4));
    }
    if (o.m) {  // fresh state: the reference emplaces zeros on the first step
      HIPCHK(hipMemsetAsync(o.m, 0, (size_t)n * 4, t->ctx->stream));
      HIPCHK(hipMemsetAsync(o.v, 0, (size_t)n * 4, t->ctx->stream));
    }
    o.kind = kind;
    o.lr = lr;
    o.wd = weight_decay;
    o.beta1 = beta1;
    o.beta2 = beta2;
    o.t = 1.0f;
    (which == XH_POLICY ? t->cfg.lr_policy : t->cfg.lr_value) = lr;
    (which == XH_POLICY ? t->cfg.wd_policy : t->cfg.wd_value) = weight_decay;
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_set_learning_rate(xh_trainer *t, int which, float lr) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (which != XH_POLICY && which != XH_VALUE)
      return fail(XH_ERR_INVALID, "learning rate: which %d", which);
    if (which == XH_VALUE && t->cfg.algo == XH_PG)
      return fail(XH_ERR_INVALID, "learning rate: REINFORCE has no value net");
    t->opt[which].lr = lr;
    (which == XH_POLICY ? t->cfg.lr_policy : t->cfg.lr_value) = lr;
    return XH_OK;
  });
}

int xh_trainer_set_record_last_step(xh_trainer *t, int on) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    t->cfg.record_last_step = on ? 1 : 0;
    return XH_OK;
  });
}

int xh_trainer_rollout(xh_trainer *t) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    HIPCHK(hipSetDevice(t->ctx->device));
    return do_rollout(t);
  });
}

int xh_trainer_learn(xh_trainer *t) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    HIPCHK(hipSetDevice(t->ctx->device));
    return do_learn(t);
  });
}

int xh_trainer_forget(xh_trainer *t) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    // replay_buffer::forget() keeps the last state of the open trajectories
    // of a window that exists: without a rollout since the last learn() /
    // forget() there is none, and slot T holds no start states to shift
    if (!t->rolled)
      return fail(XH_ERR_STATE, "forget: no rollout since the last learn() / "
                  "forget()");
    t->need_shift = true;  // as at the end of do_learn / do_pg_learn
    t->rolled = false;
    wrote(t, kWroteBatch);  // the window is gone
    t->stats.open = false;  // the row's learner part stays NaN
    return XH_OK;
  });
}

int xh_trainer_iterate(xh_trainer *t, int iterations) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    HIPCHK(hipSetDevice(t->ctx->device));
    for (int i = 0; i < iterations; ++i) {
      CHK(do_rollout(t));
      CHK(do_learn(t));
    }
    return XH_OK;
  });
}

int xh_trainer_set_forced_actions(xh_trainer *t, const int32_t *host) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    if (!host) {
      t->use_forced = false;
      return XH_OK;
    }
    const size_t n = t->T() * t->N();
    for (size_t i = 0; i < n; ++i)
      if (host[i] < 0 || host[i] >= t->cfg.bins)
        return fail(XH_ERR_INVALID, "forced action %d out of range", host[i]);
    HIPCHK(hipSetDevice(t->ctx->device));
    wrote(t, kWroteBatch);
    HIPCHK(copy_to_device(t->forced, host, n * 4, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    t->use_forced = true;
    return XH_OK;
  });
}

size_t xh_trainer_buffer_bytes(const xh_trainer *t, int which) {
  const buffer_view b = t ? buffer_of(t, which) : buffer_view{nullptr, 0};
  return b.ptr ? b.bytes : 0;
}

int xh_trainer_get_buffer(xh_trainer *t, int which, void *host, size_t bytes) {
  return guard([&]() -> int {
    if (!t || !host) return fail(XH_ERR_INVALID, "null arg");
    const size_t want = xh_trainer_buffer_bytes(t, which);
    if (!want || bytes != want)
      return fail(XH_ERR_INVALID, "buffer %d: %zu bytes, expected %zu", which,
                  bytes, want);
    if ((which == XH_BUF_LOGITS || which == XH_BUF_PROBS) &&
        t->cfg.algo != XH_PG && !t->last_step_recorded)
      return fail(XH_ERR_STATE, "buffer %d: no rollout recorded its last step "
                  "(xh_config.record_last_step is off)", which);
    HIPCHK(hipSetDevice(t->ctx->device));
    HIPCHK(copy_to_host(host, buffer_of(t, which).ptr, bytes, t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_set_buffer(xh_trainer *t, int which, const void *host,
                          size_t bytes) {
  return guard([&]() -> int {
    if (!t || !host) return fail(XH_ERR_INVALID, "null arg");
    const size_t want = xh_trainer_buffer_bytes(t, which);
    if (!want || bytes != want)
      return fail(XH_ERR_INVALID, "buffer %d: %zu bytes, expected %zu", which,
                  bytes, want);
    if (which == XH_BUF_ACTION) {
      const int32_t *a = static_cast<const int32_t *>(host);
      for (size_t i = 0; i < bytes / 4; ++i)
        if (a[i] < 0 || a[i] >= t->cfg.bins)
          return fail(XH_ERR_INVALID, "action %d out of range", a[i]);
    }
    const bool states = t->cfg.algo != XH_PG &&
                        (which == XH_BUF_BINS || which == XH_BUF_ITEMS);
    std::vector<char> wide;
    if (states && which == XH_BUF_BINS) {  // as xh_trainer_set_env_state
      const int8_t *b = static_cast<const int8_t *>(host);
      const size_t per_slot = t->N() * t->BD();
      wide.assign(t->T() + 1, 0);
      for (size_t i = 0; i < bytes; ++i) {
        if (b[i] > kBinCapacity)
          return fail(XH_ERR_INVALID, "bin value %d above the capacity %d",
                      b[i], kBinCapacity);
        if (b[i] < -kBinCapacity) wide[i / per_slot] = 1;
      }
    }
    std::vector<char> ok;
    if (states && which == XH_BUF_ITEMS) {
      const int8_t *v = static_cast<const int8_t *>(host);
      const size_t N = t->N(), D = (size_t)t->cfg.dims;
      ok.assign(t->T() + 1, 1);
      for (size_t sl = 0; sl <= t->T(); ++sl)
        for (size_t e = 0; e < N; ++e) {
          const int8_t *it = v + (sl * N + e) * 4;
          for (size_t d = 0; d < D; ++d)
            if (it[d] < 0 || it[d] > kBinCapacity)
              return fail(XH_ERR_INVALID, "item value %d outside [0, %d]", it[d],
                          kBinCapacity);
          if (!table_item(t->env, it)) ok[sl] = 0;
        }
    }
    HIPCHK(hipSetDevice(t->ctx->device));
    wrote(t, kWroteBatch);
    HIPCHK(copy_to_device(buffer_of(t, which).ptr, host, bytes,
                          t->ctx->stream));
    HIPCHK(hipStreamSynchronize(t->ctx->stream));
    if (which == XH_BUF_BINS || which == XH_BUF_ITEMS) t->need_shift = false;
    // statistics: uploaded bin states start new episodes, as
    // xh_trainer_set_env_state's do
    if (which == XH_BUF_BINS && t->stats.ep_len)
      HIPCHK(hipMemsetAsync(t->stats.ep_len, 0, t->N() * 4, t->ctx->stream));
    if (!ok.empty()) t->items_ok = std::move(ok);
    if (!wide.empty()) t->bins_wide = std::move(wide);
    return XH_OK;
  });
}

int xh_trainer_seed_streams(xh_trainer *t, uint32_t x) {
  return guard([&]() -> int {
    if (!t) return fail(XH_ERR_INVALID, "null trainer");
    x %= 2147483647u;
    HIPCHK(hipSetDevice(t->ctx->device));
    if (t->cfg.algo == XH_PG) {
      HIPCHK(xh::launch_pg_seed(t->batch(), x ? x : 1u, t->cfg.env_offset,
                                kEvalStride, t->ctx->stream));
      return XH_OK;
    }
    HIPCHK(xh::launch_env_seed(t->batch(), x ? x : 1u, t->cfg.env_offset,
                               t->ctx->stream));
    return XH_OK;
  });
}

int xh_trainer_get_env_state(xh_trainer *t, int first, int count, int8_t *bins,
                             int8_t *items) {
  return guard([&]() -> int {
    CHK(check_env_range(t, first, count, bins, items));
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    const size_t BD = t->BD(), D = (size_t)t->cfg.dims, N = t->N();
    const size_t slot = t->need_shift ? t->T() : 0;
    std::vector<int8_t> it((size_t)count * 4);
    HIPCHK(copy_to_host(bins, t->bins + (slot * N + first) * BD,
                        (size_t)count * BD, s));
    HIPCHK(copy_to_host(it.data(), t->items + (slot * N + first) * 4,
                        (size_t)count * 4, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int e = 0; e < count; ++e) {
      auto o = t->env_override.find(first + e);
      if (o != t->env_override.end()) {
        std::memcpy(bins + (size_t)e * BD, o->second.data(), BD);
        std::memcpy(items + (size_t)e * D, o->second.data() + BD, D);
      } else {
        std::memcpy(items + (size_t)e * D, it.data() + (size_t)e * 4, D);
      }
    }
    return XH_OK;
  });
}

int xh_trainer_set_env_state(xh_trainer *t, int first, int count,
                             const int8_t *bins, const int8_t *items) {
  return guard([&]() -> int {
    CHK(check_env_range(t, first, count, bins, items));
    const size_t BD = t->BD(), D = (size_t)t->cfg.dims;
    // negative values are the overflowed (game-over) states an apply by hand
    // leaves (bin_packing.h:53-63); applying to a game-over env again keeps
    // subtracting, so any int8 value up to the capacity is a reachable state
    // (below -capacity the next rollout step / learn() run the f32 kernels,
    // bins_wide)
    for (size_t i = 0; i < (size_t)count * BD; ++i)
      if (bins[i] > kBinCapacity)
        return fail(XH_ERR_INVALID, "bin value %d above the capacity %d",
                    bins[i], kBinCapacity);
    // a whole item-table entry (the train kernels carry the item columns of
    // dW1 as per-entry sums)
    for (int e = 0; e < count; ++e)
      if (!table_item(t->env, items + e * D))
        return fail(XH_ERR_INVALID, "env %d: item is not an item-table entry",
                    first + e);
    if (count > 0) wrote(t, kWroteBatch);
    for (int e = 0; e < count; ++e) {
      std::vector<int8_t> v(BD + D);
      std::memcpy(v.data(), bins + (size_t)e * BD, BD);
      std::memcpy(v.data() + BD, items + (size_t)e * D, D);
      t->env_override[first + e] = std::move(v);
    }
    // statistics: a replaced state starts a new episode (ordered on the
    // stream after the last window's episode_stats_kernel)
    if (t->stats.ep_len && count > 0) {
      HIPCHK(hipSetDevice(t->ctx->device));
      HIPCHK(hipMemsetAsync(t->stats.ep_len + first, 0, (size_t)count * 4,
                            t->ctx->stream));
    }
    return XH_OK;
  });
}

}  // extern "C"
