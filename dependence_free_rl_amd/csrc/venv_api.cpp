// venv_api.cpp -- the vectorised envs of the C ABI (include/xylo_hip.h,
// "venv"): N envs stepped by one kernel per call for a caller's own policy
// (xh_venv_create / step / act / apply / reset / observe, venv_kernels.hip),
// the trajectory record with its optional distributions and legal words, the
// learner's side of a recorded window (record_obs / record_ends / advantages,
// venv_learn_kernels.hip) and the loss head (policy_loss / kl_beta,
// venv_loss_kernels.hip), the opt-in episode statistics (set_episode_stats /
// episode_row, venv_episode_kernels.hip) and the logit tables (table_info /
// table_obs / act_table / table_gather / table_grad, venv_table_kernels.hip,
// xh_venv_table.h).  A venv holds a reference on its
// context and never touches a trainer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../include/xylo_hip.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_venv_table.h"

using namespace xh::host;

// The record's arrays: the six XH_VREC_* of xh_venv_set_record, then two that
// the public `which` does not reach and that are dropped with the record --
// kRecDistrib (xh_venv_set_record_distrib): f32 [rec_steps][N][B], the p[] each
// recorded xh_venv_act sampled from; kRecLegal (xh_venv_set_action_mask, while
// it is on): u32 [rec_steps][N][W], the legal words each one masked with.
enum { kRecDistrib = XH_VREC_COUNT, kRecLegal, kRecArrays };

struct xh_venv {
  // one device array of the record: null / 0 while it does not exist
  struct array {
    void *ptr = nullptr;
    size_t bytes = 0;
  };
  xh_ctx *ctx = nullptr;
  xh::EnvDesc env{};
  int N = 0, Ng = 0, offset = 0, policy_draws = 0;
  uint32_t skip_mul = 1, jump_mul = 1;
  void *buf[XH_VENV_BUF_COUNT] = {};
  size_t bytes[XH_VENV_BUF_COUNT] = {};
  int *err = nullptr;
  bool counted = false;
  // xh_venv_set_timing: HIP events around every step / apply / reset /
  // observe launch on the context's stream
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // recorded pairs
  std::vector<hipEvent_t> event_pool;  // recycled by set_timing
  // xh_venv_set_record: the trajectory record xh_venv_act writes
  int rec_steps = 0, rec_pos = 0;
  array rec[kRecArrays];
  bool mask_on = false;  // xh_venv_set_action_mask
  // the item set in use (xh_venv_get_item_set): the default set until
  // xh_venv_create_ex / xh_venv_set_item_set gives one.  `general`: one was
  // given, and every launch runs the general kernels on `table`, which goes
  // with the launch's arguments -- so a switch is ordered on the stream
  bool general = false;
  xh_item_set items{};
  xh::VenvItemTable table{};
  const xh::VenvItemTable *tab() const { return general ? &table : nullptr; }
  // xh_venv_legal's own [N][W] output, allocated at its first use
  uint32_t *legal_buf = nullptr;
  // scratch of xh_venv_record_ends / xh_venv_advantages, allocated at their
  // first use: launch_end_list's block totals and n_open; the scan's block
  // partials [venv_gae_grid(N)][2], their ended-row counts, and stats [4]
  int *end_scratch = nullptr;
  double *adv_part = nullptr, *adv_stats = nullptr;
  int *adv_end_part = nullptr;
  // xh_venv_policy_loss's block partials [kVenvLossMaxBlocks][XH_VLOSS_COUNT],
  // allocated at the first call that asks for stats
  double *loss_part = nullptr;
  // ... and its kl_stats partials [kVenvLossMaxBlocks][XH_VKL_COUNT], at the
  // first call that asks for kl_stats
  double *kl_part = nullptr;
  // ... and xh_venv_policy_loss_ex's ext_stats partials [kVenvLossMaxBlocks]
  // [XH_VEXT_COUNT], at the first call that asks for ext_stats
  double *ext_part = nullptr;
  // xh_venv_table_grad's scratch, allocated at its first use: the maximum's
  // bit pattern (16 bytes) and XH_VTAB_MAX_ENTRIES int64 sums
  void *tab_scratch = nullptr;
  // xh_venv_set_episode_stats (opt-in; everything null / 0 while off): the
  // per-env blocks the step / act / apply launches count into, the row
  // kernel's workgroup partials, and the device ring of XH_VEP_COUNT doubles
  // per row (ring.rows counts the rows taken); `calls` counts the launches
  // since the last one
  struct episode_stats {
    xh::host::row_ring ring{nullptr, XH_VEP_COUNT};
    long calls = 0;
    int32_t *state[XH_VEPS_COUNT] = {};  // XH_VEPS_RUNNING, XH_VEPS_FIRST
    xh::VenvEpAcc *acc = nullptr;
    double *psum = nullptr, *pext = nullptr;
  } ep;

  template <class T>
  T *rec_as(int entry) const {
    return static_cast<T *>(rec[entry].ptr);
  }

  xh::VenvArgs args() const {
    xh::VenvArgs a{};
    a.env = env;
    a.N = N;
    a.bins = (int8_t *)buf[XH_VENV_BINS];
    a.items = (int8_t *)buf[XH_VENV_ITEMS];
    a.rng = (uint32_t *)buf[XH_VENV_RNG];
    a.action = (const int32_t *)buf[XH_VENV_ACTIONS];
    a.reward = (float *)buf[XH_VENV_REWARD];
    a.done = (uint8_t *)buf[XH_VENV_DONE];
    a.err = err;
    a.skip_mul = skip_mul;
    a.jump_mul = jump_mul;
    a.ep_running = ep.state[XH_VEPS_RUNNING];
    a.ep_first = ep.state[XH_VEPS_FIRST];
    a.ep_acc = ep.acc;
    return a;
  }
};

namespace {

// ---- item sets ----
// XH_OK, or XH_ERR_INVALID with the first rule of include/xylo_hip.h the set
// breaks; touches nothing
int item_set_check(const xh_item_set *s, int D) {
  if (!s) return fail(XH_ERR_INVALID, "item set: null");
  if (D < 1 || D > 3) return fail(XH_ERR_INVALID, "item set: dims %d (1..3)", D);
  const int K = s->num_items;
  if (K < 1 || K > XH_ITEMS_MAX)
    return fail(XH_ERR_INVALID, "item set: %d items (1..%d)", K, XH_ITEMS_MAX);
  for (int d = 0; d < D; ++d)
    if (s->capacity[d] < 1 || s->capacity[d] > 64)
      return fail(XH_ERR_INVALID, "item set: capacity %d of dim %d (1..64)",
                  s->capacity[d], d);
  double sum = 0.0;
  for (int k = 0; k < K; ++k) {
    bool any = false;
    for (int d = 0; d < D; ++d) {
      if (s->item[k][d] < 0 || s->item[k][d] > s->capacity[d])
        return fail(XH_ERR_INVALID, "item set: item %d is %d in dim %d "
                    "(0..%d, the capacity)", k, s->item[k][d], d,
                    s->capacity[d]);
      any |= s->item[k][d] > 0;
    }
    if (!any)
      return fail(XH_ERR_INVALID, "item set: item %d is zero in every dim (its "
                  "episodes would never end)", k);
    if (!(s->weight[k] >= 0.0) || !std::isfinite(s->weight[k]))
      return fail(XH_ERR_INVALID, "item set: weight %g of item %d (finite, "
                  ">= 0)", s->weight[k], k);
    sum += s->weight[k];
  }
  if (!(sum > 0.0) || !std::isfinite(sum))
    return fail(XH_ERR_INVALID, "item set: the weights sum to %g", sum);
  return XH_OK;
}

// the K thresholds of a checked set (include/xylo_hip.h: the draw)
void item_set_thresholds(const xh_item_set &s, double *c) {
  const int K = s.num_items;
  double W = 0.0;
  for (int k = 0; k < K; ++k) W += s.weight[k];
  double acc = 0.0;
  int last = 0;  // the last item of positive weight
  for (int k = 0; k < K; ++k) {
    acc += s.weight[k] / W;
    c[k] = acc;
    if (s.weight[k] > 0.0) last = k;
  }
  for (int k = last; k < K; ++k) c[k] = 1.0;
}

// the kernels' table of a checked set
xh::VenvItemTable item_set_table(const xh_item_set &s, int D) {
  xh::VenvItemTable t{};
  double c[XH_ITEMS_MAX];
  item_set_thresholds(s, c);
  for (int k = 0; k < xh::kVenvItemsMax; ++k) {
    t.thr[k] = k < s.num_items ? c[k] : 1.0;
    uint32_t w = 0;
    for (int d = 0; d < D && k < s.num_items; ++d)
      w |= (uint32_t)(s.item[k][d] & 0xff) << (8 * d);
    t.shape[k] = w;
  }
  for (int d = 0; d < 4; ++d) t.cap[d] = d < D ? s.capacity[d] : 1;
  return t;
}

// a copy with everything past K and past D zeroed (what get_item_set returns)
xh_item_set item_set_clean(const xh_item_set &s, int D) {
  xh_item_set o{};
  o.num_items = s.num_items;
  for (int d = 0; d < D; ++d) o.capacity[d] = s.capacity[d];
  for (int k = 0; k < s.num_items; ++k) {
    for (int d = 0; d < D; ++d) o.item[k][d] = s.item[k][d];
    o.weight[k] = s.weight[k];
  }
  return o;
}

// An array allocated (zeroed on the stream) at its first use; the slot stays
// NULL when that fails.  XH_VENV_POLICY / PCHOICE are such, so a venv that
// never acts holds nothing for xh_venv_act, and xh_venv_legal's own output.
int venv_ensure(xh_venv *v, void **slot, size_t bytes, const char *what) {
  if (*slot) return XH_OK;
  HIPCHK(hipSetDevice(v->ctx->device));
  return dev_zalloc(v->ctx->stream, slot, bytes, what);
}
int venv_ensure(xh_venv *v, int which) {
  return venv_ensure(v, &v->buf[which], v->bytes[which], "venv");
}
int venv_ensure_legal_buf(xh_venv *v) {
  return venv_ensure(v, (void **)&v->legal_buf,
                     (size_t)v->N * xh::venv_legal_words(v->env.B) * 4,
                     "venv legal");
}

// ---- the record's arrays ----
int rec_alloc(xh_venv *v, int entry, size_t bytes, const char *what) {
  CHK(dev_zalloc(v->ctx->stream, &v->rec[entry].ptr, bytes, what));
  v->rec[entry].bytes = bytes;
  return XH_OK;
}

// the record's zero-filled legal words (the mask is on, a record exists)
int rec_alloc_legal(xh_venv *v) {
  return rec_alloc(v, kRecLegal, (size_t)v->rec_steps * v->N *
                                     xh::venv_legal_words(v->env.B) * 4,
                   "venv action mask");
}

void venv_free_record(xh_venv *v) {
  for (xh_venv::array &a : v->rec) {
    if (a.ptr) (void)hipFree(a.ptr);
    a = xh_venv::array{};
  }
  v->rec_steps = v->rec_pos = 0;
}

// one array of a record that stays: the stream may still write it
int rec_drop(xh_venv *v, int entry) {
  xh_venv::array &a = v->rec[entry];
  if (!a.ptr) return XH_OK;
  HIPCHK(hipStreamSynchronize(v->ctx->stream));
  (void)hipFree(a.ptr);
  a = xh_venv::array{};
  return XH_OK;
}

size_t rec_bytes(const xh_venv *v, int entry) {
  return v ? v->rec[entry].bytes : 0;
}
void *rec_ptr(const xh_venv *v, int entry) {
  return v ? v->rec[entry].ptr : nullptr;
}

// entry < 0: no such array (a public `which` outside its range)
int rec_to_host(xh_venv *v, int entry, void *host, size_t bytes,
                const char *what) {
  return guard([&]() -> int {
    if (!v || !host) return fail(XH_ERR_INVALID, "null arg");
    const xh_venv::array a = entry < 0 ? xh_venv::array{} : v->rec[entry];
    if (!a.ptr || bytes != a.bytes)
      return fail(XH_ERR_INVALID, "%s: %zu bytes, expected %zu", what, bytes,
                  a.bytes);
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(copy_to_host(host, a.ptr, bytes, v->ctx->stream));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    return XH_OK;
  });
}

bool vrec_which(int which) { return which >= 0 && which < XH_VREC_COUNT; }

// the body of an ABI call on a venv: no exception crosses, NULL is refused
template <class F>
int venv_call(xh_venv *v, F &&f) {
  return guard([&]() -> int {
    return v ? f() : fail(XH_ERR_INVALID, "null venv");
  });
}

int venv_check_err(xh_venv *v) {
  int err = 0;
  HIPCHK(copy_to_host(&err, v->err, 4, v->ctx->stream));
  HIPCHK(hipStreamSynchronize(v->ctx->stream));
  if (!err) return XH_OK;
  HIPCHK(hipMemsetAsync(v->err, 0, 4, v->ctx->stream));
  HIPCHK(hipStreamSynchronize(v->ctx->stream));
  if (err & 8)
    return fail(XH_ERR_INVALID, "venv table: a state outside the table's "
                "domain (a bin outside [0, capacity], or an item that is none "
                "of the set's shapes) or a NaN / infinity in dout; those envs, "
                "output rows or g_dev were left untouched%s%s%s",
                err & 4 ? ", and a row index was outside its rows" : "",
                err & 2 ? ", and a policy row was refused" : "",
                err & 1 ? ", and an action was out of range" : "");
  if (err & 4)
    return fail(XH_ERR_INVALID, "venv: xh_venv_record_obs or "
                "xh_venv_policy_loss met a row index outside its rows (the "
                "loss: or an action outside its range); those output rows "
                "were left untouched%s%s",
                err & 2 ? ", and a policy row was refused" : "",
                err & 1 ? ", and an action was out of range" : "");
  if (err & 2)
    return fail(XH_ERR_INVALID, "venv: a policy row was refused (a NaN, a "
                "negative probability, or a sum that is zero or not finite)"
                "%s; those envs were left untouched",
                err & 1 ? ", and an action was out of range" : "");
  return fail(XH_ERR_INVALID, "venv: an action was outside [0, %d); those "
              "envs were left untouched", v->env.B);
}

// xh_venv_get / xh_venv_set: the buffer exists and `bytes` is its size
int venv_check_buffer(const xh_venv *v, int which, const void *host,
                      size_t bytes) {
  if (!v || !host) return fail(XH_ERR_INVALID, "null arg");
  if (which < 0 || which >= XH_VENV_BUF_COUNT || bytes != v->bytes[which])
    return fail(XH_ERR_INVALID, "venv buffer %d: %zu bytes, expected %zu",
                which, bytes, xh_venv_bytes(v, which));
  return XH_OK;
}

// one launch on the context's stream, bracketed by HIP events when timing
template <class F>
int venv_timed(xh_venv *v, F &&launch) {
  // events from a pool (no creation per launch); a pair is kept only once
  // both of its records are on the stream, so a failed launch leaves no
  // half-recorded pair behind
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (v->timing) {
    HIPCHK(pooled_event(v->event_pool, &ev.first));
    HIPCHK(pooled_event(v->event_pool, &ev.second));
    HIPCHK(hipEventRecord(ev.first, v->ctx->stream));
  }
  const hipError_t e = launch();
  if (e != hipSuccess) {
    if (v->timing) {
      v->event_pool.push_back(ev.first);
      v->event_pool.push_back(ev.second);
    }
    return fail(XH_ERR_HIP, "venv launch: %s", hipGetErrorString(e));
  }
  if (v->timing) {
    HIPCHK(hipEventRecord(ev.second, v->ctx->stream));
    v->events.push_back(ev);
  }
  return XH_OK;
}

// ---- what xh_venv_act and xh_venv_act_heuristic share ----
// the record has a free slot; the device is current and PCHOICE exists
int venv_act_ready(xh_venv *v, const char *what) {
  if (v->rec_steps > 0 && v->rec_pos >= v->rec_steps)
    return fail(XH_ERR_STATE, "%s: the record's %d slots are full "
                "(xh_venv_record_rewind)", what, v->rec_steps);
  HIPCHK(hipSetDevice(v->ctx->device));
  return venv_ensure(v, XH_VENV_PCHOICE);
}

// an act launch's arguments but for its policy: agent::step's, the outputs,
// the record's slot at the cursor and the mask's switch
xh::VenvActArgs venv_act_args(const xh_venv *v, bool write_obs) {
  xh::VenvActArgs a{};
  a.v = v->args();
  a.v.mode = 1;
  a.v.obs = write_obs ? (float *)v->buf[XH_VENV_OBS] : nullptr;
  a.action = (int32_t *)v->buf[XH_VENV_ACTIONS];
  a.pchoice = (float *)v->buf[XH_VENV_PCHOICE];
  if (v->rec_steps > 0) {
    a.rec_action = v->rec_as<int32_t>(XH_VREC_ACTION);
    a.rec_pchoice = v->rec_as<float>(XH_VREC_PCHOICE);
    a.rec_reward = v->rec_as<float>(XH_VREC_REWARD);
    a.rec_done = v->rec_as<uint8_t>(XH_VREC_DONE);
    a.rec_bins = v->rec_as<int8_t>(XH_VREC_BINS);
    a.rec_items = v->rec_as<int8_t>(XH_VREC_ITEMS);
    a.slot = v->rec_pos;
    a.rec_legal = v->rec_as<uint32_t>(kRecLegal);
  }
  a.legal = v->mask_on ? 1 : 0;
  return a;
}

// after the launch: the cursor and the episode statistics' call count
int venv_act_done(xh_venv *v, int st) {
  if (st == XH_OK && v->rec_steps > 0) ++v->rec_pos;
  if (st == XH_OK && v->ep.ring.history) ++v->ep.calls;
  return st;
}

int venv_launch(xh_venv *v, int op, int mode, bool use_mask, bool obs) {
  HIPCHK(hipSetDevice(v->ctx->device));
  xh::VenvArgs a = v->args();
  a.mode = mode;
  a.mask = use_mask ? (const uint8_t *)v->buf[XH_VENV_MASK] : nullptr;
  a.obs = obs ? (float *)v->buf[XH_VENV_OBS] : nullptr;
  if (op == xh::kVenvObserve) a.obs = (float *)v->buf[XH_VENV_OBS];
  if (mode == 0) a.reward = nullptr;
  CHK(venv_timed(
      v, [&] { return xh::launch_venv(a, op, v->ctx->stream, v->tab()); }));
  if (op == xh::kVenvStep && v->ep.ring.history) ++v->ep.calls;
  return XH_OK;
}

// the recorded pairs back into the pool (the stream is synchronised first)
void venv_drop_events(xh_venv *v) {
  for (auto &ev : v->events) {
    v->event_pool.push_back(ev.first);
    v->event_pool.push_back(ev.second);
  }
  v->events.clear();
}

// ---- episode statistics ----
constexpr int kMaxEpisodeRows = 1 << 20;  // the trainer's bound: 100 MB

// the stream must be idle
void venv_free_episode_stats(xh_venv *v) {
  auto &ep = v->ep;
  for (int32_t *p : ep.state)
    if (p) (void)hipFree(p);
  if (ep.acc) (void)hipFree(ep.acc);
  if (ep.psum) (void)hipFree(ep.psum);
  if (ep.pext) (void)hipFree(ep.pext);
  if (ep.ring.dev) (void)hipFree(ep.ring.dev);
  ep = xh_venv::episode_stats{};
}

bool veps_which(int which) { return which >= 0 && which < XH_VEPS_COUNT; }

// xh_venv_episode_get / _set: statistics are on, the array exists and `bytes`
// is its size
int venv_check_episode_array(const xh_venv *v, int which, const void *host,
                             size_t bytes, const char *what) {
  if (!v || !host) return fail(XH_ERR_INVALID, "null arg");
  if (!v->ep.ring.history)
    return fail(XH_ERR_STATE, "%s: episode statistics are off "
                "(xh_venv_set_episode_stats)", what);
  if (!veps_which(which) || bytes != (size_t)v->N * 4)
    return fail(XH_ERR_INVALID, "%s %d: %zu bytes, expected %zu", what, which,
                bytes, xh_venv_episode_bytes(v, which));
  return XH_OK;
}

// ---- xh_venv_policy_loss, in the order its refusals are tested ----

// what a call reads besides the caller's own arrays: each is the caller's
// pointer, or with NULL the record's
struct loss_inputs {
  const uint32_t *legal = nullptr;  // masked calls only
  const float *distrib = nullptr;   // read only when want_q
  bool want_q = false;              // the rows' sampling distributions
  long total = 0;                   // rows the row indices run over
};

// the legal words and the distributions, with the checks of the scalars
int loss_resolve_inputs(const xh_venv *v, const xh_venv_loss *p, bool masked,
                        const uint32_t *legal_dev, loss_inputs *in) {
  if (masked) {
    in->legal = legal_dev ? legal_dev : v->rec_as<const uint32_t>(kRecLegal);
    if (!in->legal)
      return fail(XH_ERR_STATE, "venv policy loss: legal_dev NULL takes the "
                  "record's legal words and there are none "
                  "(xh_venv_set_action_mask with a record)");
    if (!legal_dev && (p->action || p->p_old))
      return fail(XH_ERR_INVALID, "venv policy loss: the record's legal "
                  "words go with the record's rows (action and p_old NULL)");
    if (reinterpret_cast<uintptr_t>(in->legal) & 3)
      return fail(XH_ERR_INVALID, "venv policy loss: legal_dev must be "
                  "4-byte aligned");
  }
  if (!p->policy || !p->adv || !p->grad)
    return fail(XH_ERR_INVALID, "venv policy loss: null policy / adv / grad");
  if (p->kind != XH_ACT_PROBS && p->kind != XH_ACT_LOGITS)
    return fail(XH_ERR_INVALID, "venv policy loss: kind %d (XH_ACT_PROBS / "
                "LOGITS)", p->kind);
  const bool kl_loss = p->loss == XH_LOSS_KL_REGULATED;
  if (p->loss != XH_LOSS_SOFTMAX_GRADIENT_LOG && p->loss != XH_LOSS_CLIPPED &&
      !kl_loss)
    return fail(XH_ERR_INVALID, "venv policy loss: loss %d "
                "(XH_LOSS_SOFTMAX_GRADIENT_LOG / XH_LOSS_CLIPPED / "
                "XH_LOSS_KL_REGULATED)", p->loss);
  in->want_q = kl_loss || p->kl_stats;
  in->distrib = p->distrib ? p->distrib : v->rec_as<const float>(kRecDistrib);
  if (in->want_q && !in->distrib)
    return fail(XH_ERR_INVALID, "venv policy loss: %s needs each row's "
                "sampling distribution: pass distrib, or record it "
                "(xh_venv_set_record_distrib)",
                kl_loss ? "XH_LOSS_KL_REGULATED" : "kl_stats");
  if (kl_loss && !p->beta_dev && !(p->beta >= 0.0f && std::isfinite(p->beta)))
    return fail(XH_ERR_INVALID, "venv policy loss: beta %g", (double)p->beta);
  if (p->first < 0 || p->count < 0 || p->total < 0)
    return fail(XH_ERR_INVALID, "venv policy loss: first %ld, count %ld, "
                "total %ld", p->first, p->count, p->total);
  if (p->loss == XH_LOSS_CLIPPED && !(p->eps > 0.0f && std::isfinite(p->eps)))
    return fail(XH_ERR_INVALID, "venv policy loss: eps %g", (double)p->eps);
  if (p->values_new && (!p->target || !p->dvalue))
    return fail(XH_ERR_INVALID, "venv policy loss: values_new needs target "
                "and dvalue");
  return XH_OK;
}

// rows read from the record: total == 0 means what it holds (`of` them),
// more than that is refused
int loss_total_of_record(const xh_venv *v, long *total, const char *of) {
  const long recorded = (long)v->rec_pos * v->N;
  if (*total == 0) *total = recorded;
  if (*total > recorded)
    return fail(XH_ERR_INVALID, "venv policy loss: total %ld, the record "
                "holds %s%ld rows", *total, of, recorded);
  return XH_OK;
}

int loss_resolve_total(const xh_venv *v, const xh_venv_loss *p,
                       loss_inputs *in) {
  in->total = p->total;
  if (!p->action || !p->p_old) {
    if (v->rec_steps <= 0)
      return fail(XH_ERR_STATE, "venv policy loss: action / p_old NULL take "
                  "the record's and there is no record (xh_venv_set_record)");
    CHK(loss_total_of_record(v, &in->total, ""));
  }
  if (in->want_q && !p->distrib)
    CHK(loss_total_of_record(v, &in->total, "the distributions of "));
  if (!p->rows_dev && p->first + p->count > in->total)
    return fail(XH_ERR_INVALID, "venv policy loss: rows %ld .. %ld of %ld",
                p->first, p->first + p->count - 1, in->total);
  return XH_OK;
}

// alignment and overlap of policy / grad / probs_out / distrib
int loss_check_memory(const xh_venv_loss *p, int B, const loss_inputs &in) {
  const uintptr_t bytes = (uintptr_t)p->count * B * 4;
  const uintptr_t pol = reinterpret_cast<uintptr_t>(p->policy);
  const uintptr_t grd = reinterpret_cast<uintptr_t>(p->grad);
  const uintptr_t prb = reinterpret_cast<uintptr_t>(p->probs_out);
  if ((pol | grd | prb) & 15)
    return fail(XH_ERR_INVALID, "venv policy loss: policy, grad and "
                "probs_out must be 16-byte aligned (the kernel moves "
                "16-byte pieces)");
  auto overlap = [&](uintptr_t x, uintptr_t y) {
    return x < y + bytes && y < x + bytes;
  };
  if ((grd != pol && overlap(grd, pol)) ||
      (prb && (overlap(prb, pol) || overlap(prb, grd))))
    return fail(XH_ERR_INVALID, "venv policy loss: grad may be policy "
                "itself; any other overlap of policy, grad and probs_out "
                "is refused");
  if (!in.want_q) return XH_OK;
  const uintptr_t dst = reinterpret_cast<uintptr_t>(in.distrib);
  const uintptr_t dbytes = (uintptr_t)in.total * B * 4;
  if (dst & 15)
    return fail(XH_ERR_INVALID, "venv policy loss: distrib must be 16-byte "
                "aligned (the kernel reads 16-byte pieces)");
  auto hits = [&](uintptr_t x) {
    return x && x < dst + dbytes && dst < x + bytes;
  };
  if (hits(grd) || hits(prb))
    return fail(XH_ERR_INVALID, "venv policy loss: distrib overlaps grad "
                "or probs_out");
  return XH_OK;
}

// xh_venv_policy_loss_ex's own refusals
int loss_check_ext(const xh_venv_loss *p, const xh_venv_loss_ext *x) {
  if (x->legal_dev && !x->masked)
    return fail(XH_ERR_INVALID, "venv policy loss: legal_dev without masked");
  if (!x->ent_coef_dev &&
      !(x->ent_coef >= 0.0f && std::isfinite(x->ent_coef)))
    return fail(XH_ERR_INVALID, "venv policy loss: ent_coef %g",
                (double)x->ent_coef);
  if (x->v_old && !p->values_new)
    return fail(XH_ERR_INVALID, "venv policy loss: v_old needs values_new "
                "(the value head)");
  if (x->v_old && !(x->vclip > 0.0f && std::isfinite(x->vclip)))
    return fail(XH_ERR_INVALID, "venv policy loss: vclip %g",
                (double)x->vclip);
  return XH_OK;
}

// the extension is off: the call is xh_venv_policy_loss[_masked] itself
bool loss_ext_off(const xh_venv_loss_ext *x) {
  return !x || (x->ent_coef == 0.0f && !x->ent_coef_dev && !x->v_old &&
                !x->ext_stats);
}

xh::VenvLossArgs loss_args(const xh_venv *v, const xh_venv_loss *p,
                           const loss_inputs &in) {
  xh::VenvLossArgs a{};
  a.B = v->env.B;
  if (in.want_q) {
    a.distrib = in.distrib;
    a.beta = p->beta;
    a.beta_dev = p->beta_dev;
    a.kl_part = p->kl_stats ? v->kl_part : nullptr;
  }
  a.logits = p->kind == XH_ACT_LOGITS;
  a.loss = p->loss;
  a.policy = p->policy;
  a.rows = p->rows_dev;
  a.first = p->first;
  a.count = p->count;
  a.total = in.total;
  a.adv = p->adv;
  a.action = p->action ? p->action : v->rec_as<const int32_t>(XH_VREC_ACTION);
  a.p_old = p->p_old ? p->p_old : v->rec_as<const float>(XH_VREC_PCHOICE);
  a.eps = p->eps;
  a.scale = p->scale;
  a.values_new = p->values_new;
  a.target = p->target;
  a.value_scale = p->value_scale;
  a.grad = p->grad;
  a.dvalue = p->dvalue;
  a.probs_out = p->probs_out;
  a.part = p->stats ? v->loss_part : nullptr;
  a.err = v->err;
  a.legal = in.legal;
  return a;
}

// xh_venv_policy_loss (masked == false; legal_dev unused),
// xh_venv_policy_loss_masked (legal_dev, or with NULL the record's words) and
// xh_venv_policy_loss_ex (x: its block, which gives masked and legal_dev; an
// x that leaves the extension off changes nothing below its checks)
int venv_policy_loss(xh_venv *v, const xh_venv_loss *p, bool masked,
                     const uint32_t *legal_dev,
                     const xh_venv_loss_ext *x = nullptr) {
  return venv_call(v, [&]() -> int {
    if (!p) return fail(XH_ERR_INVALID, "venv policy loss: null args");
    if (x) {
      CHK(loss_check_ext(p, x));
      masked = x->masked != 0;
      legal_dev = x->legal_dev;
      if (loss_ext_off(x)) x = nullptr;
    }
    loss_inputs in;
    CHK(loss_resolve_inputs(v, p, masked, legal_dev, &in));
    CHK(loss_resolve_total(v, p, &in));
    if (p->count == 0) return XH_OK;
    if (in.total == 0)
      return fail(XH_ERR_INVALID, "venv policy loss: %ld rows of none",
                  p->count);
    const int B = v->env.B;
    CHK(loss_check_memory(p, B, in));
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    if (p->stats && !v->loss_part)
      HIPCHK(hipMalloc((void **)&v->loss_part,
                       (size_t)xh::kVenvLossMaxBlocks * XH_VLOSS_COUNT * 8));
    if (p->kl_stats && !v->kl_part)
      HIPCHK(hipMalloc((void **)&v->kl_part,
                       (size_t)xh::kVenvLossMaxBlocks * XH_VKL_COUNT * 8));
    if (x && x->ext_stats && !v->ext_part)
      HIPCHK(hipMalloc((void **)&v->ext_part,
                       (size_t)xh::kVenvLossMaxBlocks * XH_VEXT_COUNT * 8));
    xh::VenvLossArgs a = loss_args(v, p, in);
    if (x) {
      a.ext = 1;
      a.ent_coef = x->ent_coef;
      a.ent_coef_dev = x->ent_coef_dev;
      a.v_old = x->v_old;
      a.vclip = x->vclip;
      a.ext_part = x->ext_stats ? v->ext_part : nullptr;
    }
    CHK(venv_timed(v, [&] { return xh::launch_venv_policy_loss(a, s); }));
    hipError_t e = hipSuccess;
    if (p->stats)
      e = xh::launch_venv_loss_reduce(v->loss_part,
                                      xh::venv_loss_grid(B, p->count),
                                      p->accumulate != 0, p->stats, s);
    if (e == hipSuccess && p->kl_stats)
      e = xh::launch_venv_kl_reduce(v->kl_part, xh::venv_loss_grid(B, p->count),
                                    p->accumulate != 0, p->kl_stats, s);
    if (e == hipSuccess && x && x->ext_stats)
      e = xh::launch_venv_ext_reduce(v->ext_part,
                                     xh::venv_loss_grid(B, p->count),
                                     p->accumulate != 0, x->ext_stats, s);
    if (e != hipSuccess)
      return fail(XH_ERR_HIP, "venv policy loss: %s", hipGetErrorString(e));
    return XH_OK;
  });
}

// ---- logit tables ----
// the domain of a checked set; XH_ERR_INVALID, naming E, past the limit
int table_domain(const xh_item_set &s, int D, xh::VenvTabDomain *m) {
  const xh::vt::Domain d = xh::vt::domain(s.capacity, D, s.num_items);
  if (d.entries > XH_VTAB_MAX_ENTRIES)
    return fail(XH_ERR_INVALID, "venv table: the set's domain has E = %ld "
                "entries (%d items x %d bin states), the limit is %d "
                "(XH_VTAB_MAX_ENTRIES); such a venv keeps the per-row calls",
                d.entries, d.K, d.states, XH_VTAB_MAX_ENTRIES);
  *m = xh::VenvTabDomain{};
  m->D = D;
  m->K = d.K;
  for (int i = 0; i < 4; ++i) m->side[i] = d.side[i];
  m->states = d.states;
  m->entries = d.entries;
  return XH_OK;
}

void table_info(const xh::VenvTabDomain &m, int B,
                struct xh_venv_table_info *out) {
  out->entries = (int)m.entries;
  out->states = m.states;
  out->items = m.K;
  out->rows = (int)xh::vt::rows(m.entries, B);
  for (int d = 0; d < 4; ++d) out->side[d] = m.side[d];
}

// what xh_venv_table_gather and xh_venv_table_grad share: the domain and
// xh_venv_record_obs's checks and addressing of the STATE view's rows
int table_rows(const xh_venv *v, const char *what, const int32_t *rows_dev,
               long first, long count, xh::VenvTabRowArgs *a) {
  CHK(table_domain(v->items, v->env.D, &a->m));
  if (!v->rec[XH_VREC_BINS].ptr)
    return fail(XH_ERR_STATE, "%s: %s", what,
                v->rec_steps > 0 ? "the record was made without states "
                                   "(xh_venv_set_record's with_states)"
                                 : "no record (xh_venv_set_record)");
  if (first < 0 || count < 0)
    return fail(XH_ERR_INVALID, "%s: first %ld, count %ld", what, first, count);
  const long P = v->rec_pos;
  const long total = (P + 1) * (long)v->N;
  if (count > 0 && !rows_dev && first + count > total)
    return fail(XH_ERR_INVALID, "%s: rows %ld .. %ld of %ld (cursor %ld, %d "
                "envs)", what, first, first + count - 1, total, P, v->N);
  a->B = v->env.B;
  a->D = v->env.D;
  a->N = v->N;
  a->P = (int)P;
  a->rec_bins = v->rec_as<const int8_t>(XH_VREC_BINS);
  a->rec_items = v->rec_as<const int8_t>(XH_VREC_ITEMS);
  a->cur_bins = (const int8_t *)v->buf[XH_VENV_BINS];
  a->cur_items = (const int8_t *)v->buf[XH_VENV_ITEMS];
  a->rows = rows_dev;
  a->first = first;
  a->count = count;
  a->err = v->err;
  return XH_OK;
}

}  // namespace

// xh_host.h: xh_venv_record_obs's checks and row addressing, for it and for the
// nets that read the record themselves (net_api.cpp)
int xh::host::venv_record_rows(xh_venv *v, const char *who, int view,
                               const int32_t *rows_dev, long first, long count,
                               xh::VenvObsArgs *a, const int32_t **cap,
                               xh_ctx **ctx) {
  if (!v) return fail(XH_ERR_INVALID, "%s: null venv", who);
  if (view != XH_VOBS_STATE && view != XH_VOBS_NEXT)
    return fail(XH_ERR_INVALID, "%s: view %d (XH_VOBS_STATE / NEXT)", who, view);
  if (!v->rec[XH_VREC_BINS].ptr)
    return fail(XH_ERR_STATE, "%s: %s", who,
                v->rec_steps > 0 ? "the record was made without states "
                                   "(xh_venv_set_record's with_states)"
                                 : "no record (xh_venv_set_record)");
  if (first < 0 || count < 0)
    return fail(XH_ERR_INVALID, "%s: first %ld, count %ld", who, first, count);
  if (cap) *cap = v->table.cap;
  if (ctx) *ctx = v->ctx;
  a->B = v->env.B;
  a->D = v->env.D;
  a->N = v->N;
  a->count = 0;
  if (count == 0) return XH_OK;
  const long P = v->rec_pos;
  const long total = (view == XH_VOBS_NEXT ? P : P + 1) * (long)v->N;
  if (total == 0 || (!rows_dev && first + count > total))
    return fail(XH_ERR_INVALID, "%s: rows %ld .. %ld of %ld (cursor %ld, %d "
                "envs)", who, first, first + count - 1, total, P, v->N);
  a->P = (int)P;
  a->next = view == XH_VOBS_NEXT;
  a->rec_bins = v->rec_as<const int8_t>(XH_VREC_BINS);
  a->rec_items = v->rec_as<const int8_t>(XH_VREC_ITEMS);
  a->cur_bins = (const int8_t *)v->buf[XH_VENV_BINS];
  a->cur_items = (const int8_t *)v->buf[XH_VENV_ITEMS];
  a->rec_action = v->rec_as<const int32_t>(XH_VREC_ACTION);
  a->rec_done = v->rec_as<const uint8_t>(XH_VREC_DONE);
  a->rows = rows_dev;
  a->first = first;
  a->count = count;
  a->err = v->err;
  return XH_OK;
}

extern "C" {

void xh_item_set_default(xh_item_set *s, int dims) {
  if (!s) return;
  *s = xh_item_set{};
  if (dims < 1 || dims > 3) return;
  const xh::EnvDesc env = make_env(8, dims);
  s->num_items = 2;
  for (int d = 0; d < dims; ++d) {
    s->capacity[d] = kBinCapacity;
    s->item[0][d] = env.item_a[d];
    s->item[1][d] = env.item_b[d];
  }
  s->weight[0] = env.p_a;
  s->weight[1] = 0.6;
}

int xh_item_set_thresholds(const xh_item_set *s, int dims, double *out) {
  return guard([&]() -> int {
    if (!out) return fail(XH_ERR_INVALID, "item set: null out");
    CHK(item_set_check(s, dims));
    item_set_thresholds(*s, out);
    return XH_OK;
  });
}

int xh_venv_create(xh_ctx *ctx, int num_envs, int bins, int dims,
                   uint32_t rng_state, int env_offset, int num_envs_global,
                   int policy_draws, xh_venv **out) {
  return xh_venv_create_ex(ctx, num_envs, bins, dims, rng_state, env_offset,
                           num_envs_global, policy_draws, nullptr, out);
}

int xh_venv_create_ex(xh_ctx *ctx, int num_envs, int bins, int dims,
                      uint32_t rng_state, int env_offset, int num_envs_global,
                      int policy_draws, const xh_item_set *items,
                      xh_venv **out) {
  return guard([&]() -> int {
    if (!ctx || !out) return fail(XH_ERR_INVALID, "null arg");
    if (!xh::venv_shape_supported(bins, dims))
      return fail(XH_ERR_INVALID, "venv: bins %d (8/16/32/64/128), dims %d "
                  "(1..3)", bins, dims);
    if (num_envs < 1 || env_offset < 0 || num_envs_global < num_envs ||
        env_offset + num_envs > num_envs_global)
      return fail(XH_ERR_INVALID, "venv: envs %d at offset %d of %d", num_envs,
                  env_offset, num_envs_global);
    if (policy_draws < 0 || policy_draws > 64)
      return fail(XH_ERR_INVALID, "venv: policy_draws %d", policy_draws);
    if (items) CHK(item_set_check(items, dims));
    HIPCHK(hipSetDevice(ctx->device));
    auto *v = new xh_venv;
    v->ctx = ctx;
    v->env = make_env(bins, dims);
    if (items) {
      v->general = true;
      v->items = item_set_clean(*items, dims);
      v->table = item_set_table(v->items, dims);
    } else {
      xh_item_set_default(&v->items, dims);
      // the table calls run the general kernels on the default set
      v->table = item_set_table(v->items, dims);
    }
    v->N = num_envs;
    v->Ng = num_envs_global;
    v->offset = env_offset;
    v->policy_draws = policy_draws;
    const uint64_t k = (uint64_t)policy_draws + 2;
    v->skip_mul = mstd_pow((uint64_t)policy_draws);
    v->jump_mul = mstd_pow(k * (uint64_t)(num_envs_global - 1));
    const size_t N = (size_t)num_envs, BD = (size_t)bins * dims;
    const size_t sz[XH_VENV_BUF_COUNT] = {N * 4, N * 4, N, N * BD, N * 4, N * 4,
                                          N * BD * 2 * 4, N,
                                          N * (size_t)bins * 4, N * 4};
    int st = XH_OK;
    for (int b = 0; b < XH_VENV_BUF_COUNT && st == XH_OK; ++b) {
      v->bytes[b] = sz[b];
      // xh_venv_act's buffers at their first use (venv_ensure)
      if (b == XH_VENV_POLICY || b == XH_VENV_PCHOICE) continue;
      st = dev_zalloc(ctx->stream, &v->buf[b], sz[b], "venv");
    }
    if (st == XH_OK && (hipMalloc((void **)&v->err, 4) != hipSuccess ||
                        hipMemsetAsync(v->err, 0, 4, ctx->stream) != hipSuccess))
      st = fail(XH_ERR_HIP, "venv: error flag");
    if (st == XH_OK) {
      uint32_t x0 = rng_state % 2147483647u;
      const hipError_t e = xh::launch_venv_init(v->args(), x0 ? x0 : 1u,
                                                env_offset, num_envs_global,
                                                (int)k, ctx->stream, v->tab());
      if (e != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        st = fail(XH_ERR_HIP, "venv init: %s", hipGetErrorString(e));
    }
    v->counted = true;
    ++ctx->trainers;
    if (st != XH_OK) return fail_after(st, [&] { xh_venv_destroy(v); });
    *out = v;
    return XH_OK;
  });
}

int xh_venv_set_item_set(xh_venv *v, const xh_item_set *s) {
  return venv_call(v, [&]() -> int {
    const int D = v->env.D;
    CHK(item_set_check(s, D));
    for (int d = 0; d < D; ++d)
      if (s->capacity[d] != v->items.capacity[d])
        return fail(XH_ERR_INVALID, "venv item set: capacity %d of dim %d, the "
                    "venv's is %d (the stored bins are in its units)",
                    s->capacity[d], d, v->items.capacity[d]);
    // the table goes with each launch's arguments: the launches already on
    // the stream keep theirs, the next one draws from this set
    v->items = item_set_clean(*s, D);
    v->table = item_set_table(v->items, D);
    v->general = true;
    return XH_OK;
  });
}

int xh_venv_get_item_set(const xh_venv *v, xh_item_set *out) {
  return guard([&]() -> int {
    if (!v || !out) return fail(XH_ERR_INVALID, "null arg");
    *out = v->items;
    return XH_OK;
  });
}

int xh_venv_destroy(xh_venv *v) {
  return guard([&]() -> int {
    if (!v) return XH_OK;
    (void)hipSetDevice(v->ctx->device);
    (void)hipStreamSynchronize(v->ctx->stream);
    venv_drop_events(v);
    for (hipEvent_t e : v->event_pool) (void)hipEventDestroy(e);
    for (void *p : v->buf)
      if (p) (void)hipFree(p);
    if (v->err) (void)hipFree(v->err);
    if (v->end_scratch) (void)hipFree(v->end_scratch);
    if (v->adv_part) (void)hipFree(v->adv_part);  // adv_stats, adv_end_part too
    if (v->loss_part) (void)hipFree(v->loss_part);
    if (v->kl_part) (void)hipFree(v->kl_part);
    if (v->ext_part) (void)hipFree(v->ext_part);
    if (v->tab_scratch) (void)hipFree(v->tab_scratch);
    if (v->legal_buf) (void)hipFree(v->legal_buf);
    venv_free_episode_stats(v);
    venv_free_record(v);
    xh_ctx *c = v->ctx;
    const bool counted = v->counted;
    delete v;
    ctx_release(c, counted);
    return XH_OK;
  });
}

size_t xh_venv_bytes(const xh_venv *v, int which) {
  return v && which >= 0 && which < XH_VENV_BUF_COUNT ? v->bytes[which] : 0;
}

void *xh_venv_device_ptr(xh_venv *v, int which) {
  if (!v || which < 0 || which >= XH_VENV_BUF_COUNT) return nullptr;
  guard([&] { return venv_ensure(v, which); });
  return v->buf[which];
}

int xh_venv_get(xh_venv *v, int which, void *host, size_t bytes) {
  return guard([&]() -> int {
    CHK(venv_check_buffer(v, which, host, bytes));
    HIPCHK(hipSetDevice(v->ctx->device));
    if (const int st = venv_ensure(v, which)) return st;
    HIPCHK(copy_to_host(host, v->buf[which], bytes, v->ctx->stream));
    return venv_check_err(v);
  });
}

int xh_venv_set(xh_venv *v, int which, const void *host, size_t bytes) {
  return guard([&]() -> int {
    CHK(venv_check_buffer(v, which, host, bytes));
    if (which == XH_VENV_ACTIONS) {
      const int32_t *a = static_cast<const int32_t *>(host);
      for (int i = 0; i < v->N; ++i)
        if (a[i] < 0 || a[i] >= v->env.B)
          return fail(XH_ERR_INVALID, "venv: action %d of env %d outside "
                      "[0, %d)", a[i], i, v->env.B);
    }
    if (which == XH_VENV_BINS) {
      const int8_t *b = static_cast<const int8_t *>(host);
      // any int8 value up to the capacity: the venv computes in int / f32
      // (an apply to a game-over env keeps subtracting, bin_packing.h:53-63)
      for (size_t i = 0; i < bytes; ++i)
        if (b[i] > v->items.capacity[i % v->env.D])
          return fail(XH_ERR_INVALID, "venv: bin value %d above the capacity %d",
                      b[i], v->items.capacity[i % v->env.D]);
    }
    HIPCHK(hipSetDevice(v->ctx->device));
    if (const int st = venv_ensure(v, which)) return st;
    HIPCHK(copy_to_device(v->buf[which], host, bytes, v->ctx->stream));
    // new bins are new episodes: every running length restarts
    if (which == XH_VENV_BINS && v->ep.ring.history)
      HIPCHK(hipMemsetAsync(v->ep.state[XH_VEPS_RUNNING], 0, (size_t)v->N * 4,
                            v->ctx->stream));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    return XH_OK;
  });
}

int xh_venv_step(xh_venv *v, int write_obs) {
  return venv_call(v, [&] {
    return venv_launch(v, xh::kVenvStep, 1, false, write_obs != 0);
  });
}

int xh_venv_apply(xh_venv *v, int use_mask) {
  return venv_call(v, [&] {
    return venv_launch(v, xh::kVenvStep, 0, use_mask != 0, false);
  });
}

int xh_venv_reset(xh_venv *v, int use_mask) {
  return venv_call(v, [&] {
    return venv_launch(v, xh::kVenvReset, 0, use_mask != 0, false);
  });
}

int xh_venv_observe(xh_venv *v) {
  return venv_call(
      v, [&] { return venv_launch(v, xh::kVenvObserve, 0, false, true); });
}

int xh_venv_act(xh_venv *v, const float *policy_dev, int kind, int mode,
                int write_obs) {
  return venv_call(v, [&]() -> int {
    if (kind != XH_ACT_PROBS && kind != XH_ACT_LOGITS)
      return fail(XH_ERR_INVALID, "venv act: kind %d (XH_ACT_PROBS / LOGITS)",
                  kind);
    if (mode != XH_ACT_SAMPLE && mode != XH_ACT_ARGMAX)
      return fail(XH_ERR_INVALID, "venv act: mode %d (XH_ACT_SAMPLE / ARGMAX)",
                  mode);
    if (mode == XH_ACT_SAMPLE && v->policy_draws != 2)
      return fail(XH_ERR_INVALID, "venv act: sampling takes two draws per env "
                  "and step, the venv was created with policy_draws %d",
                  v->policy_draws);
    if (reinterpret_cast<uintptr_t>(policy_dev) & 15)
      return fail(XH_ERR_INVALID, "venv act: the policy rows must be 16-byte "
                  "aligned (the kernel reads them as 16-byte loads)");
    CHK(venv_act_ready(v, "venv act"));
    if (!policy_dev)
      if (const int st = venv_ensure(v, XH_VENV_POLICY)) return st;
    xh::VenvActArgs a = venv_act_args(v, write_obs != 0);
    a.policy = policy_dev ? policy_dev : (const float *)v->buf[XH_VENV_POLICY];
    a.logits = kind == XH_ACT_LOGITS;
    a.argmax = mode == XH_ACT_ARGMAX;
    a.rec_distrib = v->rec_as<float>(kRecDistrib);
    return venv_act_done(v, venv_timed(v, [&] {
      return xh::launch_venv_act(a, v->ctx->stream, v->tab());
    }));
  });
}

int xh_venv_act_heuristic(xh_venv *v, int heuristic, int write_obs) {
  return venv_call(v, [&]() -> int {
    if (heuristic != XH_HEUR_RANDOM && heuristic != XH_HEUR_FIRSTFIT &&
        heuristic != XH_HEUR_BESTFIT && heuristic != XH_HEUR_MINWASTE)
      return fail(XH_ERR_INVALID, "venv act heuristic: heuristic %d "
                  "(XH_HEUR_RANDOM / FIRSTFIT / BESTFIT / MINWASTE)",
                  heuristic);
    if (heuristic == XH_HEUR_RANDOM && v->policy_draws != 2)
      return fail(XH_ERR_INVALID, "venv act heuristic: the random pick takes "
                  "two draws per env and step, the venv was created with "
                  "policy_draws %d", v->policy_draws);
    if (v->rec[kRecDistrib].ptr)
      return fail(XH_ERR_STATE, "venv act heuristic: the distribution record "
                  "is on and a heuristic has no distribution to record "
                  "(xh_venv_set_record_distrib(v, 0))");
    CHK(venv_act_ready(v, "venv act heuristic"));
    xh::VenvHeurArgs h{};
    h.a = venv_act_args(v, write_obs != 0);
    h.heur = heuristic;
    return venv_act_done(v, venv_timed(v, [&] {
      return xh::launch_venv_heur(h, v->ctx->stream, v->tab());
    }));
  });
}

int xh_venv_set_record(xh_venv *v, int steps, int with_states) {
  return venv_call(v, [&]() -> int {
    if (steps < 0) return fail(XH_ERR_INVALID, "venv record: steps %d", steps);
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    venv_free_record(v);
    if (steps == 0) return XH_OK;
    const size_t TN = (size_t)steps * v->N;
    const size_t BD = (size_t)v->env.B * v->env.D;
    const size_t sz[XH_VREC_COUNT] = {TN * 4, TN * 4, TN * 4, TN,
                                      with_states ? TN * BD : 0,
                                      with_states ? TN * 4 : 0};
    v->rec_steps = steps;
    int st = XH_OK;
    for (int w = 0; w < XH_VREC_COUNT && st == XH_OK; ++w)
      if (sz[w]) st = rec_alloc(v, w, sz[w], "venv record");
    if (st == XH_OK && v->mask_on) st = rec_alloc_legal(v);
    // a failure in the middle leaves no record
    if (st != XH_OK) return fail_after(st, [&] { venv_free_record(v); });
    return XH_OK;
  });
}

int xh_venv_record_pos(xh_venv *v, int *pos) {
  return guard([&]() -> int {
    if (!v || !pos) return fail(XH_ERR_INVALID, "null arg");
    *pos = v->rec_pos;
    return XH_OK;
  });
}

int xh_venv_record_rewind(xh_venv *v) {
  return venv_call(v, [&]() -> int {
    v->rec_pos = 0;
    return XH_OK;
  });
}

size_t xh_venv_record_bytes(const xh_venv *v, int which) {
  return vrec_which(which) ? rec_bytes(v, which) : 0;
}

void *xh_venv_record_ptr(xh_venv *v, int which) {
  return vrec_which(which) ? rec_ptr(v, which) : nullptr;
}

int xh_venv_get_record(xh_venv *v, int which, void *host, size_t bytes) {
  char what[32];
  std::snprintf(what, sizeof what, "venv record %d", which);
  return rec_to_host(v, vrec_which(which) ? which : -1, host, bytes, what);
}

int xh_venv_set_record_distrib(xh_venv *v, int on) {
  return venv_call(v, [&]() -> int {
    HIPCHK(hipSetDevice(v->ctx->device));
    if (!on) return rec_drop(v, kRecDistrib);
    if (v->rec_steps <= 0)
      return fail(XH_ERR_STATE, "venv record distrib: no record "
                  "(xh_venv_set_record)");
    if (v->rec_pos != 0)
      return fail(XH_ERR_STATE, "venv record distrib: the cursor is at %d; "
                  "turn it on at cursor 0 (xh_venv_record_rewind), so every "
                  "recorded slot has its distribution", v->rec_pos);
    if (v->rec[kRecDistrib].ptr) return XH_OK;
    return rec_alloc(v, kRecDistrib,
                     (size_t)v->rec_steps * v->N * v->env.B * 4,
                     "venv record distrib");
  });
}

size_t xh_venv_record_distrib_bytes(const xh_venv *v) {
  return rec_bytes(v, kRecDistrib);
}

float *xh_venv_record_distrib_ptr(xh_venv *v) {
  return static_cast<float *>(rec_ptr(v, kRecDistrib));
}

int xh_venv_get_record_distrib(xh_venv *v, float *host, size_t bytes) {
  return rec_to_host(v, kRecDistrib, host, bytes, "venv record distrib");
}

// ---- invalid-action masking (venv_legal_kernel, venv_act_kernel's MASK) ----
int xh_venv_legal_words(const xh_venv *v) {
  return v ? xh::venv_legal_words(v->env.B) : 0;
}

int xh_venv_set_action_mask(xh_venv *v, int on) {
  return venv_call(v, [&]() -> int {
    HIPCHK(hipSetDevice(v->ctx->device));
    if (!on) {
      CHK(rec_drop(v, kRecLegal));
      v->mask_on = false;
      return XH_OK;
    }
    if (v->rec_steps > 0 && v->rec_pos != 0)
      return fail(XH_ERR_STATE, "venv action mask: the record's cursor is at "
                  "%d; turn it on at cursor 0 (xh_venv_record_rewind), so "
                  "every recorded slot has its legal words", v->rec_pos);
    if (v->rec_steps > 0 && !v->rec[kRecLegal].ptr) CHK(rec_alloc_legal(v));
    v->mask_on = true;
    return XH_OK;
  });
}

int xh_venv_legal(xh_venv *v, uint32_t *out_dev) {
  return venv_call(v, [&]() -> int {
    const int W = xh::venv_legal_words(v->env.B);
    if (reinterpret_cast<uintptr_t>(out_dev) & (uintptr_t)(4 * W - 1))
      return fail(XH_ERR_INVALID, "venv legal: out_dev must be %d-byte aligned "
                  "(the kernel stores an env's words as one piece)", 4 * W);
    HIPCHK(hipSetDevice(v->ctx->device));
    if (!out_dev)
      if (const int st = venv_ensure_legal_buf(v)) return st;
    uint32_t *out = out_dev ? out_dev : v->legal_buf;
    const xh::VenvArgs a = v->args();
    return venv_timed(
        v, [&] { return xh::launch_venv_legal(a, out, v->ctx->stream); });
  });
}

uint32_t *xh_venv_legal_ptr(xh_venv *v) {
  if (!v) return nullptr;
  guard([&] { return venv_ensure_legal_buf(v); });
  return v->legal_buf;
}

size_t xh_venv_record_legal_bytes(const xh_venv *v) {
  return rec_bytes(v, kRecLegal);
}

uint32_t *xh_venv_record_legal_ptr(xh_venv *v) {
  return static_cast<uint32_t *>(rec_ptr(v, kRecLegal));
}

int xh_venv_get_record_legal(xh_venv *v, uint32_t *host, size_t bytes) {
  return rec_to_host(v, kRecLegal, host, bytes, "venv record legal");
}

// ---- the learner's side of a recorded window (venv_learn_kernels.hip) ----
int xh_venv_record_obs(xh_venv *v, int view, const int32_t *rows_dev,
                       long first, long count, float *obs_dev) {
  return venv_call(v, [&]() -> int {
    xh::VenvObsArgs a{};
    CHK(venv_record_rows(v, "venv record obs", view, rows_dev, first, count, &a,
                         nullptr, nullptr));
    if (count == 0) return XH_OK;
    if (!obs_dev || (reinterpret_cast<uintptr_t>(obs_dev) & 15))
      return fail(XH_ERR_INVALID, "venv record obs: obs_dev must be 16-byte "
                  "aligned (the kernel writes 16-byte stores)");
    HIPCHK(hipSetDevice(v->ctx->device));
    a.obs = obs_dev;
    return venv_timed(v, [&] {
      return xh::launch_venv_record_obs(a, v->ctx->stream,
                                        v->general ? v->table.cap : nullptr);
    });
  });
}

int xh_venv_record_ends(xh_venv *v, int32_t *list_dev, int32_t *n_dev) {
  return guard([&]() -> int {
    if (!v || !list_dev || !n_dev) return fail(XH_ERR_INVALID, "null arg");
    if (v->rec_steps <= 0)
      return fail(XH_ERR_STATE, "venv record ends: no record "
                  "(xh_venv_set_record)");
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    if (v->rec_pos == 0) {  // nothing recorded: an empty list
      HIPCHK(hipMemsetAsync(n_dev, 0, 4, s));
      return XH_OK;
    }
    const int ns = xh::end_list_scratch_ints(v->N);
    if (!v->end_scratch)
      HIPCHK(hipMalloc((void **)&v->end_scratch, (size_t)(ns + 1) * 4));
    xh::EndListArgs ea{v->rec_as<const uint8_t>(XH_VREC_DONE), v->N, v->rec_pos,
                       list_dev, n_dev, v->end_scratch + ns, nullptr, 0};
    return venv_timed(
        v, [&] { return xh::launch_end_list(ea, v->end_scratch, s); });
  });
}

int xh_venv_advantages(xh_venv *v, const xh_venv_adv *p) {
  return guard([&]() -> int {
    if (!v || !p) return fail(XH_ERR_INVALID, "null arg");
    if (p->steps < 0)
      return fail(XH_ERR_INVALID, "venv advantages: steps %d", p->steps);
    if (!p->values || !p->adv)
      return fail(XH_ERR_INVALID, "venv advantages: null values / adv");
    xh::VenvGaeArgs a{};
    a.N = v->N;
    a.T = p->steps;
    a.reward = p->reward;
    a.done = p->done;
    if (p->steps == 0) {  // the record's window
      if (v->rec_steps <= 0)
        return fail(XH_ERR_STATE, "venv advantages: steps 0 takes the "
                    "record's window and there is no record "
                    "(xh_venv_set_record)");
      a.T = v->rec_pos;
      if (!a.reward) a.reward = v->rec_as<const float>(XH_VREC_REWARD);
      if (!a.done) a.done = v->rec_as<const uint8_t>(XH_VREC_DONE);
    } else if (!a.reward || !a.done) {
      return fail(XH_ERR_INVALID, "venv advantages: a window of %d steps of "
                  "the caller's own needs reward and done", p->steps);
    }
    if (a.T == 0)
      return fail(XH_ERR_STATE, "venv advantages: the record is empty");
    a.values = p->values;
    a.v_term = p->v_term;
    a.gamma = p->gamma;
    a.lambda = p->lambda;
    a.adv = p->adv;
    a.td_target = p->td_target;
    a.lambda_return = p->lambda_return;
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    const int grid = xh::venv_gae_grid(v->N);
    const bool sums = p->normalize || p->stats;
    if (sums && !v->adv_part) {  // partials, stats [4], ended-row counts
      HIPCHK(hipMalloc((void **)&v->adv_part,
                       (size_t)grid * 16 + 32 + (size_t)grid * 4));
      v->adv_stats = v->adv_part + 2 * (size_t)grid;
      v->adv_end_part = reinterpret_cast<int *>(v->adv_stats + 4);
    }
    if (sums) {
      a.part = v->adv_part;
      a.end_part = v->adv_end_part;
    }
    CHK(venv_timed(v, [&] { return xh::launch_venv_gae(a, s); }));
    if (!sums) return XH_OK;
    const double rows = (double)a.T * (double)v->N;
    hipError_t e = xh::launch_adv_stats(v->adv_part, grid, v->adv_stats, s);
    if (e == hipSuccess)
      e = xh::launch_venv_adv_counts(v->adv_end_part, grid, rows, v->adv_stats,
                                     s);
    if (e == hipSuccess && p->normalize)
      e = xh::launch_adv_normalize(p->adv, (long)a.T * v->N, v->adv_stats, rows,
                                   s);
    if (e != hipSuccess)
      return fail(XH_ERR_HIP, "venv advantages: %s", hipGetErrorString(e));
    if (p->stats)
      HIPCHK(hipMemcpyAsync(p->stats, v->adv_stats, 32,
                            hipMemcpyDeviceToDevice, s));
    return XH_OK;
  });
}

int xh_venv_policy_loss(xh_venv *v, const xh_venv_loss *p) {
  return venv_policy_loss(v, p, false, nullptr);
}

int xh_venv_policy_loss_masked(xh_venv *v, const xh_venv_loss *p,
                               const uint32_t *legal_dev) {
  return venv_policy_loss(v, p, true, legal_dev);
}

int xh_venv_policy_loss_ex(xh_venv *v, const xh_venv_loss *p,
                           const xh_venv_loss_ext *x) {
  return venv_policy_loss(v, p, false, nullptr, x);
}

int xh_venv_kl_beta(xh_venv *v, const double *kl_stats_dev, float d_targ,
                    float *beta_dev, float *log_dev) {
  return guard([&]() -> int {
    if (!v || !kl_stats_dev || !beta_dev)
      return fail(XH_ERR_INVALID, "venv kl beta: null venv / kl_stats_dev / "
                  "beta_dev");
    if (!(d_targ > 0.0f && std::isfinite(d_targ)))
      return fail(XH_ERR_INVALID, "venv kl beta: d_targ %g", (double)d_targ);
    HIPCHK(hipSetDevice(v->ctx->device));
    // kl_stats' first two entries are KL_SUM and ROWS: kl_beta_kernel's input
    static_assert(XH_VKL_KL_SUM == 0 && XH_VKL_ROWS == 1, "kl_beta_kernel");
    const hipError_t e = xh::launch_kl_beta_update(kl_stats_dev, beta_dev,
                                                   d_targ, log_dev,
                                                   v->ctx->stream);
    if (e != hipSuccess)
      return fail(XH_ERR_HIP, "venv kl beta: %s", hipGetErrorString(e));
    return XH_OK;
  });
}

// ---- logit tables (venv_table_kernels.hip, xh_venv_table.h) ----
int xh_item_set_table_info(const xh_item_set *s, int dims, int bins,
                           struct xh_venv_table_info *out) {
  return guard([&]() -> int {
    if (!out) return fail(XH_ERR_INVALID, "venv table: null out");
    CHK(item_set_check(s, dims));
    if (!xh::venv_shape_supported(bins, dims))
      return fail(XH_ERR_INVALID, "venv table: bins %d (8/16/32/64/128), dims "
                  "%d (1..3)", bins, dims);
    xh::VenvTabDomain m;
    CHK(table_domain(*s, dims, &m));
    table_info(m, bins, out);
    return XH_OK;
  });
}

int xh_venv_table_info(const xh_venv *v, struct xh_venv_table_info *out) {
  return guard([&]() -> int {
    if (!v || !out) return fail(XH_ERR_INVALID, "null arg");
    xh::VenvTabDomain m;
    CHK(table_domain(v->items, v->env.D, &m));
    table_info(m, v->env.B, out);
    return XH_OK;
  });
}

int xh_venv_table_obs(xh_venv *v, float *obs_dev) {
  return venv_call(v, [&]() -> int {
    xh::VenvTabDomain m;
    CHK(table_domain(v->items, v->env.D, &m));
    if (!obs_dev || (reinterpret_cast<uintptr_t>(obs_dev) & 15))
      return fail(XH_ERR_INVALID, "venv table obs: obs_dev must be 16-byte "
                  "aligned");
    HIPCHK(hipSetDevice(v->ctx->device));
    const long total = xh::vt::rows(m.entries, v->env.B) * v->env.B;
    return venv_timed(v, [&] {
      return xh::launch_venv_table_obs(m, v->table, total, obs_dev,
                                       v->ctx->stream);
    });
  });
}

int xh_venv_act_table(xh_venv *v, const float *table_dev, int mode,
                      int write_obs) {
  return venv_call(v, [&]() -> int {
    xh::VenvTabActArgs h{};
    CHK(table_domain(v->items, v->env.D, &h.m));
    if (mode != XH_ACT_SAMPLE && mode != XH_ACT_ARGMAX)
      return fail(XH_ERR_INVALID, "venv act table: mode %d (XH_ACT_SAMPLE / "
                  "ARGMAX)", mode);
    if (mode == XH_ACT_SAMPLE && v->policy_draws != 2)
      return fail(XH_ERR_INVALID, "venv act table: sampling takes two draws "
                  "per env and step, the venv was created with policy_draws %d",
                  v->policy_draws);
    if (!table_dev || (reinterpret_cast<uintptr_t>(table_dev) & 3))
      return fail(XH_ERR_INVALID, "venv act table: table_dev must be a 4-byte "
                  "aligned device pointer to %ld floats", h.m.entries);
    CHK(venv_act_ready(v, "venv act table"));
    h.a = venv_act_args(v, write_obs != 0);
    h.a.logits = 1;
    h.a.argmax = mode == XH_ACT_ARGMAX;
    h.a.rec_distrib = v->rec_as<float>(kRecDistrib);
    h.table = table_dev;
    return venv_act_done(v, venv_timed(v, [&] {
      return xh::launch_venv_act_table(h, v->ctx->stream, v->table);
    }));
  });
}

int xh_venv_table_gather(xh_venv *v, const float *table_dev,
                         const int32_t *rows_dev, long first, long count,
                         float *out_dev) {
  return venv_call(v, [&]() -> int {
    xh::VenvTabRowArgs a{};
    CHK(table_rows(v, "venv table gather", rows_dev, first, count, &a));
    if (!table_dev || (reinterpret_cast<uintptr_t>(table_dev) & 3))
      return fail(XH_ERR_INVALID, "venv table gather: table_dev must be a "
                  "4-byte aligned device pointer to %ld floats", a.m.entries);
    if (count == 0) return XH_OK;
    if (!out_dev || (reinterpret_cast<uintptr_t>(out_dev) & 15))
      return fail(XH_ERR_INVALID, "venv table gather: out_dev must be 16-byte "
                  "aligned (the kernel writes 16-byte stores)");
    HIPCHK(hipSetDevice(v->ctx->device));
    a.table = table_dev;
    a.out = out_dev;
    return venv_timed(v, [&] {
      return xh::launch_venv_table_gather(a, v->ctx->stream, v->table);
    });
  });
}

int xh_venv_table_grad(xh_venv *v, const int32_t *rows_dev, long first,
                       long count, const float *dout_dev, float *g_dev,
                       int accumulate) {
  return venv_call(v, [&]() -> int {
    xh::VenvTabRowArgs a{};
    CHK(table_rows(v, "venv table grad", rows_dev, first, count, &a));
    if (!g_dev || (reinterpret_cast<uintptr_t>(g_dev) & 15))
      return fail(XH_ERR_INVALID, "venv table grad: g_dev must be 16-byte "
                  "aligned");
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    const long total = xh::vt::rows(a.m.entries, v->env.B) * v->env.B;
    if (count == 0) {  // no addends: G = 0
      if (!accumulate) HIPCHK(hipMemsetAsync(g_dev, 0, (size_t)total * 4, s));
      return XH_OK;
    }
    if (!dout_dev || (reinterpret_cast<uintptr_t>(dout_dev) & 15))
      return fail(XH_ERR_INVALID, "venv table grad: dout_dev must be 16-byte "
                  "aligned (the kernel reads 16-byte pieces)");
    if (!v->tab_scratch)
      HIPCHK(hipMalloc(&v->tab_scratch, 16 + (size_t)XH_VTAB_MAX_ENTRIES * 8));
    HIPCHK(hipMemsetAsync(v->tab_scratch, 0, 16 + (size_t)a.m.entries * 8, s));
    a.dout = dout_dev;
    a.maxbits = static_cast<uint32_t *>(v->tab_scratch);
    a.acc = reinterpret_cast<unsigned long long *>(
        static_cast<char *>(v->tab_scratch) + 16);
    return venv_timed(v, [&] {
      return xh::launch_venv_table_grad(a, total, accumulate != 0, g_dev, s,
                                        v->table);
    });
  });
}

int xh_venv_set_timing(xh_venv *v, int on) {
  return venv_call(v, [&]() -> int {
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    venv_drop_events(v);
    v->timing = on != 0;
    return XH_OK;
  });
}

int xh_venv_kernel_time(xh_venv *v, double *ms, long *launches) {
  return guard([&]() -> int {
    if (!v || !ms || !launches) return fail(XH_ERR_INVALID, "null arg");
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    double total = 0;
    for (auto &ev : v->events) {
      float e = 0;
      HIPCHK(hipEventElapsedTime(&e, ev.first, ev.second));
      total += e;
    }
    *ms = total;
    *launches = (long)v->events.size();
    return XH_OK;
  });
}

// ---- episode statistics (venv_episode_kernels.hip) ----
int xh_venv_set_episode_stats(xh_venv *v, int history_rows) {
  return venv_call(v, [&]() -> int {
    if (history_rows < 0 || history_rows > kMaxEpisodeRows)
      return fail(XH_ERR_INVALID, "venv episode stats: history_rows %d not in "
                  "[0, %d]", history_rows, kMaxEpisodeRows);
    HIPCHK(hipSetDevice(v->ctx->device));
    hipStream_t s = v->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));
    venv_free_episode_stats(v);
    if (history_rows == 0) return XH_OK;
    auto &ep = v->ep;
    const size_t N = (size_t)v->N, grid = (size_t)xh::venv_ep_grid(v->N);
    const size_t ring = (size_t)history_rows * XH_VEP_COUNT * 8;
    hipError_t e = hipSuccess;
    for (int32_t *&p : ep.state)
      if (e == hipSuccess) e = hipMalloc((void **)&p, N * 4);
    if (e == hipSuccess)
      e = hipMalloc((void **)&ep.acc, N * sizeof(xh::VenvEpAcc));
    if (e == hipSuccess)
      e = hipMalloc((void **)&ep.psum, grid * xh::kVepSums * 8);
    if (e == hipSuccess)
      e = hipMalloc((void **)&ep.pext, grid * xh::kVepExts * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ep.ring.dev, ring);
    // unwritten rows read as NaN (all-ones bytes)
    if (e == hipSuccess) e = hipMemsetAsync(ep.ring.dev, 0xFF, ring, s);
    if (e == hipSuccess)
      e = xh::launch_venv_ep_init(v->N, ep.state[XH_VEPS_RUNNING],
                                  ep.state[XH_VEPS_FIRST], ep.acc, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      venv_free_episode_stats(v);
      return fail(XH_ERR_HIP, "venv episode stats(%d): %s", history_rows,
                  hipGetErrorString(e));
    }
    ep.ring.history = history_rows;
    return XH_OK;
  });
}

int xh_venv_episode_row(xh_venv *v) {
  return venv_call(v, [&]() -> int {
    auto &ep = v->ep;
    if (!ep.ring.history)
      return fail(XH_ERR_STATE, "venv episode row: episode statistics are off "
                  "(xh_venv_set_episode_stats)");
    HIPCHK(hipSetDevice(v->ctx->device));
    double *row = ring_row(ep.ring, ep.ring.rows);
    CHK(venv_timed(v, [&] {
      return xh::launch_venv_ep_row(v->N, ep.state[XH_VEPS_RUNNING],
                                    ep.state[XH_VEPS_FIRST], ep.acc, ep.psum,
                                    ep.pext, (double)ep.ring.rows,
                                    (double)ep.calls, row, v->ctx->stream);
    }));
    ++ep.ring.rows;
    ep.calls = 0;
    return XH_OK;
  });
}

int xh_venv_episode_count(xh_venv *v, long *total_rows) {
  return guard([&]() -> int {
    if (!v || !total_rows) return fail(XH_ERR_INVALID, "null arg");
    if (!v->ep.ring.history)
      return fail(XH_ERR_STATE, "venv episode count: episode statistics are "
                  "off (xh_venv_set_episode_stats)");
    *total_rows = v->ep.ring.rows;
    return XH_OK;
  });
}

int xh_venv_get_episode_rows(xh_venv *v, long first, int count, double *out) {
  return guard([&]() -> int {
    if (!v || (count > 0 && !out)) return fail(XH_ERR_INVALID, "null arg");
    const auto &ep = v->ep;
    if (!ep.ring.history)
      return fail(XH_ERR_STATE, "venv episode rows: episode statistics are off "
                  "(xh_venv_set_episode_stats)");
    return ring_read(ep.ring, v->ctx, first, count, out, "venv episode rows");
  });
}

size_t xh_venv_episode_bytes(const xh_venv *v, int which) {
  return v && v->ep.ring.history && veps_which(which) ? (size_t)v->N * 4 : 0;
}

void *xh_venv_episode_ptr(xh_venv *v, int which) {
  return v && veps_which(which) ? v->ep.state[which] : nullptr;
}

int xh_venv_episode_get(xh_venv *v, int which, void *host, size_t bytes) {
  return guard([&]() -> int {
    CHK(venv_check_episode_array(v, which, host, bytes, "venv episode get"));
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(copy_to_host(host, v->ep.state[which], bytes, v->ctx->stream));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    return XH_OK;
  });
}

int xh_venv_episode_set(xh_venv *v, int which, const void *host,
                        size_t bytes) {
  return guard([&]() -> int {
    CHK(venv_check_episode_array(v, which, host, bytes, "venv episode set"));
    const int32_t *a = static_cast<const int32_t *>(host);
    for (int i = 0; i < v->N; ++i)
      if (a[i] < (which == XH_VEPS_FIRST ? -1 : 0))
        return fail(XH_ERR_INVALID, "venv episode set %d: %d at env %d", which,
                    a[i], i);
    HIPCHK(hipSetDevice(v->ctx->device));
    HIPCHK(copy_to_device(v->ep.state[which], host, bytes, v->ctx->stream));
    HIPCHK(hipStreamSynchronize(v->ctx->stream));
    return XH_OK;
  });
}

int xh_venv_synchronize(xh_venv *v) {
  return venv_call(v, [&]() -> int {
    HIPCHK(hipSetDevice(v->ctx->device));
    return venv_check_err(v);
  });
}

}  // extern "C"
