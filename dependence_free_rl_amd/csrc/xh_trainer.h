// xh_trainer.h -- the trainer behind the C ABI's xh_trainer handle, shared by
// the translation units that implement calls on it (xylo_hip.cpp: lifecycle,
// data accessors and the rollout; trainer_learn.cpp: learn() and the optimizer
// step; trainer_pg.cpp: REINFORCE; trainer_diag.cpp: the opt-in diagnostics;
// eval_api.cpp: the evaluators; phase_trace.cpp: the diagnostic build's
// phase trace; state_api.cpp: save / restore / digest), with the helpers and
// entry points they share.
#ifndef XH_TRAINER_H_
#define XH_TRAINER_H_

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/xylo_hip.h"
#include "xh_host.h"
#include "xh_kernels.h"

struct timed_event {
  std::string name;
  hipEvent_t start, stop;
};

struct xh_trainer {
  xh_ctx *ctx = nullptr;
  xh_config cfg{};
  xh::EnvDesc env{};
  xh::PolicyLayout pl{};
  xh::ValueLayout vl{};
  int np = 0, nv = 0;
  // trajectory batch
  int8_t *bins = nullptr, *items = nullptr;
  int32_t *action = nullptr, *forced = nullptr;
  float *pold = nullptr;
  uint8_t *done = nullptr;
  uint32_t *rng = nullptr;
  // parameters and learner buffers
  float *pp = nullptr, *vp = nullptr;
  float *v_state = nullptr, *v_state0 = nullptr, *v_term = nullptr;
  float *targets = nullptr, *adv = nullptr;
  float *row_g = nullptr;               // [T*N] dL/dV of the value step
  float *vact[2] = {nullptr, nullptr};  // value layer 1 / 2 outputs
  float *vgr[2] = {nullptr, nullptr};   // their dL/d(pre-activation)
  float *pslab = nullptr, *vslab = nullptr;
  float *vw0red = nullptr;  // value layer 0 on the reduced observation
  uint8_t *vw0frag = nullptr;  // W0's bf16 fragments (value_net_kernels.hip)
  // vw0frag holds the fragments of the current value parameters (set by a
  // bf16 value forward, cleared by every write of vp): the next iteration's
  // first forward then skips the preparation launch
  bool vfrag_ready = false;
  // PPO's epoch 0 on the rollout's forward outputs (DESIGN.md §3.0e;
  // policy_train_spec8_e0_kernel).  The buffers exist only for a trainer that
  // can use them (PPO, epochs >= 2, 64 bins 2-D [128,128], split kernels):
  // e0_mask [T][N] relu-mask records of 1 KB, e0_p [T][N][64] distributions
  // (qold itself where the trainer records them anyway).  e0_valid: they are
  // this window's forward outputs under the current policy parameters -- set
  // by a rollout that ran rollout_split_kernel over all T slots with both
  // outputs, cleared by wrote() on every write of the policy parameters and
  // every host write into the batch.
  uint32_t *e0_mask = nullptr;
  float *e0_p = nullptr;
  bool e0_valid = false;
  // the packed batch of the 64-bin 2-D [128,128] PPO / actor-critic epochs
  // (DESIGN.md §3.0e "duplicate rows", spec8_pack_layout.h), rebuilt by every
  // learn() that runs packed: the group records, the device header, the
  // pass's scratch (classes, per-chunk counts).  Null for any other trainer.
  // pk_learned: the header is the last learn()'s (xh_trainer_pack_stats).
  uint8_t *pk = nullptr, *pk_cls = nullptr;
  int *pk_hdr = nullptr, *pk_blk = nullptr;
  bool pk_learned = false;
  // the epoch on the table (spec8_table_layout.h), beside the
  // packed batch: the static table batch (written once, at creation), the
  // entries' logits, the per-entry sums G of the loss gradient with their
  // bound max |G|, the streaming pass's per-workgroup sums, and the count of
  // rows outside the table.  tab_learned: the last learn() ran its epochs on
  // the table (xh_trainer_table_stats).  The lean table kernels
  // (table_mm_kernels.hip; tiles: table_tile_layout.h) read neither the table
  // batch nor the bound; they keep the forward's H2 in tab_h2 and write their
  // slabs, one per tile whatever the train grid, to tab_slab.
  uint8_t *tab_pk = nullptr;
  float *tab_logits = nullptr, *tab_G = nullptr, *tab_gmax = nullptr;
  float *tab_h2 = nullptr, *tab_slab = nullptr;
  double *tab_part = nullptr;
  int *tab_ood = nullptr;
  bool tab_learned = false;
  int pslab_stride = 0, vslab_stride = 0, pslab_n = 0, vslab_n = 0;
  float *pgrads = nullptr, *vgrad = nullptr;
  float *logits = nullptr, *probs = nullptr;
  double *adv_part = nullptr, *adv_stats = nullptr;  // adv_normalize
  float *g_bound = nullptr;  // the learn()'s bound on the loss gradient g
  // KL-PPO state
  float *qold = nullptr, *beta = nullptr, *kl_log = nullptr;
  int *end_list = nullptr, *n_end = nullptr, *n_open = nullptr;
  int *vrows = nullptr;  // device: (T+1)N + n_end rows of the first V batch
  int *end_scratch = nullptr;  // launch_end_list_par's block totals
  double *kl_part = nullptr, *kl_sum = nullptr;
  // optimizers of the policy [0] and value [1] nets (nn.h:589-698)
  struct opt_state {
    int kind = XH_OPT_SGD;
    float lr = 0, wd = 0, beta1 = 0.9f, beta2 = 0.999f;
    float t = 1.0f;                    // adam_optimizer::t (nn.h:694)
    float *m = nullptr, *v = nullptr;  // velocity / moments (device)
  } opt[2];
  // REINFORCE (XH_PG): full-MLP policy buffers and episode bookkeeping
  struct pg_state {
    int nlayers = 0, w[4] = {0, 0, 0, 0};
    float *act[3] = {nullptr, nullptr, nullptr};
    float *grad[3] = {nullptr, nullptr, nullptr};
    int *ep_done = nullptr, *len = nullptr, *active = nullptr;
    int *row_off = nullptr, *list = nullptr, *nrows = nullptr;
    float *rtg = nullptr;
    double *ep_part = nullptr, *stats = nullptr;
    int *host_active = nullptr;  // pinned
    int slot_end = 0;            // slot holding the envs' current states
  } pg;
  // xh_trainer_set_stats (opt-in; everything null / 0 while off): the device
  // ring of rows, the envs' running episode lengths, the kernels' workgroup
  // partials and the three gradient norms; ring.rows = rows opened so far;
  // open = the last row's window is not consumed yet (learn() fills its
  // learner part)
  struct stats_state {
    xh::host::row_ring ring{nullptr, XH_STAT_COUNT};
    bool open = false;
    double *part = nullptr, *norms = nullptr;
    int *ep_len = nullptr;
  } stats;
  // xh_trainer_set_grad_clip of the policy [0] and value [1] nets (opt-in;
  // null / 0 while off): one device block per net holding the workgroup
  // partials of the sum of squares (kClipMaxParts doubles) and then the log,
  // {norm, scale} per optimizer step of a learn(); learned = a learn() has
  // filled the log since the clip was set
  struct clip_state {
    float max_norm = 0.0f;
    double *part = nullptr, *log = nullptr;
    bool learned = false;
  } clip[2];
  // xh_trainer_set_update_diag (opt-in; everything null / 0 while off): one
  // device block holding the ring of rows, the sum kernel's workgroup partials
  // and the per-row records [T][N] of the last probed learn() (ent, kl, then
  // p_new); learns = learn() calls since it was set, ring.rows = probed ones
  // (ring rows written); info / kl_source = what the last probed learn() ran
  struct upd_state {
    xh::host::row_ring ring{nullptr, XH_UPD_COUNT};
    int every = 1;
    long learns = 0;
    double *part = nullptr, *ent = nullptr, *kl = nullptr;
    float *p_new = nullptr;
    xh::KernelInfo info;
    const char *kl_source = nullptr;
  } upd;
  // the state digest's workspace (xh_trainer_state_digest,
  // xh_trainer_load_state; null until the first of them): the workgroup
  // partials, then the digests
  uint64_t *dig_ws = nullptr;
  int Tb = 0;  // Batch steps: cfg.steps, or REINFORCE's per-iteration bound
  uint32_t jump_mul = 1;
  int rgrid = 0;
  bool need_shift = false;
  // a rollout window exists that no learn() / forget() has consumed yet
  // (xh_trainer_forget refuses to shift without one)
  bool rolled = false;
  // XH_BUF_LOGITS / XH_BUF_PROBS hold a recorded rollout step
  bool last_step_recorded = false;
  // xh_trainer_set_env_state: states the next rollout starts from, keyed by
  // env (B*D bin bytes then D item bytes), applied after the forget() shift
  std::map<int, std::vector<int8_t>> env_override;
  bool use_forced = false;
  // Slots of `items` whose every env holds an item-table entry.  The train
  // kernels fold the item's layer-1 contribution into per-table-entry biases,
  // so learn() refuses a batch that reads a slot with any other item
  // (xh_trainer_set_buffer accepts them for rollout-only use).
  std::vector<char> items_ok;
  // Slots of `bins` that may hold a bin below -capacity (an overflowed state
  // the reference reaches by applying to a game-over env again, bin_packing.h:
  // 53-63, uploaded by hand).  The f16-pair kernels bound every observation
  // feature by |bins / capacity| <= 1, so a rollout step
  // or learn() that reads such a slot runs the f32-MFMA kernels instead.
  std::vector<char> bins_wide;
  // bins_wide[0] has been set at a rollout: a bin below -capacity that no
  // action takes survives into later slots and windows, which bins_wide does
  // not follow (RolloutArgs::wide_seen)
  bool wide_seen = false;
  // what the last rollout step / policy epoch launched (xh_trainer_kernel_info)
  xh::KernelInfo last_rollout, last_train;
  int timing = 0;  // 0 off, 1 every launch, XH_TIMING_TRAIN policy_train only
  bool counted = false;  // holds a reference on ctx
  std::vector<timed_event> events;
  std::vector<hipEvent_t> event_pool;  // recycled by reset_timing
  std::vector<void *> allocs;

  xh::Batch batch() const {
    xh::Batch b;
    b.N = cfg.num_envs;
    b.T = Tb;
    b.bins = bins;
    b.items = items;
    b.action = action;
    b.pold = pold;
    b.done = done;
    b.rng = rng;
    return b;
  }
  xh::ValueArgs vargs() const {
    xh::ValueArgs a{};
    a.env = env;
    a.b = batch();
    a.v_state = v_state;
    a.v_term = v_term;
    a.row_g = row_g;
    return a;
  }
  size_t N() const { return (size_t)cfg.num_envs; }
  size_t T() const { return (size_t)Tb; }
  size_t BD() const { return (size_t)cfg.bins * cfg.dims; }
};

namespace xh {
namespace host {

// Every write of a net's parameters and every host write into the batch (or
// into what the next rollout starts from) says so here, before it is issued:
// what was derived from the old contents is stale -- the value net's W0
// fragments (vfrag_ready), the rollout's forward outputs that PPO's epoch 0
// reuses (e0_valid).
enum { kWrotePolicy = 1, kWroteValue = 2, kWroteBatch = 4 };
inline void wrote(xh_trainer *t, int what) {
  if (what & kWroteValue) t->vfrag_ready = false;
  if (what & (kWrotePolicy | kWroteBatch)) t->e0_valid = false;
}
inline int wrote_net(int which) {
  return which == XH_POLICY ? kWrotePolicy : kWroteValue;
}

constexpr uint64_t kEvalStride = 1ull << 26;  // draws between env streams

template <class P>
int dalloc(xh_trainer *t, P **p, size_t bytes) {
  void *q = nullptr;
  CHK(dev_zalloc(t->ctx->stream, &q, bytes < 16 ? 16 : bytes, "trainer"));
  t->allocs.push_back(q);
  *p = reinterpret_cast<P *>(q);
  return XH_OK;
}

// Launch wrapper: optional HIP-event timing on the trainer's stream.
template <class F>
int timed(xh_trainer *t, const char *name, F &&launch) {
  hipStream_t s = t->ctx->stream;
  timed_event ev;
  const bool rec = t->timing == 1 ||
                   (t->timing == XH_TIMING_TRAIN && std::strcmp(name, "policy_train") == 0);
  if (rec) {
    ev.name = name;
    HIPCHK(pooled_event(t->event_pool, &ev.start));
    HIPCHK(pooled_event(t->event_pool, &ev.stop));
    HIPCHK(hipEventRecord(ev.start, s));
  }
  hipError_t e = launch();
  if (e != hipSuccess)
    return fail(XH_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e));
  if (rec) {
    HIPCHK(hipEventRecord(ev.stop, s));
    t->events.push_back(ev);
  }
  return XH_OK;
}

// The 64-bin PPO / actor-critic epochs run over the packed batch (DESIGN.md
// §3.0e, "duplicate rows") wherever the plain policy_train_spec8_kernel would
// run: a trainer with the buffers, no kernel override, no ablation or phase
// trace; XH_SP8_PACK=0 (read per rollout() / learn()) keeps the unpacked path.
// (learn() adds: no wide slot.)
inline bool pack_selected(const xh_trainer *t) {
  const char *m = std::getenv("XH_SP8_PACK");
  const char *ov = std::getenv("XH_TRAIN_KERNEL"), *ab = std::getenv("XH_ABLATE");
  return t->pk && !(m && *m && std::atoi(m) == 0) && !(ov && *ov) &&
         !(ab && std::atoi(ab)) && !(xh::diag_build() && std::getenv("XH_PHASE_TRACE"));
}
// The rollout writes epoch 0's records (relu masks, distributions: +0.05 ms
// at config 3) only where something reads them: a learn() that does not run
// packed, XH_E0_REUSE=2, or the update diagnostics' KL (e0_p).
inline bool rollout_wants_e0(const xh_trainer *t) {
  const char *m = std::getenv("XH_E0_REUSE");
  return !pack_selected(t) || (m && std::atoi(m) == 2) || t->upd.ring.history;
}

// A slot of the batch learn() reads may hold a bin below -capacity (bins_wide)
inline bool batch_wide(const xh_trainer *t) {
  bool wide = false;
  for (size_t sl = 0; sl < t->T() && sl < t->bins_wide.size(); ++sl)
    wide |= t->bins_wide[sl] != 0;
  return wide;
}

// trainer_learn.cpp
int allreduce(xh_trainer *t, float *buf, int n);
int allreduce_d(xh_trainer *t, double *buf, int n);
xh::MlpArgs value_mlp(xh_trainer *t, int rows, float *out);
int reduce_and_step(xh_trainer *t, int which, int step, const float *slab,
                    int nslab, int stride, int n, float *grad, float *params,
                    xh::SlabAlias al = xh::SlabAlias{0, 0, 0, 0});
int do_learn(xh_trainer *t);
// trainer_pg.cpp
int create_pg(xh_ctx *ctx, const xh_config &c, xh_trainer **out);
int do_pg_rollout(xh_trainer *t);
int do_pg_learn(xh_trainer *t);
// trainer_diag.cpp: the hooks of the opt-in diagnostics in rollout / learn
void stats_free(xh_trainer *t);
int stats_rollout(xh_trainer *t);
int stats_learn(xh_trainer *t);
void upd_free(xh_trainer *t);
int upd_learn(xh_trainer *t, bool e0_at_entry);
void clip_free(xh_trainer *t, int which);
// phase_trace.cpp: XH_ABLATE -> pa->ablate (refused by the product library)
// and, in the diagnostic build under XH_PHASE_TRACE, pa->trace armed for the
// next train launch; the report reads it back, prints it and disarms it
int phase_trace_begin(xh_trainer *t, xh::PolicyTrainArgs *pa);
int phase_trace_report(xh_trainer *t, xh::PolicyTrainArgs *pa);

}  // namespace host
}  // namespace xh

#endif  // XH_TRAINER_H_
