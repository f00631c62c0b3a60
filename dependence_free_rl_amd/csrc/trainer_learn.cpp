// trainer_learn.cpp -- learn() of the PPO / actor-critic / KL-PPO trainer in
// the reference order (policy_gradient.h:159-185): value eval -> TD targets ->
// value SGD step -> value re-eval -> GAE -> k policy epochs, and the optimizer
// step every net's gradient ends in.  With world > 1 each flat gradient is
// SUM-all-reduced with RCCL on the same stream before the identical step on
// every rank (the reference's loss is a sum over rows, nn.h:94-98, so the
// sharded sum equals the single-process gradient).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/xylo_hip.h"
#include "spec8_pack_layout.h"
#include "spec8_table_layout.h"
#include "table_tile_layout.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

namespace xh {
namespace host {
namespace {

// SUM all-reduce of a flat device buffer on the trainer's stream.  An RCCL
// failure is reported as XH_ERR_RCCL with ncclGetErrorString (and the
// communicator's async error, if it holds one), not as a HIP error.
int allreduce_t(xh_trainer *t, void *buf, int n, ncclDataType_t dt) {
  if (!t->ctx->comm) return XH_OK;
  hipStream_t s = t->ctx->stream;
  ncclResult_t r = ncclSuccess;
  if (t->ctx->fault == XH_FAULT_RCCL_ARG) {
    // test hook: the next all-reduce passes RCCL an invalid datatype, so RCCL
    // itself rejects the call
    dt = (ncclDataType_t)ncclNumTypes;
    t->ctx->fault = 0;
  }
  const int st = timed(t, "allreduce", [&]() -> hipError_t {
    r = ncclAllReduce(buf, buf, (size_t)n, dt, ncclSum, t->ctx->comm, s);
    return hipSuccess;
  });
  if (st != XH_OK) return st;
  if (r != ncclSuccess) {
    ncclResult_t ar = ncclSuccess;
    (void)ncclCommGetAsyncError(t->ctx->comm, &ar);
    return fail(XH_ERR_RCCL, "ncclAllReduce(%d x %s, rank %d of %d): %s%s%s", n,
                dt == ncclFloat64 ? "f64" : dt == ncclFloat32 ? "f32" : "?",
                t->ctx->rank, t->ctx->world,
                ncclGetErrorString(r), ar != ncclSuccess ? "; async: " : "",
                ar != ncclSuccess ? ncclGetErrorString(ar) : "");
  }
  return XH_OK;
}

// optimizer::step's next_parameters for net `which` (nn.h:594-698).
// The optimizer step's scalars (advances adam's step counter).
xh::OptStep opt_step(xh_trainer *t, int which) {
  auto &o = t->opt[which];
  // lr_scale_rows (opt-in): lr / rows of the job instead of the raw lr on
  // the row-summed gradient (nn.h:94-98, 624)
  const float lr = t->cfg.lr_scale_rows
                       ? (float)((double)o.lr /
                                 ((double)t->T() * t->cfg.num_envs_global))
                       : o.lr;
  xh::OptStep st{o.kind, lr, o.beta1, o.beta2, 1.0f, 1.0f, o.wd};
  if (o.kind == XH_OPT_ADAM) {  // host float powf, as the reference
    st.c1 = 1 - powf(o.beta1, o.t);
    st.c2 = 1 - powf(o.beta2, o.t);
    o.t += 1;
  }
  return st;
}

int opt_apply(xh_trainer *t, int which, float *params, const float *grad,
              int n) {
  wrote(t, wrote_net(which));
  hipStream_t s = t->ctx->stream;
  auto &o = t->opt[which];
  const xh::OptStep st = opt_step(t, which);
  if (o.kind == XH_OPT_SGD)
    return timed(t, "reduce_sgd", [&]() {
      return xh::launch_sgd(params, grad, n, st.lr, st.wd, s);
    });
  return timed(t, "reduce_sgd", [&]() {
    return xh::launch_opt(params, grad, o.m, o.v, n, st, s);
  });
}

}  // namespace

int allreduce(xh_trainer *t, float *buf, int n) {
  return allreduce_t(t, buf, n, ncclFloat32);
}
int allreduce_d(xh_trainer *t, double *buf, int n) {
  return allreduce_t(t, buf, n, ncclFloat64);
}

// Slab reduce -> (all-reduce) -> optimizer step.  One rank: one fused launch
// (the same sums and updates); more ranks: the all-reduce sits between.
// With xh_trainer_set_grad_clip on for the net, on either path: slab reduce
// -> (all-reduce) -> sum of squares -> clip-and-step, which logs {norm,
// scale} in row `step` of the net's clip log (clip_kernels.hip).
int reduce_and_step(xh_trainer *t, int which, int step, const float *slab,
                    int nslab, int stride, int n, float *grad, float *params,
                    xh::SlabAlias al) {
  wrote(t, wrote_net(which));
  hipStream_t s = t->ctx->stream;
  if (t->clip[which].part) {
    auto &c = t->clip[which];
    auto &o = t->opt[which];
    CHK(timed(t, "reduce_sgd", [&]() {
      return xh::launch_slab_reduce(slab, nslab, stride, n, grad, s, al);
    }));
    CHK(allreduce(t, grad, n));
    const xh::OptStep st = opt_step(t, which);
    // the optimizer steps on the mean gradient when lr_scale_rows folds
    // 1 / rows into lr (opt_step): the norm is that gradient's
    const double r = t->cfg.lr_scale_rows
                         ? 1.0 / ((double)t->T() * t->cfg.num_envs_global)
                         : 1.0;
    CHK(timed(t, "reduce_sgd", [&]() {
      return xh::launch_clip_sumsq(grad, n, c.part, s);
    }));
    return timed(t, "reduce_sgd", [&]() {
      return xh::launch_clip_step(c.part, r, c.max_norm, grad, params, o.m, o.v,
                                  n, st, nullptr, c.log + 2 * (size_t)step, s);
    });
  }
  if (!t->ctx->comm) {
    auto &o = t->opt[which];
    const xh::OptStep st = opt_step(t, which);
    return timed(t, "reduce_sgd", [&]() {
      return xh::launch_slab_reduce_opt(slab, nslab, stride, n, grad, params,
                                        o.m, o.v, st, s, al);
    });
  }
  CHK(timed(t, "reduce_sgd", [&]() {
    return xh::launch_slab_reduce(slab, nslab, stride, n, grad, s, al);
  }));
  CHK(allreduce(t, grad, n));
  return opt_apply(t, which, params, grad, n);
}

// The value net (full_layer Fin -> V1 -> V2 -> 1, ppo_training.cc:19-26) as a
// Dense MLP over `rows` rows: S_0..S_T (row = slot * N + env), then the
// terminal views E_t of transition row - N(T+1).  `out` receives V.
// layer 0 of the value net on the reduced observation (dense_kernels.hip)
#ifndef XH_VALUE_REDUCED
#define XH_VALUE_REDUCED 1
#endif
xh::MlpArgs value_mlp(xh_trainer *t, int rows, float *out) {
  xh::MlpArgs m{};
  m.env = t->env;
  m.bins = t->bins;
  m.items = t->items;
  m.N = (int)t->N();
  m.action = t->action;
  m.term_from = (int)((t->T() + 1) * t->N());
  m.max_rows = rows;
  m.nlayers = 3;
  m.w[0] = t->vl.Fin;
  m.w[1] = t->vl.V1;
  m.w[2] = t->vl.V2;
  m.w[3] = 1;
  m.params = t->vp;
  m.act[0] = t->vact[0];
  m.act[1] = t->vact[1];
  m.act[2] = out;
  m.grad[0] = t->vgr[0];
  m.grad[1] = t->vgr[1];
  m.grad[2] = t->row_g;
  // worth its extra launch from a 256-wide input on (config 2's 64-wide
  // layer 0 measured 1% slower with it)
  m.w0red = XH_VALUE_REDUCED && t->vl.Fin >= 256 ? t->vw0red : nullptr;
  m.w0frag = t->vw0frag;
  return m;
}

namespace {

// the train kernels fold the item into per-table-entry biases: every slot
// they read must hold item-table entries only
int check_items(const xh_trainer *t) {
  for (size_t sl = 0; sl < t->T(); ++sl)
    if (sl >= t->items_ok.size() || !t->items_ok[sl])
      return fail(XH_ERR_STATE,
                  "learn: slot %zu of the batch holds an item that is not an "
                  "item-table entry (set by xh_trainer_set_buffer, or no "
                  "rollout yet)", sl);
  return XH_OK;
}

// The PPO / actor-critic epochs of the 64-bin 2-D [128,128] policy over the
// packed batch (duplicate rows computed once): where the
// plain policy_train_spec8_kernel would run -- no kernel override, no wide
// slot, no ablation or phase trace.  XH_SP8_PACK=0 (read per learn()) keeps
// the unpacked path.
bool decide_pack(const xh_trainer *t) {
  return pack_selected(t) && !batch_wide(t);
}

// The packed learn()'s epochs on the table ("the epoch on the
// table"): the rollout table's own condition on top of decide_pack -- no slot
// of this trainer has held a bin below -capacity, which has no table entry.
// XH_TRAIN_TABLE (read per learn()): 0 keeps the packed launches; spec8 keeps
// the table's former launches (the spec8 kernel's table build, forward and
// backward, with the stream's reduce between them); unset or anything else:
// the lean table kernels (table_mm_kernels.hip).
enum TableMode { kTabOff = 0, kTabSpec8, kTabMm };
TableMode decide_table(const xh_trainer *t, bool pack) {
  const char *m = std::getenv("XH_TRAIN_TABLE");
  const bool spec8 = m && std::strcmp(m, "spec8") == 0;
  const bool on = pack && t->tab_pk && (t->cfg.algo == XH_PPO || t->cfg.algo == XH_AC) &&
                  !t->wide_seen && !batch_wide(t) && !(m && *m && !spec8 && std::atoi(m) == 0);
  return !on ? kTabOff : spec8 ? kTabSpec8 : kTabMm;
}

// The launches epoch e of a learn() runs: epoch 0 on the rollout's outputs, the
// epoch on the table, the packed build, or the selected plain kernel.  One
// predicate for policy_epochs and for advantages(), which skips the bound on
// |g| when no launch of the learn() reads it.
enum EpochPath { kEpE0, kEpTable, kEpPack, kEpPlain };
EpochPath epoch_path(int e, bool use_e0, bool wide, int ablate, bool trace, bool pk,
                     TableMode table) {
  if (e == 0 && use_e0 && !wide && !ablate && !trace) return kEpE0;
  if (pk && !trace && table != kTabOff) return kEpTable;
  if (pk && !trace) return kEpPack;
  return kEpPlain;
}

// Every epoch of this learn() runs the lean table kernels, which take no bound
// (XH_ABLATE / XH_PHASE_TRACE as phase_trace_begin will read them).
bool bound_unread(const xh_trainer *t, bool use_e0, bool pack, TableMode table) {
  if (table != kTabMm) return false;
  const char *ab = std::getenv("XH_ABLATE");
  const int ablate = ab ? std::atoi(ab) : 0;
  const bool trace = xh::diag_build() && std::getenv("XH_PHASE_TRACE");
  const bool wide = batch_wide(t);
  for (int e = 0; e < t->cfg.epochs; ++e)
    if (epoch_path(e, use_e0, wide, ablate, trace, pack, table) != kEpTable) return false;
  return true;
}

// One epoch on the table, the lean kernels: the tiles' forward -> the entries'
// logits and H2; the streaming pass over the packed batch -> its workgroups'
// sums; the tiles' backward, which sums them into G -> tt::kTiles slabs in
// tab_slab.  zero_ood: the forward also zeroes the out-of-domain counter.
hipError_t table_epoch_mm(xh_trainer *t, const xh::PolicyTrainArgs &pa, bool count,
                          bool zero_ood, hipStream_t s) {
  hipError_t e = xh::launch_table_fwd(
      xh::TableFwdArgs{pa.env, pa.params, t->tab_logits, t->tab_h2,
                       zero_ood ? t->tab_ood : nullptr}, s);
  if (e != hipSuccess) return e;
  const xh::TableStreamArgs sa{pa.pk,       pa.pk_hdr,   t->tab_logits,
                               pa.algo,     pa.clip_eps, t->tab_part,
                               t->tab_G,    t->tab_gmax, count ? t->tab_ood : nullptr};
  e = xh::launch_table_stream(sa, t->pslab_n, s, false);
  if (e != hipSuccess) return e;
  return xh::launch_table_bwd(
      xh::TableBwdArgs{pa.env, pa.params, t->tab_h2, t->tab_part, t->pslab_n, t->tab_G,
                       t->tab_slab, t->pslab_stride}, s);
}

// One epoch on the table, the former launches (XH_TRAIN_TABLE=spec8): the table
// batch's forward -> the entries' logits; the streaming pass over the packed
// batch and its reduce -> G and max |G|; the table batch's backward weighted by
// G -> `grid` slabs.
hipError_t table_epoch(xh_trainer *t, const xh::PolicyTrainArgs &pa, int grid, bool count,
                       hipStream_t s) {
  xh::PolicyTrainArgs ta = pa;
  ta.pk = t->tab_pk;
  hipError_t e = xh::launch_policy_train_spec8_tab(
      ta, xh::PolicyTrainTabArgs{t->tab_logits, nullptr, 1}, grid, s);
  if (e != hipSuccess) return e;
  const xh::TableStreamArgs sa{pa.pk,       pa.pk_hdr,   t->tab_logits,
                               pa.algo,     pa.clip_eps, t->tab_part,
                               t->tab_G,    t->tab_gmax, count ? t->tab_ood : nullptr};
  e = xh::launch_table_stream(sa, t->pslab_n, s);
  if (e != hipSuccess) return e;
  ta.g_bound = t->tab_gmax;
  return xh::launch_policy_train_spec8_tab(ta, xh::PolicyTrainTabArgs{nullptr, t->tab_G, 0},
                                           grid, s);
}

// the compaction pass: once per learn(), behind the final advantages.
// XH_SP8_PACK_DEDUP=loop (read per learn(); A/B runs and tests): the former
// classify and write kernels, the same bytes.
int pack_batch(xh_trainer *t, xh::PolicyTrainArgs *pa) {
  hipStream_t s = t->ctx->stream;
  const xh::PackArgs ka{t->env, t->batch(), t->adv, t->pk, t->pk_hdr, t->pk_cls, t->pk_blk};
  const char *dd = std::getenv("XH_SP8_PACK_DEDUP");
  const bool loop = dd && std::strcmp(dd, "loop") == 0;
  CHK(timed(t, "pack", [&]() { return xh::launch_spec8_pack(ka, loop, s); }));
  pa->pk = t->pk;
  pa->pk_hdr = t->pk_hdr;
  t->pk_learned = true;
  return XH_OK;
}

// Epoch 0 on the rollout's forward outputs (policy_train_spec8_e0_kernel):
// PPO with a later epoch to follow, the outputs valid, nothing that selects
// or instruments the train kernel.  XH_E0_REUSE (read per learn()): 0 never,
// unset / 1 when valid and the learn() does not run packed, 2 (tests, A/B
// runs) always, failing the learn() when epoch 0 cannot.
int decide_e0_reuse(const xh_trainer *t, bool pack, bool *use_e0) {
  const xh_config &c = t->cfg;
  const char *m = std::getenv("XH_E0_REUSE");
  const int mode = m && *m ? std::atoi(m) : 1;
  const char *ov = std::getenv("XH_TRAIN_KERNEL"), *ab = std::getenv("XH_ABLATE");
  const bool wide = batch_wide(t);
  // (a packed learn(): its epoch 0 runs packed as well, a quarter of the
  // groups against the e0 kernel's saved forward pass -- DESIGN.md §8 -- unless
  // 2 asks for the e0 kernel)
  *use_e0 = mode != 0 && (mode == 2 || !pack) && t->e0_valid && t->e0_mask && t->e0_p &&
            c.algo == XH_PPO && c.epochs >= 2 && !(ov && *ov) && !wide &&
            !(ab && std::atoi(ab)) &&
            !(xh::diag_build() && std::getenv("XH_PHASE_TRACE"));
  if (mode == 2 && !*use_e0)
    return fail(XH_ERR_STATE, "learn: XH_E0_REUSE=2, but epoch 0 cannot run on "
                "the rollout's forward outputs (%s)",
                !t->e0_mask ? "this trainer has none: PPO with epochs >= 2 at "
                              "64 bins, 2-D, [128,128] only"
                : !t->e0_valid ? "not valid: no split rollout of this window "
                                 "under the current policy parameters and batch"
                               : "a kernel override or a wide slot");
  return XH_OK;
}

// update_value_model (policy_gradient.h:196-218): V over S_0..S_T and the
// terminal views E_t of the ended transitions in one batch (NS + n_end
// rows, a device count), TD targets and dL/dV = V - target on the
// transition rows (end rows have zero gradient), backward, one step
// (the terminal views' values also land on their transition rows, v_term).
// Leaves `vm` set up for the re-evaluation and says whether the bf16 value
// kernel runs it (vnet).
int value_step(xh_trainer *t, xh::MlpArgs *vm_out, bool *vnet_out) {
  hipStream_t s = t->ctx->stream;
  xh::ValueArgs va = t->vargs();
  const int NS = (int)((t->T() + 1) * t->N()), NT = (int)(t->T() * t->N());
  // the transitions that ended an episode (env-major, t ascending); their
  // terminal views are the only end rows whose V the targets read
  xh::EndListArgs ea{t->done, (int)t->N(), (int)t->T(), t->end_list,
                     t->n_end, t->n_open, t->vrows, NS};
  CHK(timed(t, "value", [&]() {
    return xh::launch_end_list(ea, t->end_scratch, s);
  }));
  xh::MlpArgs vm = value_mlp(t, NS + NT, t->v_state0);
  vm.act_rows = NT;  // the backward reads the transition rows' activations
  vm.rows = t->vrows;
  vm.term_list = t->end_list;
  vm.v_term = t->v_term;
  vm.term_n = t->n_end;
  const bool vnet = std::strcmp(xh::value_kernel_name(vm), "vnet_bf16") == 0;
  vm.w0frag_ready = vnet && t->vfrag_ready;
  CHK(timed(t, "value", [&]() { return xh::mlp_forward(vm, s); }));
  t->vfrag_ready = vnet;
  vm.rows = nullptr;
  vm.term_list = nullptr;
  vm.v_term = nullptr;
  va.v_state = t->v_state0;
  vm.max_rows = NT;
  CHK(timed(t, "value", [&]() {
    return xh::value_backward(vm, va, t->cfg.gamma, t->targets, t->vslab,
                              t->vslab_stride, t->vslab_n, s);
  }));
  // the reduced layer 0 writes bin 0's item columns only (EpSlabRed)
  const xh::SlabAlias al =
      xh::value_reduced_slab(vm) ? xh::SlabAlias{t->cfg.value_h1, t->vl.Fin, t->cfg.bins,
                               t->cfg.dims}
               : xh::SlabAlias{0, 0, 0, 0};
  CHK(reduce_and_step(t, XH_VALUE, 0, t->vslab, t->vslab_n, t->vslab_stride,
                      t->nv, t->vgrad, t->vp, al));
  *vm_out = vm;
  *vnet_out = vnet;
  return XH_OK;
}

// calculate_advantage (policy_gradient.h:220-281) on post-update values;
// GAE zeroes V(terminal), the targets above used V(E_t).  Then the opt-in
// normalisation and, for PPO / AC, the bound on |g| in pa->g_bound -- unless
// no launch of this learn() reads it (need_bound false: bound_unread).
int advantages(xh_trainer *t, xh::MlpArgs vm, bool vnet,
               xh::PolicyTrainArgs *pa, bool need_bound) {
  hipStream_t s = t->ctx->stream;
  const xh_config &c = t->cfg;
  const int NS = (int)((t->T() + 1) * t->N()), NT = (int)(t->T() * t->N());
  vm.max_rows = NS;
  vm.act[2] = t->v_state;
  vm.act_rows = -1;  // no backward reads these
  vm.w0frag_ready = 0;  // (new parameters)
  CHK(timed(t, "value", [&]() { return xh::mlp_forward(vm, s); }));
  t->vfrag_ready = vnet;
  xh::ValueArgs va = t->vargs();
  va.row_g = nullptr;
  CHK(timed(t, "value", [&]() {
    return xh::launch_gae(va, c.gamma, c.lambda, t->adv,
                          c.adv_normalize ? t->adv_part : nullptr, s);
  }));
  if (c.adv_normalize) {  // opt-in: job-wide mean / std of the advantages
    CHK(timed(t, "value", [&]() {
      return xh::launch_adv_stats(t->adv_part, xh::gae_grid((int)t->N()),
                                  t->adv_stats, s);
    }));
    CHK(allreduce_d(t, t->adv_stats, 2));
    CHK(timed(t, "value", [&]() {
      return xh::launch_adv_normalize(t->adv, (long)(t->T() * t->N()),
                                      t->adv_stats,
                                      (double)t->T() * c.num_envs_global, s);
    }));
  }
  if ((c.algo == XH_PPO || c.algo == XH_AC) && need_bound) {
    // the bound on |g| the 64-bin train kernel scales dW2's operand by: from
    // the final advantages and p_old, the same in all k epochs
    CHK(timed(t, "value", [&]() {
      return xh::launch_g_bound(t->adv, t->pold, (long)NT, c.algo == XH_PPO,
                                c.clip_eps, t->g_bound, s);
    }));
    pa->g_bound = t->g_bound;
  }
  return XH_OK;
}

// optimize_action: k policy steps (policy_gradient.h:297-307); KL-PPO adapts
// beta from the job's mean KL after each of them.
int policy_epochs(xh_trainer *t, xh::PolicyTrainArgs &pa, bool use_e0, TableMode table,
                  bool ood_zeroed) {
  hipStream_t s = t->ctx->stream;
  const xh_config &c = t->cfg;
  pa.env = t->env;
  pa.b = t->batch();
  pa.algo = c.algo;
  pa.clip_eps = c.clip_eps;
  pa.params = t->pp;
  pa.adv = t->adv;
  pa.slab = t->pslab;
  pa.slab_stride = t->pslab_stride;
  pa.wide = batch_wide(t);
  CHK(phase_trace_begin(t, &pa));
  const bool kl = c.algo == XH_KLPPO;
  if (kl) {
    pa.qold = t->qold;
    pa.beta = t->beta;
    pa.end_list = t->end_list;
    pa.n_end = t->n_end;
    pa.kl_part = t->kl_part;
    // end_list / n_end / n_open: built before the value step
  }
  bool counted = false;  // the table's out-of-domain rows: once per learn()
  for (int e = 0; e < c.epochs; ++e) {
    float *g = t->pgrads + (size_t)e * t->np;
    int nslab = t->pslab_n;
    const float *slab = t->pslab;
    const EpochPath path = epoch_path(e, use_e0, pa.wide, pa.ablate, pa.trace != nullptr,
                                      pa.pk != nullptr, table);
    if (path == kEpE0) {
      // (the later epochs' launches report the kernel: last_train)
      const xh::PolicyTrainE0Args ea{t->e0_p, t->e0_mask};
      CHK(timed(t, "policy_train", [&]() {
        return xh::launch_policy_train_spec8_e0(pa, ea, t->pslab_n, s);
      }));
    } else if (path == kEpTable) {
      // the epoch on the table: its launches in one interval; the arithmetic
      // behind g is the same kernel's, and it reports as the plain one
      t->last_train.name = "policy_train_spec8_kernel";
      t->last_train.math = xh::kMathSplitTrainF16Pair;
      if (table == kTabMm) {
        // the tiles' own slabs, whatever the train grid
        nslab = xh::tt::kTiles;
        slab = t->tab_slab;
        CHK(timed(t, "policy_train", [&]() {
          return table_epoch_mm(t, pa, !counted, !counted && !ood_zeroed, s);
        }));
      } else {
        nslab = t->pslab_n < xh::tb::kGroups ? t->pslab_n : xh::tb::kGroups;
        CHK(timed(t, "policy_train", [&]() { return table_epoch(t, pa, nslab, !counted, s); }));
      }
      counted = true;
      t->tab_learned = true;
    } else if (path == kEpPack) {
      // the same kernel's packed build: it reports as the plain one
      t->last_train.name = "policy_train_spec8_kernel";
      t->last_train.math = xh::kMathSplitTrainF16Pair;
      CHK(timed(t, "policy_train", [&]() {
        return xh::launch_policy_train_spec8_pack(pa, t->pslab_n, s);
      }));
    } else {
      CHK(timed(t, "policy_train", [&]() {
        return xh::launch_policy_train(pa, c.policy_h1, c.policy_h2, t->pslab_n,
                                       s, &t->last_train);
      }));
    }
    if (pa.trace) CHK(phase_trace_report(t, &pa));  // first epoch only
    // the optimizer step does not read beta: it may precede the KL update
    CHK(reduce_and_step(t, XH_POLICY, e, slab, nslab,
                        t->pslab_stride, t->np, g, t->pp));
    if (kl) {  // mean KL over the job's rows -> beta for the next epoch
      CHK(timed(t, "kl", [&]() {
        return xh::launch_kl_reduce(t->kl_part, t->pslab_n, t->n_end,
                                    t->n_open, (double)t->T() * t->N(),
                                    t->kl_sum, s);
      }));
      CHK(allreduce_d(t, t->kl_sum, 2));
      CHK(timed(t, "kl", [&]() {
        return xh::launch_kl_beta_update(t->kl_sum, t->beta, c.kl_target,
                                         t->kl_log + 3 * e, s);
      }));
    }
  }
  return XH_OK;
}

}  // namespace

int do_learn(xh_trainer *t) {
  if (t->cfg.algo == XH_PG) return do_pg_learn(t);
  CHK(check_items(t));
  const bool e0_at_entry = t->e0_valid;  // for the update diagnostics
  bool use_e0 = false;
  const bool pack = decide_pack(t);
  CHK(decide_e0_reuse(t, pack, &use_e0));
  xh::MlpArgs vm{};
  bool vnet = false;
  CHK(value_step(t, &vm, &vnet));
  xh::PolicyTrainArgs pa{};
  const TableMode table = decide_table(t, pack);
  const bool lean = bound_unread(t, use_e0, pack, table);
  CHK(advantages(t, vm, vnet, &pa, !lean));
  t->pk_learned = false;
  if (pack) CHK(pack_batch(t, &pa));
  t->tab_learned = false;
  // the out-of-domain counter: zeroed by the first table forward where the
  // lean kernels run epoch 0, by a memset otherwise
  if (table != kTabOff && !lean)
    HIPCHK(hipMemsetAsync(t->tab_ood, 0, sizeof(int), t->ctx->stream));
  CHK(policy_epochs(t, pa, use_e0, table, !lean));
  for (auto &cl : t->clip) cl.learned = cl.part != nullptr;
  if (t->upd.ring.history) CHK(upd_learn(t, e0_at_entry));
  if (t->stats.ring.history) CHK(stats_learn(t));
  t->need_shift = true;
  t->rolled = false;
  return XH_OK;
}

}  // namespace host
}  // namespace xh
