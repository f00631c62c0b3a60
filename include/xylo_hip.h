/* xylo_hip.h -- C ABI of the MI355X-native PPO / actor-critic hot path.
 *
 * The drop-in boundary for the rollout-and-update path of
 * beehover/dependence_free_rl (reference @ 2024_10_08; citations are
 * file:line under that tree).  Plain pointers, sizes and int status codes;
 * no C++ or torch types cross this boundary; no exception escapes it.
 * Host wrappers (include/xylo_hip/ headers, dependence_free_rl_amd/_lib.py)
 * rethrow / raise on a non-zero status with xh_last_error().
 *
 * Reference interfaces replaced (one xh_trainer = many envs + the learner):
 *   xylo::environment<A,S>::apply/view/reset   xylo/rl.h:163-170
 *   bp::environment, bp::agent                 apps/bin_packing/bin_packing.h:46-107
 *   xylo::agent::step / play_steps             xylo/rl.h:325-360
 *   xylo::replay_buffer (sample_td, forget)    xylo/rl.h:213-296
 *   xylo::policy_gradient_policy::react        xylo/policy_gradient.h:337-354
 *   xylo::discrete_action::from_vector         xylo/rl.h:27-30
 *   xylo::actor_critic_learner::learn          xylo/policy_gradient.h:159-281
 *   xylo::ppo_learner::optimize_action         xylo/policy_gradient.h:297-307
 *   xylo::model::parameters / set_parameters   xylo/nn.h:490-508
 *   xylo::sgd_optimizer                        xylo/nn.h:616-628
 *   (and the tensor.{h,cc} / nn.h Dense, relu, softmax loops underneath)
 */
#ifndef XYLO_HIP_H_
#define XYLO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ status ---- */
enum {
  XH_OK = 0,
  XH_ERR_INVALID = 1,     /* bad argument / unsupported shape   */
  XH_ERR_HIP = 2,         /* HIP runtime error                   */
  XH_ERR_RCCL = 3,        /* RCCL error                          */
  XH_ERR_STATE = 4        /* call out of order                   */
};
/* Message of the last failing call on this thread ("" if none). */
const char *xh_last_error(void);
/* Library version string. */
const char *xh_version(void);
/* Number of visible HIP devices (initialises the HIP runtime). */
int xh_device_count(int *out);
/* JSON object naming the HIP and RCCL shared objects this process bound and
 * their versions: {"libamdhip64": path, "hip_runtime": n, "librccl": path,
 * "rccl_version": n}.  Written NUL-terminated into buf[cap]. */
int xh_runtime_info(char *buf, size_t cap);

/* ------------------------------------------------------------ context --- */
typedef struct xh_ctx xh_ctx;
/* 128-byte RCCL unique id (ncclGetUniqueId) for a world > 1 job. */
int xh_comm_unique_id(void *out128);
/* device: HIP device ordinal; rank/world: this process in a one-process-per-
 * GPU job; uid128 (required when world > 1): the id from rank 0, broadcast
 * by the caller.  With world == 1 a non-null uid128 creates a one-rank RCCL
 * communicator, so the all-reduce path runs on a single device too. */
int xh_ctx_create(int device, int rank, int world, const void *uid128,
                  xh_ctx **out);
int xh_ctx_destroy(xh_ctx *ctx);
int xh_ctx_synchronize(xh_ctx *ctx);
/* Sum-all-reduce of n floats of host memory over the job (tests/tools). */
int xh_ctx_allreduce_host(xh_ctx *ctx, float *data, size_t n);
/* Test hook: make the next gradient all-reduce of a trainer on this context
 * pass RCCL an invalid argument (XH_FAULT_RCCL_ARG), so that the error path
 * (XH_ERR_RCCL with ncclGetErrorString) runs against the real library.
 * XH_FAULT_NONE clears it.  XH_ERR_STATE without a communicator. */
enum { XH_FAULT_NONE = 0, XH_FAULT_RCCL_ARG = 1 };
int xh_ctx_inject_fault(xh_ctx *ctx, int kind);

/* ------------------------------------------------------------ trainer --- */
/* XH_KLPPO: kl_ppo_learner (policy_gradient.h:310-335, ppo2_training.cc):
 * PPO's k = 4 full-batch epochs with kl_regulated_loss and an adaptive beta
 * that carries over from one learn() to the next.  Per-bin shapes with
 * bins <= 64, and 128 bins 3-D [128,128] (the split train kernel only: a
 * batch holding an overflowed bin fails its learn() there). */
/* XH_PG: policy_gradient_learner = REINFORCE (policy_gradient.h:88-147,
 * bp::pg_learner, pg_training.cc) with a FULL-layer policy
 * full(4B, policy_h1) - relu [- full(policy_h1, policy_h2) - relu] -
 * full(., B) - softmax_cross_entropy (policy_h2 = 0: one hidden layer), no
 * value net.  `steps` is the number of whole episodes each env plays per
 * iteration (play_one_episode, rl.h:351-354); env g plays on its own engine
 * stream, rng_state advanced by g * 2^26 draws (env 0 = the single-env
 * reference run).  The batch buffers hold `xh_trainer_buffer_bytes`-sized
 * [Tmax][N] grids, Tmax = steps * (longest possible episode); XH_BUF_LEN
 * gives each env's step count of the last rollout. */
enum { XH_PPO = 0, XH_AC = 1, XH_KLPPO = 2, XH_PG = 3 };

typedef struct {
  int algo;            /* XH_PPO | XH_AC (actor_critic_learner) | XH_KLPPO
                          | XH_PG */
  int num_envs;        /* envs on this rank (multiple of 64/bins)            */
  int num_envs_global; /* envs in the whole job (reference-order RNG streams) */
  int env_offset;      /* global index of this rank's first env              */
  int bins, dims;      /* B (bin_packing.h:12 num_bins), D (2 in the ref)    */
  int steps;           /* T: env steps per env per iteration (play_steps(T));
                          1..1024 (REINFORCE: episodes per env, 1..64)     */
  int epochs;          /* PPO / KL-PPO k (policy_gradient.h:300), 1 for AC  */
  int policy_h1, policy_h2; /* per-bin conv1d_1 widths                       */
  int value_h1, value_h2;   /* value full_layer widths (64, 32)              */
  float lr_policy, lr_value, wd_policy, wd_value;
  float gamma;         /* 0.99 */
  float lambda;        /* 0.95 (policy_gradient.h:286) */
  float clip_eps;      /* 0.2  (rl.h:56) */
  uint32_t rng_state;  /* minstd_rand0 state before the envs are constructed */
  float kl_beta;       /* KL-PPO initial beta (1, policy_gradient.h:332)     */
  float kl_target;     /* KL-PPO d_targ (1e-9, policy_gradient.h:333)        */
  /* Opt-in options, both 0 (off) in the reference-parity configuration:   */
  int adv_normalize;   /* 1: after GAE, A <- (A - mean) / (std + 1e-8) over
                          the job's T * num_envs_global transitions (the
                          reference normalises nothing, policy_gradient.h:
                          220-281); statistics by wave reductions, summed
                          across ranks */
  int lr_scale_rows;   /* 1: both optimizers apply lr / rows, rows = T *
                          num_envs_global, i.e. SGD on the mean instead of the
                          reference's sum over rows (nn.h:94-98, 624) */
  /* Test-only: 0 (default) = the policy train kernels' own grid (one or two
     workgroups per CU); > 0 caps the number of train workgroups, so that a
     batch the oracle can check in seconds runs each workgroup over as many
     row groups as the benchmark's full batch does (the f32 accumulation
     depth of the per-workgroup gradient slabs).  Reported by
     xh_trainer_kernel_info ("train_grid", "train_grid_cap"); bench.py
     refuses a trainer with a cap. */
  int train_grid_cap;
  /* 1: rollouts also record every step's whole sampling distribution into
     XH_BUF_QOLD (always on for XH_KLPPO), for a learner assembled on the
     host from the layer / loss pieces below whose loss reads it
     (discrete_action::distrib, rl.h:27-30).  0 (default): only p_old. */
  int record_distrib;
  /* 1: the rollout also writes the last slot's logits and probabilities
     (XH_BUF_LOGITS / XH_BUF_PROBS: [N][B] f32 each, 16.8 MB per iteration at
     config 3) for tests and health checks.  0 (default): the product path
     writes neither, and reading those buffers fails with XH_ERR_STATE.
     xh_trainer_set_record_last_step changes it between iterations. */
  int record_last_step;
} xh_config;

/* Fill `c` with the reference defaults (ppo_training.cc) for B bins, D dims. */
void xh_config_default(xh_config *c, int algo, int bins, int dims, int num_envs,
                       int steps);

typedef struct xh_trainer xh_trainer;
/* Allocates all device buffers, constructs the envs (2 engine draws each,
 * bin_packing.h:50-52) and zero-initialises both nets (set params next). */
int xh_trainer_create(xh_ctx *ctx, const xh_config *cfg, xh_trainer **out);
int xh_trainer_destroy(xh_trainer *t);

enum { XH_POLICY = 0, XH_VALUE = 1 };
/* Flat parameters in the reference model::parameters() layout (nn.h:499-508):
 * per dense layer [A(out x in) row-major, b(out)]; weights.20 loads as-is. */
size_t xh_trainer_num_params(const xh_trainer *t, int which);
int xh_trainer_set_params(xh_trainer *t, int which, const float *host,
                          size_t n);
int xh_trainer_get_params(xh_trainer *t, int which, float *host, size_t n);

/* Optimizer of the policy (XH_POLICY) or value (XH_VALUE) net, replacing
 * xylo::sgd_optimizer / momentum_optimizer / adam_optimizer (nn.h:616-698)
 * passed to the learner constructor.  Default: sgd with the xh_config lr /
 * wd.  momentum: v = 0.9 v + g, p - lr v.  adam: moments with beta1, beta2,
 * bias-corrected with the step counter t = 1, 2, ... of this optimizer,
 * p - lr m^ / (sqrt(v^) + 1e-7).  weight_decay must be 0 unless sgd.  The
 * state (velocity, moments, t) restarts from zero at this call and then
 * persists across learn() calls, as the reference optimizer object's does. */
enum { XH_OPT_SGD = 0, XH_OPT_MOMENTUM = 1, XH_OPT_ADAM = 2 };
int xh_trainer_set_optimizer(xh_trainer *t, int which, int kind, float lr,
                             float weight_decay, float beta1, float beta2);

/* optimizer::set_rate (nn.h:591): new learning rate for the policy / value
 * optimizer from the next learn() on; its state (velocity, moments, adam's
 * step counter) is kept. */
int xh_trainer_set_learning_rate(xh_trainer *t, int which, float lr);

/* Global-norm gradient clipping, off by default (the reference's optimizers
 * have none): with it off learn() launches what it launches without this call
 * and no buffer is allocated.  With it on for net `which`, every optimizer
 * step of that net becomes, entirely on the trainer's stream:
 *   ss    = sum_i (double)g[i] * (double)g[i]   g: the gradient the optimizer
 *           is about to read (XH_BUF_POLICY_GRADS row e / XH_BUF_VALUE_GRAD:
 *           slab-reduced and, with a communicator, all-reduced); double
 *           partials in a fixed order, no floating-point atomics
 *   norm  = sqrt(ss) * r                        r = 1 / (T * num_envs_global)
 *           in double with xh_config.lr_scale_rows (the optimizer then works
 *           on the mean gradient), else exactly 1
 *   scale = (float)(norm > max_norm ? (double)max_norm / norm : 1.0)
 *   g'[i] = g[i] * scale                        one f32 multiply
 * and the optimizer of xh_trainer_set_optimizer steps on g'.  A zero or NaN
 * norm gives scale 1 (the comparison is false; a NaN still reaches the log
 * and the parameters), an infinite norm scale 0.  The clip is per net and per
 * optimizer step: each policy epoch has its own norm.  The gradient buffers
 * and XH_STAT_PGRAD_SQ_* / XH_STAT_VGRAD_SQ keep reporting g as reduced, not
 * g'.  Two launches are added per clipped step, no host synchronisation.  In
 * a world > 1 job every rank computes the same ss from the same all-reduced
 * bits in the same order (no collective is added); every rank must set the
 * same max_norm.
 *
 * max_norm > 0 and finite: clip net `which` from the next learn() on; 0: off
 * (workspace freed).  Negative, NaN or inf: XH_ERR_INVALID.  XH_VALUE on an
 * XH_PG trainer: XH_ERR_INVALID.  Optimizer state is kept;
 * xh_trainer_set_optimizer keeps the clip. */
int xh_trainer_set_grad_clip(xh_trainer *t, int which, float max_norm);
/* Synchronises.  out[rows][2] = {norm, scale} of every optimizer step of net
 * `which` in the last learn(): `epochs` rows for the policy (1 for XH_PG), 1
 * for the value net.  XH_ERR_STATE when clipping is off for `which` or no
 * learn() has run since it was set; XH_ERR_INVALID when cap_rows is too
 * small. */
int xh_trainer_get_grad_clip_log(xh_trainer *t, int which, double *out,
                                 int cap_rows, int *rows);

/* Turn the last-step logits / probabilities record (xh_config.
 * record_last_step) on or off from the next rollout on. */
int xh_trainer_set_record_last_step(xh_trainer *t, int on);

/* One iteration's rollout: T steps of every env (one kernel per step). */
int xh_trainer_rollout(xh_trainer *t);
/* learn(): value step, advantages, `epochs` policy steps; then the batch's
 * final states become the next iteration's starting states (forget()). */
int xh_trainer_learn(xh_trainer *t);
/* `iterations` x (rollout + learn), asynchronous on the trainer's stream. */
int xh_trainer_iterate(xh_trainer *t, int iterations);
/* Teacher forcing: actions [T][N] used instead of sampling (the sampler's two
 * engine draws are still consumed).  NULL disables. */
int xh_trainer_set_forced_actions(xh_trainer *t, const int32_t *host);

/* Batch / diagnostics buffers (host copies; sizes in bytes must match). */
enum {
  XH_BUF_BINS = 0,     /* int8  [T+1][N][B][D]  states S_t (slot T = next S_0) */
  XH_BUF_ITEMS = 1,    /* int8  [T+1][N][4]                                  */
  XH_BUF_ACTION = 2,   /* int32 [T][N]                                       */
  XH_BUF_POLD = 3,     /* f32   [T][N]  distrib[choice] at sampling          */
  XH_BUF_DONE = 4,     /* uint8 [T][N]                                       */
  XH_BUF_RNG = 5,      /* uint32 [N]   per-env engine state                  */
  XH_BUF_V_STATE = 6,  /* f32   [T+1][N] V(S_t) of the last value eval       */
  XH_BUF_V_TERM = 7,   /* f32   [T][N]  V(terminal view of step t); entries  */
                       /*   of transitions that did not end are unspecified */
  XH_BUF_TARGETS = 8,  /* f32   [T][N]  TD targets                           */
  XH_BUF_ADV = 9,      /* f32   [T][N]  advantages                           */
  XH_BUF_VALUE_GRAD = 10,  /* f32 [value params]  last value gradient        */
  XH_BUF_POLICY_GRADS = 11,/* f32 [epochs][policy params]                    */
  XH_BUF_LOGITS = 12,  /* f32   [N][B]  logits of the last rollout step
                                  (xh_config.record_last_step)              */
  XH_BUF_PROBS = 13,   /* f32   [N][B]  probabilities of the last step (idem) */
  XH_BUF_V_STATE0 = 14,/* f32   [T+1][N] V(S_t) before the value step        */
  XH_BUF_QOLD = 15,    /* f32   [T][N][B] sampled distributions (KL-PPO, or
                                  xh_config.record_distrib)                  */
  XH_BUF_KL = 16,      /* f32   [epochs][3] KL-PPO: beta used, mean KL, new
                                  beta of the last learn()                   */
  XH_BUF_LEN = 17,     /* int32 [N]  REINFORCE: env steps of the last rollout */
  XH_BUF_COUNT
};
size_t xh_trainer_buffer_bytes(const xh_trainer *t, int which);
int xh_trainer_get_buffer(xh_trainer *t, int which, void *host, size_t bytes);
int xh_trainer_set_buffer(xh_trainer *t, int which, const void *host,
                          size_t bytes);

/* Deterministic evaluation (policy_gradient_deterministic_policy,
 * policy_gradient.h:356-373; agent::play_one_episode, rl.h:351-354; the
 * drivers' 100-episode eval, ppo_training.cc:67-81; deep_agent.cc:25-41)
 * with the trainer's current policy.  n_envs independent envs (a multiple of
 * 64/bins) each play `episodes` whole episodes taking the argmax action (over
 * the softmax output if argmax_probs, else over the raw logits).
 *
 * Env e's minstd_rand0 stream starts at rng_state advanced by e * 2^26 draws,
 * so env 0 reproduces a single-env reference run whose global engine is at
 * rng_state.  With init_items == NULL every env is first constructed
 * (bins at capacity + get_item = 2 draws, bin_packing.h:50-52); otherwise env
 * e starts with bins at capacity and item init_items[e*dims ...] (an env that
 * was constructed or reset earlier) and draws nothing before its first step.
 * Outputs (host arrays, each may be NULL): totals/steps per env (summed
 * rewards, env steps), final_items (item after the last reset), rng_out (the
 * stream state after the last draw), trace (env 0's actions, the first
 * trace_cap of them). */
typedef struct xh_eval {
  int n_envs;
  int episodes;
  int argmax_probs;
  uint32_t rng_state;
  const int32_t *init_items; /* [n_envs][dims] or NULL */
  int32_t *final_items;      /* [n_envs][dims] or NULL */
  uint32_t *rng_out;         /* [n_envs] or NULL */
  double *totals;            /* [n_envs] or NULL */
  long *steps;               /* [n_envs] or NULL */
  int32_t *trace;            /* [trace_cap] or NULL */
  long trace_cap;
  double elapsed_ms;         /* out: device time of the evaluation kernel */
} xh_eval;
int xh_trainer_evaluate(xh_trainer *t, xh_eval *e);

/* The reference's heuristic agents as device policies, on independent envs
 * with the stream convention of xh_trainer_evaluate (env 0 reproduces a
 * single-env reference run): XH_HEUR_RANDOM = xylo::random_policy (rl.h:
 * 305-316, random_agent.cc), XH_HEUR_FIRSTFIT (firstfit_agent.cc:10-28),
 * XH_HEUR_BESTFIT (bestfit_agent.cc:10-30), XH_HEUR_MINWASTE
 * (minwaste_agent.cc:10-39).  bins in {8,16,32,64}, dims 1..3. */
enum { XH_HEUR_RANDOM = 0, XH_HEUR_FIRSTFIT = 1, XH_HEUR_BESTFIT = 2,
       XH_HEUR_MINWASTE = 3 };
int xh_heuristic_evaluate(xh_ctx *ctx, int policy, int bins, int dims,
                          xh_eval *e);

/* Re-base the per-env engine streams on a global minstd_rand0 state x: the
 * next rollout steps env g (global index) from x advanced by 4*T*g draws, i.e.
 * the reference order in which worker 0 plays its T steps, then worker 1, ...
 * (ppo_training.cc:53-62 run sequentially, 4 draws per step).  After that
 * rollout the global engine is at x advanced by 4*T*num_envs_global.
 * XH_PG: env g's stream <- x advanced by g * 2^26 draws (env 0 continues the
 * engine as a single reference worker does). */
int xh_trainer_seed_streams(xh_trainer *t, uint32_t x);

/* The state each env of the trainer starts its NEXT rollout step from (after
 * learn() that is the batch's final state, which forget() keeps,
 * rl.h:274-291): envs [first, first + count), bins int8 [count][B][D] and
 * items int8 [count][D] (bp::environment::view, bin_packing.h:65).  set
 * replaces it (a host-side apply / reset of that env between iterations);
 * it never alters the current batch the learner reads. */
int xh_trainer_get_env_state(xh_trainer *t, int first, int count, int8_t *bins,
                             int8_t *items);
int xh_trainer_set_env_state(xh_trainer *t, int first, int count,
                             const int8_t *bins, const int8_t *items);

/* ------------------------------------------- training statistics ---- */
/* On-device training statistics, off by default: with them off no launch is
 * added and no buffer allocated.  With them on, every iteration leaves one
 * row of XH_STAT_COUNT doubles in a device ring of `history_rows` rows, so
 * that xh_trainer_iterate(t, n) can be followed by ONE synchronising read of
 * its n rows (the reference drivers report only a separate 100-episode argmax
 * evaluation every 100 rounds, ppo_training.cc:67-81; an episode spans
 * several play_steps(T) windows, rl.h:325-360, so no single batch holds its
 * return).
 *
 * The rollout opens a row and writes the episode part; learn() fills the
 * learner part of the open row.  A row whose window xh_trainer_forget
 * consumed, or nothing consumed yet, keeps NaN in its learner part.
 *
 * Every entry is a double sum formed on the device without floating-point
 * atomics: per-workgroup partials, then a fixed-order sum in one wave, so a
 * row is bit-identical from run to run.  In a world > 1 job the "summed"
 * entries are the job's (one SUM all-reduce of doubles per phase); the others
 * are job-wide already. */
enum {
  /* -- episode part (rollout); summed over ranks from EPISODES on -- */
  XH_STAT_ITER = 0,        /* row index: rollouts since xh_trainer_set_stats */
  XH_STAT_TRANSITIONS = 1, /* T * num_envs_global (every agent's
                              play_steps(T), rl.h:356-360)                   */
  XH_STAT_EPISODES = 2,    /* episodes that ended in this window (game_over,
                              bin_packing.h:94-101; rl.h:341-346)            */
  XH_STAT_EPLEN_SUM = 3,   /* over those episodes: length in env steps, the
                              overflowing step included, counted across
                              windows and the forget() shift (rl.h:274-291)  */
  XH_STAT_EPLEN_SQSUM = 4, /* ... and its square                             */
  XH_STAT_REWARD_SUM = 5,  /* reward of the window: 1 per step, 0 on the
                              overflowing step (bin_packing.h:102-106) =
                              transitions - dones; an episode's return is its
                              length - 1                                     */
  XH_STAT_NEGLOGP_SUM = 6, /* sum of -log((double)p_old) over the window
                              (XH_BUF_POLD: distrib[choice], rl.h:27-30); its
                              mean estimates the sampling policy's entropy   */
  /* -- learner part (learn()), summed over ranks: over the T * N
        transition rows of update_value_model / calculate_advantage
        (policy_gradient.h:196-281) -- */
  XH_STAT_VERR_SUM = 7,    /* target - V0: XH_BUF_TARGETS - XH_BUF_V_STATE0
                              (the value step's -dL/dV, nn.h:548-550)        */
  XH_STAT_VERR_SQSUM = 8,  /* its square: / rows = the value loss (mean
                              squared error of the pre-update values)        */
  XH_STAT_TARGET_SUM = 9,  /* TD target (policy_gradient.h:205-215)          */
  XH_STAT_TARGET_SQSUM = 10,
  XH_STAT_ADV_SUM = 11,    /* XH_BUF_ADV as the policy epochs read it (after
                              xh_config.adv_normalize when that is on)       */
  XH_STAT_ADV_SQSUM = 12,
  /* -- learner part, job-wide after the gradient all-reduce -- */
  XH_STAT_PGRAD_SQ_FIRST = 13, /* squared L2 norm of the first epoch's policy
                              gradient (XH_BUF_POLICY_GRADS row 0;
                              optimize_action, policy_gradient.h:297-307)    */
  XH_STAT_PGRAD_SQ_LAST = 14,  /* ... of the last epoch's                     */
  XH_STAT_VGRAD_SQ = 15,   /* squared L2 norm of XH_BUF_VALUE_GRAD           */
  XH_STAT_KL_BETA = 16,    /* XH_KLPPO: the last epoch's new beta (XH_BUF_KL;
                              policy_gradient.h:310-335); NaN otherwise      */
  XH_STAT_KL_MEAN = 17,    /* XH_KLPPO: the last epoch's mean KL; NaN
                              otherwise                                      */
  /* -- learner part, job-wide: gradient clipping (xh_trainer_set_grad_clip);
        each NaN while clipping is off for its net -- */
  XH_STAT_PCLIP_STEPS = 18,     /* policy steps of this learn() with scale < 1 */
  XH_STAT_PCLIP_SCALE_MIN = 19, /* smallest policy scale of this learn(); 1 if
                                   no step was clipped                        */
  XH_STAT_VCLIP_SCALE = 20,     /* scale of the value step                     */
  XH_STAT_COUNT
};
/* history_rows > 0 (at most 2^20): statistics on, with a fresh device ring of
 * history_rows x XH_STAT_COUNT doubles and an int32 [N] array of running
 * episode lengths; every env's running length and the row counter restart at
 * zero.  0: off, buffers freed.  XH_PG: XH_ERR_INVALID (REINFORCE plays whole
 * episodes and reports XH_BUF_LEN).  xh_trainer_set_env_state on an env zeroes
 * its running length: the replaced state starts a new episode and the
 * replaced one is not counted as finished; xh_trainer_set_buffer(XH_BUF_BINS)
 * does the same for every env (XH_BUF_ITEMS alone changes no count).
 * In a world > 1 job every rank must switch statistics on and off at the same
 * point of its loop: the statistics add one all-reduce per phase, which has
 * to meet the same all-reduce on every other rank. */
int xh_trainer_set_stats(xh_trainer *t, int history_rows);
/* Rows written since statistics were switched on. */
int xh_trainer_stats_count(xh_trainer *t, long *total_rows);
/* Synchronises the stream and copies rows [first, first + count) to out
 * [count][XH_STAT_COUNT].  XH_ERR_INVALID for rows the ring has overwritten
 * (first < total - history_rows) or not written yet; XH_ERR_STATE when
 * statistics are off. */
int xh_trainer_get_stats(xh_trainer *t, long first, int count, double *out);

/* ------------------------------------------- PPO update diagnostics ---- */
/* What a learn() did to the policy, off by default: with them off no launch is
 * added and no buffer allocated.  With them on, every `every`-th learn() ends
 * with one more forward of the UPDATED policy over the batch's T * N
 * transitions (the rollout's forward with the sampler replaced by a record per
 * row), reduced on the device to one row of XH_UPD_COUNT doubles in a ring of
 * `history_rows` rows of its own (the statistics row above is unchanged).
 * Three launches and, with a communicator, one all-reduce of the seven sums;
 * no host synchronisation.  The forward runs on f16 pairs where the rollout
 * does (64 bins 2-D [128,128] and 32 bins 1-D [64,64], no wide slot, no
 * XH_ROLLOUT_KERNEL override) and on f32 MFMA otherwise -- at 128 bins always.
 *
 * Per row, with p_new the updated policy's probability of the action taken,
 * p_old = XH_BUF_POLD, A = XH_BUF_ADV as the epochs read it and eps =
 * clip_eps (csrc/xh_diag.h, the function the kernel compiles):
 *   r32     = p_new / p_old in f32, as the clipped loss forms it (rl.h:54-74)
 *   clipped = 1 where r32 > 1.0f + eps or r32 < 1.0f - eps
 *   surr    = min(clamp(r32, 1 - eps, 1 + eps) * A, r32 * A), f32: the
 *             surrogate objective (without the loss's factor -1)
 *   logr    = log((double)p_new) - log((double)p_old)
 *   k3      = ((double)p_new / (double)p_old - 1) - logr
 *   H       = -sum_b p_b log((double)p_b) over the row's B probabilities
 *   KL      = sum_b q_b (log q_b - log p_b), q the sampling distribution: from
 *             XH_BUF_QOLD where the trainer records it (XH_KLPPO,
 *             record_distrib), else from the distributions PPO's epoch 0
 *             reuses when they were valid at this learn() (64 bins), else NaN
 * Nothing is masked: p_new == 0 gives logr = -inf, a NaN stays a NaN, and a
 * non-finite entry in a row is the signal that the policy collapsed.
 *
 * Sums are double, fixed order, no floating-point atomics: a row is
 * bit-identical from run to run.  -LOGR_SUM / ROWS is the usual approximate
 * KL(old || new), LOGR_SQSUM / (2 ROWS) and K3_SUM / ROWS its lower-variance
 * forms, CLIPPED / ROWS the clip fraction. */
enum { XH_UPD_LEARN = 0,       /* learn() calls since the diagnostics were set, this one's index */
       XH_UPD_ROWS = 1,        /* T * num_envs_global */
       /* summed over ranks, contiguous: */
       XH_UPD_LOGR_SUM = 2, XH_UPD_LOGR_SQSUM = 3, XH_UPD_K3_SUM = 4,
       XH_UPD_CLIPPED = 5, XH_UPD_SURR_SUM = 6, XH_UPD_ENTROPY_SUM = 7,
       XH_UPD_KL_SUM = 8,      /* NaN when no distributions were recorded */
       XH_UPD_COUNT };
/* history_rows > 0 (at most 2^20) with every >= 1: diagnostics on, with a
 * fresh ring and fresh record buffers (f32 + 2 f64 per transition); the learn
 * counter restarts at 0 and learn() number k is probed when k % every == 0.
 * history_rows == 0: off, buffers freed.  xh_trainer_forget is no learn().
 * XH_PG: XH_ERR_INVALID.  In a world > 1 job every rank sets the same values
 * at the same point of its loop (the all-reduce has to meet its peers). */
int xh_trainer_set_update_diag(xh_trainer *t, int history_rows, int every);
/* Rows written (probed learns) since the diagnostics were switched on. */
int xh_trainer_update_diag_count(xh_trainer *t, long *total_rows);
/* Synchronises the stream and copies rows [first, first + count) to out
 * [count][XH_UPD_COUNT].  XH_ERR_INVALID for rows the ring has overwritten or
 * not written yet; XH_ERR_STATE when the diagnostics are off or no probed
 * learn() has run. */
int xh_trainer_get_update_diag(xh_trainer *t, long first, int count, double *out);
/* The per-row records of the last probed learn(), [T][N] each: p_new, H, KL
 * (NaN without distributions).  Synchronises. */
int xh_trainer_get_update_diag_rows(xh_trainer *t, float *p_new, double *entropy,
                                    double *kl, size_t n);   /* last probed learn, n = T*N; any may be NULL */
/* JSON {"kernel": name|null, "math": "f32_mfma"|"f16_pair", "kl_source":
 * "qold"|"e0_p"|null, "history_rows": n, "every": n}: what the last probed
 * learn() ran (kernel null before the first). */
int xh_trainer_update_diag_info(xh_trainer *t, char *buf, size_t cap);

/* ------------------------------------------------------ trainer state ---- */
/* Everything a run has learned or consumed, as one flat buffer: a run that is
 * saved, destroyed, restored into a new trainer and continued produces the
 * bits of the run that was never interrupted (every sum of rollout() and
 * learn() is formed in a fixed order).  Opt-in: without these calls rollout()
 * and learn() launch what they launch without them and nothing is allocated.
 *
 * STATE (saved and restored):
 *   - both nets' flat parameters (XH_PG: the policy only);
 *   - per net the optimizer as xh_trainer_set_optimizer and
 *     xh_trainer_set_learning_rate left it: kind, lr, weight decay, beta1,
 *     beta2, the step counter t, and the device velocity / moments (absent
 *     for sgd);
 *   - XH_KLPPO's adaptive beta;
 *   - the [N] per-env engine states (XH_BUF_RNG);
 *   - the env states the next rollout starts from, [N][B][D] bins and [N][4]
 *     items, resolved as xh_trainer_get_env_state resolves them (slot T after
 *     a learn(), slot 0 otherwise, pending xh_trainer_set_env_state overrides
 *     applied; XH_PG: the slot its last rollout ended in);
 *   - the running episode lengths behind XH_STAT_EPLEN_*, while statistics
 *     are on (the section is absent while they are off).
 * SETTINGS (stay the loading trainer's own): the hyperparameter fields of
 * xh_config (gamma, lambda, clip_eps, kl_target, adv_normalize,
 * lr_scale_rows, the record_* flags), the gradient-clip thresholds, the
 * statistics and update-diagnostics rings with their row counters
 * (XH_STAT_ITER and the `every` phase restart in a new trainer), timing and
 * forced actions.
 *
 * THE BLOB: little-endian, written to a file as it is.
 *   [0, 144)       xh_state_header: magic "XHS1", version, its own size, the
 *                  section count, the blob's total byte count, the digest of
 *                  the payload = bytes [144, total_bytes), and the saving
 *                  trainer's xh_config
 *   [144, ...)     the section table: `sections` x xh_state_section {id,
 *                  offset from the blob's start, bytes, digest of those
 *                  bytes}, ids strictly increasing
 *   then           the sections, each starting at a multiple of 16 (zero
 *                  padding between them)
 * Section ids 0 .. XH_DIG_COUNT - 1 are the XH_DIG_* arrays below, copied as
 * they lie in device memory (f32 parameters and moments, int8 bins and items,
 * uint32 engine states, f32 beta); XH_SEC_OPT: for the policy then the value
 * net {int32 kind, f32 lr, wd, beta1, beta2, t, 2 x uint32 0}; XH_SEC_EP_LEN:
 * int32 [N].
 *
 * THE DIGEST of a buffer, over its 32-bit little-endian words w_i (a byte tail
 * zero-padded to a word), i = 0, 1, ...:
 *   digest = sum_i splitmix64(((uint64)i << 32) | w_i)   mod 2^64
 *   splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) *
 *   0xBF58476D1CE4E5B9; x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *   return x ^ (x >> 31)
 * The sum depends on every word's position (swapping two different words
 * changes it) but not on the order of the additions, which are integers mod
 * 2^64: the device forms it in a reduction tree (digest_kernels.hip),
 * xh_digest_host in a loop, with the same result.  It detects corruption and
 * misplaced writes; it is not a cryptographic hash. */
#define XH_STATE_VERSION 1
#define XH_STATE_MAGIC 0x31534858u /* "XHS1" */
enum { XH_STATE_ALL = 0, XH_STATE_NETS = 1 };
typedef struct {
  uint32_t magic, version, header_bytes, sections;
  uint64_t total_bytes, payload_digest;
  xh_config cfg;
  uint32_t reserved; /* 0 */
} xh_state_header;   /* 144 bytes: xh_struct_size("xh_state_header") */
typedef struct {
  uint32_t id, reserved; /* reserved: 0 */
  uint64_t offset, bytes, digest;
} xh_state_section;  /* 32 bytes: xh_struct_size("xh_state_section") */

enum { XH_DIG_POLICY_PARAMS = 0, XH_DIG_VALUE_PARAMS = 1,
       XH_DIG_POLICY_OPT_M = 2, XH_DIG_POLICY_OPT_V = 3,
       XH_DIG_VALUE_OPT_M = 4, XH_DIG_VALUE_OPT_V = 5, XH_DIG_ENV_BINS = 6,
       XH_DIG_ENV_ITEMS = 7, XH_DIG_RNG = 8, XH_DIG_KL_BETA = 9,
       XH_DIG_COUNT };
/* blob sections that are no device array of the digest call */
enum { XH_SEC_OPT = 10, XH_SEC_EP_LEN = 11, XH_SEC_COUNT };

/* Bytes xh_trainer_save_state writes for the trainer as it stands (it grows
 * with a non-sgd optimizer and with statistics on).  0 for null. */
size_t xh_trainer_state_bytes(const xh_trainer *t);
/* Synchronises the trainer's stream and writes the blob into blob[cap];
 * *written (may be NULL) = its size.  Only at an iteration boundary:
 * XH_ERR_STATE while a rollout window exists that no learn() / forget() has
 * consumed; a fresh trainer that has not rolled out yet can be saved.
 * XH_ERR_INVALID when cap is too small. */
int xh_trainer_save_state(xh_trainer *t, void *blob, size_t cap, size_t *written);
/* Restores a blob.  All-or-nothing: the whole blob is validated before the
 * first device write (magic, version, sizes against this trainer, every
 * section's bounds, the payload digest, bin values <= capacity and items that
 * are item-table entries, as xh_trainer_set_env_state checks them), and a
 * refused load leaves the trainer exactly as it was.
 *   what = XH_STATE_ALL: algo, bins, dims, steps, epochs, the four hidden
 *     widths and num_envs_global must equal the trainer's (XH_ERR_INVALID
 *     naming the first field that differs), and the blob's env slice
 *     [env_offset, env_offset + num_envs) must cover the trainer's; of a
 *     larger slice the trainer takes its own sub-range, so one checkpoint of
 *     a global batch restores into the trainers of its shards.  With
 *     statistics on, a blob without running episode lengths restarts them at
 *     zero.  XH_ERR_STATE while an unconsumed rollout window exists.
 *   what = XH_STATE_NETS: parameters, optimizers and beta only; the algo
 *     family (XH_PG or not), bins, dims and the hidden widths must match.
 *     Envs, engine states, episode lengths, num_envs and steps are untouched
 *     (continuing with a larger batch; handing nets to an evaluation trainer).
 * An accepted load uploads on the trainer's stream, drops pending
 * xh_trainer_set_env_state overrides (the restored states replace them),
 * allocates optimizer moments as xh_trainer_set_optimizer would, and then
 * digests every restored array on the device and compares it with the blob's
 * digest of it: XH_ERR_HIP naming the section on a mismatch (an upload that
 * did not land as ordered). */
int xh_trainer_load_state(xh_trainer *t, const void *blob, size_t bytes, int what);
/* Host only (no device, no trainer): parses a blob and writes one JSON object
 * {"version", "bytes", "config": {the saved xh_config}, "sections": [{"id",
 * "name", "bytes", "digest" (16 hex digits)}, ...]} NUL-terminated into
 * buf[cap].  XH_ERR_INVALID for a malformed blob: too short, bad magic,
 * unknown version, a section past the end, a payload digest mismatch. */
int xh_state_describe(const void *blob, size_t bytes, char *buf, size_t cap);
/* out[XH_DIG_COUNT] = the digests of the trainer's state arrays as they lie
 * in device memory (one launch pair; synchronises): what load verifies, and
 * what the ranks of a job compare to see that their replicated parameters and
 * optimizer state hold the same bits, in 80 bytes.  Absent arrays give 0
 * (sgd's moments, beta outside XH_KLPPO, the value net of an XH_PG trainer).
 * XH_ERR_STATE while xh_trainer_set_env_state overrides are pending: the
 * device does not hold those states yet. */
int xh_trainer_state_digest(xh_trainer *t, uint64_t *out /* [XH_DIG_COUNT] */);
/* The digest above of `bytes` bytes of host memory (data may be NULL for 0
 * bytes: digest 0). */
int xh_digest_host(const void *data, size_t bytes, uint64_t *out);

/* ------------------------------------------------- vectorised envs ---- */
/* N bp::environment instances (bin_packing.h:46-85, generalised to B bins /
 * D dims as the trainer's) whose state stays in HBM, for a caller that brings
 * its own policy: xylo::environment<A,S>::apply / view / reset
 * (rl.h:163-170) with the id parameter ranging over the whole batch, and
 * xylo::agent::step minus the policy's react (rl.h:325-349) as ONE kernel for
 * every env.
 *
 * Buffers (device memory owned by the venv; xh_venv_device_ptr gives the
 * address for the caller's own kernels on the same device, xh_venv_get /
 * xh_venv_set copy to / from host memory):
 *   XH_VENV_ACTIONS int32 [N]        the chosen bin of every env (input)
 *   XH_VENV_REWARD  f32   [N]        agent::get_reward of the last step
 *   XH_VENV_DONE    uint8 [N]        agent::game_over after the last apply
 *   XH_VENV_BINS    int8  [N][B][D]  bins (observation::bins)
 *   XH_VENV_ITEMS   int8  [N][4]     item, D used (observation::item)
 *   XH_VENV_RNG     uint32 [N]       per-env minstd_rand0 state
 *   XH_VENV_OBS     f32   [N][B][2D] observation::to_vector (bin_packing.h:
 *                                    31-40), written by xh_venv_observe and
 *                                    by xh_venv_step(write_obs = 1)
 *   XH_VENV_MASK    uint8 [N]        env selection for apply / reset
 *   XH_VENV_POLICY  f32   [N][B]     the caller's policy output for the
 *                                    current states (input of xh_venv_act)
 *   XH_VENV_PCHOICE f32   [N]        probability of the bin xh_venv_act chose
 * POLICY and PCHOICE are allocated (zero-filled) at their first use through
 * xh_venv_set / get / device_ptr or xh_venv_act; xh_venv_bytes gives their
 * sizes at any time.
 *
 * Engine draws: construction 2 per env, get_item 2, reset 2.
 * Env g of the job (env_offset + local index) starts on the global engine
 * stream at x0, constructed in env order, and xh_venv_step reproduces the
 * reference's draw order of a driver that steps every agent once per step in
 * env order, its policy taking `policy_draws` draws per step (2 for the
 * reference's discrete_action sampling and random_policy, 0 for a policy that
 * draws nothing): step s of env g draws at 2 Ng + k (s Ng + g), k =
 * policy_draws + 2.  xh_venv_apply / xh_venv_reset draw from the env's own
 * stream where it stands (with Ng = 1 every call sequence is exactly the
 * single-env reference engine).
 *
 * The problem instance -- the item shapes, their probabilities and the bins'
 * capacity -- is the reference's unless the venv is given an xh_item_set
 * (xh_venv_create_ex / xh_venv_set_item_set below): up to XH_ITEMS_MAX shapes
 * with weights and a capacity per dim, drawn from the same stream positions.
 *
 * Calls are asynchronous on the context's stream; an out-of-range action
 * leaves its env untouched and is reported by the next xh_venv_synchronize
 * (or get) as XH_ERR_INVALID. */
typedef struct xh_venv xh_venv;
enum {
  XH_VENV_ACTIONS = 0, XH_VENV_REWARD = 1, XH_VENV_DONE = 2,
  XH_VENV_BINS = 3, XH_VENV_ITEMS = 4, XH_VENV_RNG = 5, XH_VENV_OBS = 6,
  XH_VENV_MASK = 7, XH_VENV_POLICY = 8, XH_VENV_PCHOICE = 9, XH_VENV_BUF_COUNT
};
int xh_venv_create(xh_ctx *ctx, int num_envs, int bins, int dims,
                   uint32_t rng_state, int env_offset, int num_envs_global,
                   int policy_draws, xh_venv **out);
int xh_venv_destroy(xh_venv *v);
size_t xh_venv_bytes(const xh_venv *v, int which);
void *xh_venv_device_ptr(xh_venv *v, int which);
int xh_venv_get(xh_venv *v, int which, void *host, size_t bytes);
int xh_venv_set(xh_venv *v, int which, const void *host, size_t bytes);
/* Item sets and bin capacity.  xh_venv_create runs the reference's instance:
 * two items drawn bernoulli(0.4) -- (4) / (1), (4,2) / (1,2), (4,2,2) /
 * (1,2,1) at D = 1, 2, 3 -- and capacity 8 in every dim.  An xh_item_set
 * describes another: K shapes with weights, and a capacity per dim.
 *
 * The draw is the K-way form of bernoulli's u < p on the same u =
 * generate_canonical<double> (two engine draws, so every stream position of
 * the section above stays what it is): the item is the first k with u < c_k.
 * The thresholds are computed on the host in double: W = the sequential sum
 * of the weights, c_k = c_(k-1) + w_k / W with c_(-1) = 0, and c_k = 1.0
 * exactly from the last item of positive weight on (so c_(K-1) = 1.0, and
 * trailing zero weights cannot pick up the last rounding error).  A zero-weight
 * item is never drawn.  Weights {0.4, 0.6} give c = {0.4, 1.0}: the default set
 * draws bit for bit what bernoulli(0.4) draws.  xh_item_set_thresholds writes
 * those K doubles (host only, no device).
 *
 * Capacity is per dim: a reset fills bins[b][d] = capacity[d], and OBS (and
 * xh_venv_record_obs) is float(bins[b][d]) / float(capacity[d]) and
 * float(item[d]) / float(capacity[d]), IEEE f32 divisions (at capacity 8 the
 * bits of the builtin instance).  The upper limit 64 keeps two consecutive
 * xh_venv_apply calls on one bin inside int8; beyond that (applies to an env
 * that is over and is never reset) a bin wraps, as it does at capacity 8.
 * xh_venv_set(XH_VENV_BINS) refuses a value above its dim's capacity.
 *
 * A set is valid when K is in 1..XH_ITEMS_MAX, every capacity[d < D] in 1..64,
 * every item[k][d < D] in 0..capacity[d] with at least one entry above 0 (an
 * all-zero item's episodes would never end), and every weight is finite and
 * >= 0 with a sum above 0.  Entries past D and past K are ignored.  Anything
 * else is XH_ERR_INVALID, and nothing is allocated or changed.
 *
 * xh_venv_create_ex: items == NULL is xh_venv_create exactly (the same
 * kernels, launches and bits).  Any non-NULL set runs the general kernels,
 * also when it equals the default set.
 * xh_venv_set_item_set switches the set (a curriculum): ordered on the
 * context's stream like every call, it takes effect from the next draw; the
 * items the envs hold stay and no stream position moves.  The capacity must
 * equal the venv's (XH_ERR_INVALID otherwise: the stored bins are in its
 * units).  On a venv created without a set it switches that venv to the
 * general kernels.  xh_venv_get_item_set returns the set in use (the default
 * set for a venv created without one).
 * The trainer, xh_config, the evaluators and xh_heuristic_evaluate keep the
 * reference's instance; the venv's own heuristics (xh_venv_act_heuristic)
 * run on the venv's set and capacities. */
enum { XH_ITEMS_MAX = 16 };
typedef struct {
  int num_items;                 /* K, 1..XH_ITEMS_MAX                      */
  int capacity[4];               /* per dimension, first D used, 1..64      */
  int item[XH_ITEMS_MAX][4];     /* shapes, first D entries used            */
  double weight[XH_ITEMS_MAX];   /* >= 0, finite, sum > 0                   */
} xh_item_set;                   /* xh_struct_size("xh_item_set")           */
/* make_env's two items, weights 0.4 / 0.6, capacity 8 (dims outside 1..3: an
 * all-zero, invalid set) */
void xh_item_set_default(xh_item_set *s, int dims);
int xh_item_set_thresholds(const xh_item_set *s, int dims, double *out /*[K]*/);
int xh_venv_create_ex(xh_ctx *ctx, int num_envs, int bins, int dims,
                      uint32_t rng_state, int env_offset, int num_envs_global,
                      int policy_draws, const xh_item_set *items,
                      xh_venv **out);
int xh_venv_set_item_set(xh_venv *v, const xh_item_set *s);
int xh_venv_get_item_set(const xh_venv *v, xh_item_set *out);
/* agent::step minus react for every env: skip the policy's draws,
 * environment::apply(ACTIONS[e]), REWARD / DONE, reset on game over;
 * write_obs != 0 also writes OBS of the resulting states. */
int xh_venv_step(xh_venv *v, int write_obs);
/* The policy's react and agent::step in one launch: per env, pick a bin from
 * the caller's policy row (policy_gradient_policy::react,
 * policy_gradient.h:343-350), then do what xh_venv_step does with it.
 *
 * policy_dev: N*B floats on the context's device, 16-byte aligned (e.g. from
 * xh_tensor_alloc), the caller's writes ordered before the call; NULL reads
 * XH_VENV_POLICY.
 * kind: XH_ACT_PROBS, the rows as given, or XH_ACT_LOGITS, an f32 softmax with
 *   a max shift: e_j = expf(z_j - max z), p_j = e_j / se, where se adds each
 *   run of 16 consecutive bins (all of them at 8 bins) in bin order and then
 *   the runs' sums by an xor butterfly (partners 1, 2, 4).
 * mode: XH_ACT_SAMPLE, std::discrete_distribution<size_t> over p[0..B) with
 *   u = generate_canonical<double> (rl.h:27-30): p to double, divided by the
 *   sequential double sum, sequential partial sums, the last entry 1.0, the
 *   lower bound of u; two draws from the env's stream where it stands, so the
 *   venv must have been created with policy_draws == 2 (XH_ERR_INVALID
 *   otherwise).  XH_ACT_ARGMAX, the first maximum of the row's values as
 *   given (ties to the lowest bin, tensor.cc:464-466); draws nothing and
 *   skips the venv's policy_draws as xh_venv_step does.
 * Out: ACTIONS[e] = the bin, PCHOICE[e] = p[bin] (for PROBS the bits of the
 * input entry), then apply, REWARD / DONE, reset on game over, the jump over
 * the other envs' draws, and OBS if write_obs != 0.
 * A row with a NaN, a negative probability or a sum that is zero or not
 * finite is refused: its env is left untouched (ACTIONS and PCHOICE too),
 * DONE[e] = 0, and the next xh_venv_synchronize / get returns
 * XH_ERR_INVALID.
 * With a record (xh_venv_set_record) the call also writes the record's slot
 * at the cursor and advances it; on a full record it returns XH_ERR_STATE. */
enum { XH_ACT_PROBS = 0, XH_ACT_LOGITS = 1 };
enum { XH_ACT_SAMPLE = 0, XH_ACT_ARGMAX = 1 };
int xh_venv_act(xh_venv *v, const float *policy_dev, int kind, int mode,
                int write_obs);
/* The reference's heuristic agents as an act of the venv: per env, pick a bin
 * by heuristic XH_HEUR_RANDOM / FIRSTFIT / BESTFIT / MINWASTE (random_policy
 * rl.h:305-316, firstfit_agent.cc, bestfit_agent.cc, minwaste_agent.cc) from
 * the env's own state, then do what xh_venv_act does after its pick -- one
 * launch, asynchronous on the context's stream, on every venv shape and on
 * the venv's own item set and capacities.  No policy row is read.
 *
 * Scores of bin b, with fits = bins[b][d] >= item[d] for every d < D (the
 * reference's policies, generalised to D dims, a capacity per dim and items
 * with zero entries):
 *   FIRSTFIT  fits ? 1.0f : 0.0f.
 *   BESTFIT   -1.0f where the bin does not fit; otherwise the f32 sum over d =
 *     0 .. D-1, in that order, of term_d = item[d] == 0 ? +0.0f :
 *     float(item[d]) / float(bins[b][d]), a correctly rounded IEEE f32
 *     division.  (The zero-entry rule is this library's: an xh_item_set allows
 *     item[k][d] == 0, where the reference's expression would form 0 / 0.)
 *   MINWASTE  -1.0f where the bin does not fit; otherwise, with r_d =
 *     bins[b][d] - item[d]: 0.0f when exactly one d has r_d == capacity[d] / 2
 *     (integer division) and every other d has r_d == 0, else 1.0f.
 * The pick of these three is the first maximum, ties to the lowest bin
 * (from_vector_deterministic); they draw nothing and skip the venv's
 * policy_draws as XH_ACT_ARGMAX does; PCHOICE[e] = 1.0f.
 * RANDOM is, bit for bit, xh_venv_act(XH_ACT_PROBS, XH_ACT_SAMPLE) on a row
 * whose B entries are all (float)(1.0 / B): two draws from the env's stream,
 * PCHOICE that entry's bits; XH_ERR_INVALID unless the venv has policy_draws
 * == 2.
 * No env can be refused: there is no caller row.
 *
 * After the pick everything is xh_venv_act's: ACTIONS, apply, REWARD / DONE,
 * reset on game over, the jump over the other envs' draws, OBS if write_obs
 * != 0, the record's slot at the cursor (action, p_old, reward, done and the
 * state before the step; XH_ERR_STATE on a full record) and the episode
 * counters while episode statistics are on.
 *
 * With the action mask on (xh_venv_set_action_mask) the call writes eff(e)
 * into the legal-word record as xh_venv_act does.  The three deterministic
 * picks are unchanged by it: in each of them every fitting bin scores above
 * every bin that does not fit (1 > 0; a sum of terms >= 0 with one > 0, or 0
 * or 1, > -1), so where legal(e) is not empty the first maximum lies in it,
 * and where it is empty eff(e) is all B bins.  RANDOM becomes uniform over
 * eff(e): the premasked constant row (+0.0f outside eff(e)) through the same
 * sampler, so PCHOICE stays (float)(1.0 / B).
 * With a distribution record on (xh_venv_set_record_distrib) the call returns
 * XH_ERR_STATE and launches nothing: a heuristic has no distribution to
 * record.  A heuristic outside the enum is XH_ERR_INVALID. */
int xh_venv_act_heuristic(xh_venv *v, int heuristic /* XH_HEUR_* */,
                          int write_obs);
/* The trajectory record, written by xh_venv_act's own launch (no further
 * launch, no host synchronisation).  steps = T > 0 allocates T slots
 * (zero-filled, cursor 0, replacing an earlier record); steps = 0 turns the
 * record off and frees it.  The call at cursor t writes slot t of
 *   XH_VREC_ACTION  int32 [T][N]        XH_VREC_PCHOICE f32 [T][N]
 *   XH_VREC_REWARD  f32   [T][N]        XH_VREC_DONE    uint8 [T][N]
 * and, with with_states != 0, the state before the step
 *   XH_VREC_BINS    int8  [T][N][B][D]  XH_VREC_ITEMS   int8 [T][N][4]
 * (the trainer's XH_BUF_ACTION / POLD / DONE / BINS / ITEMS layouts for slots
 * 0..T-1; the state after the last step is XH_VENV_BINS / ITEMS).  A refused
 * env's ACTION / PCHOICE / REWARD / DONE entries of the slot are zero; its
 * state entries hold its (unchanged) state.  xh_venv_step / apply / reset do
 * not record.  xh_venv_record_bytes is the whole array's size (0 with the
 * record off, or for the states without with_states); xh_venv_get_record
 * copies the whole array (slots from the cursor on hold what an earlier pass
 * left there, zeros at first). */
enum { XH_VREC_ACTION = 0, XH_VREC_PCHOICE, XH_VREC_REWARD, XH_VREC_DONE,
       XH_VREC_BINS, XH_VREC_ITEMS, XH_VREC_COUNT };
int xh_venv_set_record(xh_venv *v, int steps, int with_states);
int xh_venv_record_pos(xh_venv *v, int *pos);
int xh_venv_record_rewind(xh_venv *v);
size_t xh_venv_record_bytes(const xh_venv *v, int which);
void *xh_venv_record_ptr(xh_venv *v, int which);
int xh_venv_get_record(xh_venv *v, int which, void *host, size_t bytes);
/* The distribution record: with it on, the xh_venv_act call at cursor t also
 * writes distrib[t][e][0..B), the p[] it picked env e's bin from, from the same
 * launch (no further launch): for XH_ACT_LOGITS its softmax's output, for
 * XH_ACT_PROBS the bits of the input row; XH_ACT_ARGMAX records the same p.
 * So distrib[t][e][ACTION] has XH_VREC_PCHOICE's bits, and a refused env's row
 * is zeros, like its other record entries.  It is what XH_LOSS_KL_REGULATED
 * and kl_stats of xh_venv_policy_loss read (XH_BUF_QOLD of a trainer made with
 * record_distrib).  The act launch writes 4 B more bytes per env and step.
 *   on != 0 allocates the zero-filled f32 [T][N][B] block of the current
 *     record; XH_ERR_STATE without a record, or when the cursor is not 0 (every
 *     recorded slot is to have its distribution); at cursor 0 with the block
 *     on already, XH_OK and nothing done.
 *   on == 0 frees it.
 * xh_venv_set_record (any steps) drops the block, as it drops the record it
 * replaces; xh_venv_record_rewind keeps it.  The accessors follow the other
 * record arrays': _bytes is the whole block's size (0 when off), _ptr its
 * device address (NULL when off), xh_venv_get_record_distrib copies the whole
 * block (XH_ERR_INVALID when off or on another size). */
int xh_venv_set_record_distrib(xh_venv *v, int on);
size_t xh_venv_record_distrib_bytes(const xh_venv *v);
float *xh_venv_record_distrib_ptr(xh_venv *v);
int xh_venv_get_record_distrib(xh_venv *v, float *host, size_t bytes);
/* Invalid-action masking (opt-in; nothing in the reference masks, and with it
 * off every launch is what it was).  Bin b takes env e's current item iff
 * bins[b][d] >= item[d] for every d < D; any other pick ends the episode
 * (bp::environment::apply, agent::game_over).  legal(e) is that set of bins and
 * eff(e) = legal(e) if it is not empty, else all B bins: when nothing fits
 * every pick ends the episode and the row is used as given.
 *
 * With the mask on, xh_venv_act on rows R does, bit for bit, what the
 * unmasked call does on premask(R): entry k of env e's row outside eff(e) is
 * replaced by -inf under XH_ACT_LOGITS and by +0.0f under XH_ACT_PROBS, in
 * XH_ACT_SAMPLE and in XH_ACT_ARGMAX, right after the row is loaded and before
 * anything reads it; the refusal checks, the softmax, the pick, PCHOICE, the
 * recorded p_old and the distribution record are the unmasked call's text on
 * that row (expf(-inf - m) is exactly 0, m is the maximum of the legal
 * entries, adding zeros changes no sum).  So
 *   - a NaN in an illegal entry is not seen;
 *   - a probability row whose legal entries sum to zero is refused as a
 *     zero-sum row is;
 *   - XH_ACT_SAMPLE keeps std::discrete_distribution's one edge: with u = 0
 *     exactly it picks index 0 even at probability 0; the record then has p_old
 *     = 0 and xh_venv_policy_loss skips the row like a refused one.
 *
 * The sets are packed as uint32 words, W = max(1, B / 32) per env
 * (xh_venv_legal_words): bit b % 32 of word b / 32 is bin b.
 *
 * xh_venv_set_action_mask: off at creation.  on != 0 with a record whose
 *   cursor is not 0 is XH_ERR_STATE (every recorded slot is to have its words;
 *   xh_venv_record_rewind first).  While the mask is on and a record exists a
 *   zero-filled uint32 [T][N][W] block exists with it: xh_venv_set_record
 *   allocates and drops it with the record, xh_venv_record_rewind keeps it,
 *   on == 0 frees it.  The xh_venv_act call at cursor t writes slot t from its
 *   own launch (4 W more bytes per env and step): the eff(e) it masked with, a
 *   function of the state before the step, so also for a refused env.
 *   xh_venv_record_legal_bytes / _ptr / xh_venv_get_record_legal follow the
 *   _distrib accessors' contract.
 * xh_venv_legal: eff(e) of every env's current state, [N][W] words, in one
 *   asynchronous launch on the context's stream, with the mask on or off (for
 *   a caller that masks inside its own network, or evaluates).  out_dev is
 *   device memory aligned to 4 W bytes; NULL writes a buffer the venv owns,
 *   allocated at first use, whose address is xh_venv_legal_ptr(v).
 * xh_venv_policy_loss_masked: xh_venv_policy_loss on the minibatch's rows
 *   premasked the same way, bit for bit -- grad, probs_out, dvalue, stats and
 *   kl_stats.  Row j's set is legal_dev[q][0..W), gathered through the same
 *   index q as action and p_old ([total][W], 4 W more bytes per row); a row
 *   whose words are all zero is left unmasked, so a zero-filled array is safe.
 *   legal_dev == NULL takes the record's block: XH_ERR_STATE if there is none,
 *   and XH_ERR_INVALID unless a->action == a->p_old == NULL (the record's
 *   rows).  The softmax is still the one xh_venv_act compiled, so while the
 *   parameters have not moved every ratio is exactly 1.0f under masking too;
 *   gradient entries at masked bins are zeros (of either sign).
 *   xh_venv_policy_loss itself is unchanged. */
int xh_venv_legal_words(const xh_venv *v);
int xh_venv_set_action_mask(xh_venv *v, int on);
int xh_venv_legal(xh_venv *v, uint32_t *out_dev);
uint32_t *xh_venv_legal_ptr(xh_venv *v);
size_t xh_venv_record_legal_bytes(const xh_venv *v);
uint32_t *xh_venv_record_legal_ptr(xh_venv *v);
int xh_venv_get_record_legal(xh_venv *v, uint32_t *host, size_t bytes);
/* From a recorded window to the learner's minibatches, on the device.  P is
 * the record's cursor (xh_venv_record_pos), a row index is q = t N + e.  The
 * three calls are asynchronous on the context's stream; their pointer
 * arguments are device memory on the context's device, the caller's writes to
 * them ordered before the call.  They read the record and the venv's present
 * state and change neither.
 *
 * xh_venv_record_obs writes obs_dev[count][B][2D] f32, observation::to_vector
 * (eighths: exact) of the rows first .. first + count - 1 (rows_dev == NULL)
 * or of the rows rows_dev[first .. first + count - 1] (a shuffled minibatch).
 *   XH_VOBS_STATE: S_t from the record's slot t, t in [0, P]; slot P is the
 *     venv's present state (XH_VENV_BINS / ITEMS), the state after the last
 *     recorded step.
 *   XH_VOBS_NEXT: the successor row replay_buffer::sample_td gives transition
 *     q, t in [0, P): S_t+1 where DONE[q] == 0; where the row ended the
 *     terminal view E_t, slot t's bins with bins[ACTION[q]] -= item, shown
 *     with slot t's item (the state the value net must see for it).
 * XH_ERR_STATE without a record that holds the states (with_states == 0),
 * XH_ERR_INVALID if obs_dev is not 16-byte aligned (the kernel writes 16-byte
 * stores).  An index in rows_dev outside the view's rows leaves its output
 * row untouched and is reported by the next xh_venv_synchronize / get as
 * XH_ERR_INVALID, as an out-of-range action is.
 *
 * xh_venv_record_ends writes the ended transitions of slots [0, P): list_dev
 * [j] = t N + e, env-major (e ascending, then t), and *n_dev = their count.
 * list_dev holds P N ints.  Its scratch is allocated at the first call and
 * freed with the venv.
 *
 * xh_venv_advantages: generalised advantage estimates, TD(0) targets and
 * lambda returns of a window, all in f32, one rounding per operation:
 *     lg    = lambda * gamma
 *     vn    = done ? 0 : V(S_t+1)
 *     delta = (r + gamma * vn) - V(S_t)
 *     A_t   = done ? delta : delta + lg * A_t+1        (A_steps = 0)
 *     td_target_t     = r + gamma * (done ? v_term : V(S_t+1))
 *     lambda_return_t = A_t + V(S_t)                   (A_t un-normalised)
 * With the venv's own rewards (1, or 0 on the step that ended) these are the
 * trainer's advantages and value targets bit for bit.  normalize: A <- (A -
 * mean) / (std + 1e-8), population mean and std over the window's steps * N
 * rows, in double and rounded once.  It covers THIS venv's rows only: a job
 * sharded over several venvs (env_offset) normalises each shard by its own
 * moments; nothing is all-reduced.  stats' sums are in double in a fixed
 * order (no floating-point atomics): the same inputs give the same bits.
 * A row xh_venv_act refused has reward 0 and done 0 in the record and is
 * treated as any other row.
 * XH_ERR_INVALID: steps < 0, steps > 0 without reward and done, a null
 * values / adv; XH_ERR_STATE: steps == 0 without a record. */
enum { XH_VOBS_STATE = 0, XH_VOBS_NEXT = 1 };
typedef struct {
  int steps;               /* 0: the record's P slots; > 0: a window of the
                              caller's own, reward and done both required */
  const float   *values;   /* [steps+1][N]  V(S_0 .. S_steps)               */
  const float   *v_term;   /* [steps][N] V(E_t), read only where done; NULL: 0 */
  const float   *reward;   /* [steps][N] or NULL: the record's              */
  const uint8_t *done;     /* [steps][N] or NULL: the record's              */
  float gamma, lambda;
  int normalize;           /* 1: A <- (A - mean)/(std + 1e-8) over steps*N rows */
  float *adv;              /* [steps][N] out                                */
  float *td_target;        /* out or NULL: r + gamma*(done ? v_term : V(S_t+1)) */
  float *lambda_return;    /* out or NULL: A_t (un-normalised) + V(S_t)     */
  double *stats;           /* out or NULL, device [4]: sum A, sum A^2 (both
                              before normalisation), rows, ended rows       */
} xh_venv_adv;             /* xh_struct_size("xh_venv_adv") */
int xh_venv_record_obs(xh_venv *v, int view, const int32_t *rows_dev,
                       long first, long count, float *obs_dev);
int xh_venv_record_ends(xh_venv *v, int32_t *list_dev, int32_t *n_dev);
int xh_venv_advantages(xh_venv *v, const xh_venv_adv *a);
/* The loss head of the caller's own network on a minibatch of the recorded
 * window: from the network's output rows to dL/d(output), one asynchronous
 * launch on the context's stream (plus a one-wave launch with stats).  It
 * reads the record and changes nothing of the venv's.  Every pointer is device
 * memory on the context's device.
 *
 * Output row j in [0, count) has the index q = rows_dev[first + j], or first +
 * j with rows_dev == NULL, into the [total] arrays adv, action, p_old and
 * target.  action / p_old == NULL take the record's XH_VREC_ACTION /
 * XH_VREC_PCHOICE, and total == 0 with both NULL is P * N.  A q outside [0,
 * total) or an action[q] outside [0, B) leaves row j of every output untouched
 * and is reported by the next xh_venv_synchronize / get as XH_ERR_INVALID, as
 * xh_venv_record_obs reports a bad index.
 *
 * Per row, with ch = action[q], q_old = p_old[q], A = adv[q], every f32
 * operation rounded once, in this order (no fused multiply-add):
 *   p: XH_ACT_PROBS the row as given; XH_ACT_LOGITS xh_venv_act's softmax,
 *     restated bit for bit: m = the row's maximum, e_k = expf(z_k - m), se =
 *     the sums of 16 consecutive e_k in bin order (all 8 at 8 bins), those
 *     sums added by an xor butterfly (partners 1, 2, 4), p_k = e_k / se.  So
 *     while the parameters have not moved (the first epoch) p_ch is the
 *     record's PCHOICE and the ratio below is exactly 1.0f.  probs_out, where
 *     not NULL, receives p.
 *   a skipped row: q_old <= 0 or NaN marks a row xh_venv_act refused (its
 *     record entries are zero).  grad[j] and dvalue[j] are zeros, the row adds
 *     1 to XH_VLOSS_SKIPPED and nothing else to the statistics; it is not an
 *     error (the refusal was reported when it happened).
 *   XH_LOSS_SOFTMAX_GRADIENT_LOG (policy_loss, rl.h:44-52): g_k = p_k * A,
 *     then g_ch = g_ch - A.  Through softmax_cross_entropy the same row is the
 *     logits' gradient, so both kinds give these bits from their p.
 *   XH_LOSS_CLIPPED (clipped_gradient, rl.h:54-74): ratio = p_ch / q_old;
 *     clipped = ratio > 1.0f + eps ? 1.0f + eps : ratio < 1.0f - eps ? 1.0f -
 *     eps : ratio; imp = min(clipped * A, ratio * A) * -1.0f; d = imp / p_ch.
 *     XH_ACT_PROBS: g_ch = d, every other entry 0.  XH_ACT_LOGITS:
 *     softmax_layer::backward (nn.h:393-416) on that one-hot backprop: quad =
 *     p_k * p_ch; pd = (k == ch ? p_k : 0.0f) - quad; g_k = pd * d.
 *   XH_LOSS_KL_REGULATED (kl_regulated_loss, policy_gradient.h:56-75, in
 *     xh_action_loss_grad's expressions): with the row's sampling distribution
 *     q = distrib[q] -- the caller's [total][B] array, or with distrib == NULL
 *     the record's (xh_venv_set_record_distrib) -- and beta = *beta_dev where
 *     beta_dev != NULL, the field beta otherwise:
 *       v = p_k * A;  if (k == ch) v = v - A;     softmax_gradient_log
 *       reg = (p_k - q_k) * beta;  v = v + reg;   + beta * (p - q)
 *       g_k = v
 *     As in the reference the net ends in softmax_cross_entropy, so both kinds
 *     give these bits from their p.  While the parameters have not moved p ==
 *     q bit for bit and the row is XH_LOSS_SOFTMAX_GRADIENT_LOG's.  eps is not
 *     read (but for stats).  beta_dev is read by the kernel, so a value
 *     xh_venv_kl_beta updates on the stream needs no host round trip.
 *   XH_LOSS_GRADIENT_LOG is XH_ERR_INVALID.
 *   grad[j][k] = g_k * scale.  scale = 1.0f is the reference's row-sum loss; a
 *     caller who wants the mean passes 1 / count.
 *   the value head, where values_new != NULL (square_loss_grad, nn.h:548-550):
 *     dv = values_new[j] - target[q], dvalue[j] = dv * value_scale.
 * grad may be policy itself (in place); any other overlap among policy, grad
 * and probs_out is XH_ERR_INVALID, as is one of them not 16-byte aligned (the
 * kernel moves 16-byte pieces).
 *
 * stats, where not NULL, receives the call's XH_VLOSS_* sums over the rows
 * that are neither skipped nor out of range: ROWS, SKIPPED, the sums of the
 * PPO update diagnostics' terms (xh_trainer_set_update_diag: log ratio, its
 * square, k3, clipped rows and the surrogate, from p_ch, q_old, A and eps;
 * eps is read for them under either loss), the entropy -sum_k p_k log p_k in
 * double (terms with p_k == 0 are 0), and dv and dv^2 in double (0 without
 * the value head).  All in double in a fixed order, no floating-point
 * atomics: the same inputs give the same bits.  accumulate != 0 writes old +
 * total instead, so an epoch's minibatches add up to one row in call order.
 * The block partials (4096 x XH_VLOSS_COUNT doubles) are allocated at the
 * first call with stats and freed with the venv.
 *
 * kl_stats, where not NULL, receives the XH_VKL_* sums under ANY loss kind
 * (clipped PPO's exact KL(old || new) too); it needs the rows' distributions
 * as XH_LOSS_KL_REGULATED does.  Over the rows that are neither skipped nor
 * out of range: ROWS, and with KL = sum_k q_k (log q_k - log p_k) in double
 * per row, KL_SUM = sum KL and KL_SQSUM = sum KL^2.  A term with q_k == 0 is
 * 0; nothing else is masked: p_k == 0 < q_k gives +inf and a NaN stays a NaN
 * (XH_UPD_KL_SUM's semantics).  The form differs from the reference's
 * kl_divergence, sum_k q_k log(q_k / p_k) (policy_gradient.h:41-54), by
 * rounding, and at q_k == 0, where the reference's 0 * log(0) is NaN.  Same
 * fixed-order double sums, no floating-point atomics; accumulate applies as
 * it does to stats; the block partials (4096 x XH_VKL_COUNT doubles) are
 * allocated at the first call with kl_stats.  The sums cover THIS venv's rows
 * only, as xh_venv_advantages' normalize does: nothing is all-reduced.
 * The order KL_SUM, ROWS is what xh_venv_kl_beta reads.
 *
 * XH_ERR_STATE: action or p_old NULL without a record.  XH_ERR_INVALID: a
 * null venv, args, policy, adv or grad; a kind or loss other than the above;
 * first < 0, count < 0, total < 0, or first + count > total without an index
 * list; eps not finite or not positive with XH_LOSS_CLIPPED; values_new
 * without target and dvalue; a misaligned pointer; a partial overlap;
 * XH_LOSS_KL_REGULATED or kl_stats with distrib == NULL and no recorded
 * distributions (or a total above the recorded rows); with
 * XH_LOSS_KL_REGULATED and beta_dev == NULL a beta that is negative or not
 * finite; distrib not 16-byte aligned, or overlapping grad or probs_out.
 * count == 0 returns XH_OK and launches nothing. */
enum { XH_VKL_KL_SUM = 0, XH_VKL_ROWS = 1, XH_VKL_KL_SQSUM = 2, XH_VKL_COUNT };
enum { XH_VLOSS_ROWS = 0, XH_VLOSS_SKIPPED, XH_VLOSS_LOGR_SUM,
       XH_VLOSS_LOGR_SQSUM, XH_VLOSS_K3_SUM, XH_VLOSS_CLIPPED,
       XH_VLOSS_SURR_SUM, XH_VLOSS_ENTROPY_SUM, XH_VLOSS_VERR_SUM,
       XH_VLOSS_VERR_SQSUM, XH_VLOSS_COUNT };
typedef struct {
  const float   *policy;     /* [count][B] the network's output for the rows  */
  int kind;                  /* XH_ACT_PROBS / XH_ACT_LOGITS                  */
  int loss;                  /* XH_LOSS_SOFTMAX_GRADIENT_LOG / XH_LOSS_CLIPPED */
  const int32_t *rows_dev;   /* index list or NULL: rows first .. first+count-1 */
  long first, count;
  const float   *adv;        /* [total] indexed by q                          */
  const int32_t *action;     /* [total] or NULL: the record's XH_VREC_ACTION  */
  const float   *p_old;      /* [total] or NULL: the record's XH_VREC_PCHOICE */
  long total;                /* 0 with action == p_old == NULL: P * N         */
  float eps, scale;
  const float *values_new;   /* [count] or NULL: no value head                */
  const float *target;       /* [total], required with values_new             */
  float value_scale;
  float *grad;               /* [count][B] out; may equal policy              */
  float *dvalue;             /* [count] out, required with values_new         */
  float *probs_out;          /* [count][B] out or NULL                        */
  double *stats;             /* device [XH_VLOSS_COUNT] out or NULL           */
  int accumulate;
  const float *distrib;      /* [total][B] sampling distributions indexed by q,
                                16-byte aligned; NULL: the record's
                                (xh_venv_set_record_distrib)                  */
  float beta;                /* KL_REGULATED: the regulation's weight ...     */
  const float *beta_dev;     /* ... or, where not NULL, one device float read
                                by the kernel (what xh_venv_kl_beta maintains) */
  double *kl_stats;          /* device [XH_VKL_COUNT] out or NULL; any loss kind */
} xh_venv_loss;              /* xh_struct_size("xh_venv_loss") */
int xh_venv_policy_loss(xh_venv *v, const xh_venv_loss *a);
/* the same on the rows premasked by their legal words (above) */
int xh_venv_policy_loss_masked(xh_venv *v, const xh_venv_loss *a,
                               const uint32_t *legal_dev);
/* xh_venv_policy_loss with the two terms every PPO learner adds to it: an
 * entropy bonus, -c * H(pi), and PPO2's clipped value loss.  Neither is in
 * the reference; both are opt-in through the extension block x, and xh_venv_
 * loss and its enums are as they were.
 *
 * The extension is off where x == NULL, or where ent_coef == 0, ent_coef_dev
 * == NULL, v_old == NULL and ext_stats == NULL.  The call is then
 * xh_venv_policy_loss(v, a) -- with x->masked != 0, xh_venv_policy_loss_
 * masked(v, a, x->legal_dev) -- itself: the same host path, the same kernel
 * instantiation, the same bits in every output, stats and kl_stats included.
 * Otherwise one launch of the instantiation that holds the extension (plus
 * the one-wave launches of stats, kl_stats and ext_stats) does what the plain
 * call does, premasked in the same way with masked, and in addition, every
 * f32 operation rounded once, in this order (no fused multiply-add):
 *
 * The entropy bonus, where ent_coef_dev != NULL or ent_coef > 0, with c =
 * *ent_coef_dev where given (read by the kernel: a schedule needs no host
 * round trip), the field ent_coef otherwise; under all three loss kinds, on
 * the row's p (XH_ACT_LOGITS: the softmax above):
 *   l_k = logf(p_k) where p_k > 0; a bin with p_k == 0 contributes nothing
 *   t_k = p_k * l_k
 *   S   = the sums of 16 consecutive t_k in bin order (all 8 at 8 bins), those
 *         sums added by the softmax's xor butterfly (partners 1, 2, 4); S =
 *         sum_k p_k log p_k <= 0 and the row's f32 entropy is -S
 *   XH_ACT_LOGITS: d = l_k - S; e = p_k * d; e = e * c   the gradient of
 *     -c * H(softmax(z)), c p_k (log p_k + H); a row's e sum to 0 but for
 *     rounding
 *   XH_ACT_PROBS:  d = l_k + 1.0f; e = d * c   the unconstrained partial of
 *     -c * H(p): the caller's own softmax sits behind it
 *   g_k = g_k + e, after the loss's own row g is formed and before grad[j][k]
 *     = g_k * scale.
 * e is 0 at a bin with p_k == 0 by a select, not by 0 * -inf; a masked bin has
 * p_k == 0 (its -inf logit gives exactly 0), so masked bins keep exact zero
 * gradients, and a row whose legal set is one bin has e == 0 throughout.  The
 * bonus does not touch p, so at epoch zero every ratio is still exactly 1.0f.
 * A skipped row stays all zeros.
 *
 * The clipped value loss, where v_old != NULL (it needs values_new), with vn =
 * values_new[j], tg = target[q], vo = v_old[q]:
 *   dl  = vn - vo
 *   hit = dl > vclip || dl < -vclip            |dl| == vclip is not a hit
 *   vc  = vo + (dl > vclip ? vclip : -vclip)   used only where hit
 *   e1  = vn - tg                              the plain call's dv
 *   e2  = vc - tg;  s1 = e1 * e1;  s2 = e2 * e2
 *   zero = hit && s2 > s1
 *   dvalue[j] = zero ? 0.0f : e1 * value_scale
 * the gradient of 0.5 * max((v - tg)^2, (v_clip - tg)^2), v_clip = vo + clamp(
 * v - vo, -vclip, vclip): the clipped branch does not depend on v once the
 * clip is hit.  The test is on hit, not on vc != vn -- vo + (vn - vo) need not
 * return vn, and an unclipped row never loses its gradient to that rounding.
 * A NaN compares false and propagates through e1; nothing is masked.
 * XH_VLOSS_VERR_SUM / _SQSUM stay the sums of e1.
 *
 * ext_stats, where not NULL, receives the XH_VEXT_* sums over the rows that
 * are neither skipped nor out of range: ROWS; ENTROPY_SUM = sum (double)(-S),
 * the f32 entropy the gradient used (0 without the bonus); VCLIP_ROWS, the
 * rows with zero; VLOSS_SUM = sum (zero ? (double)e2 * e2 : (double)e1 * e1),
 * twice the value loss (0 without the value head).  In double in a fixed
 * order, no floating-point atomics: the same inputs give the same bits.
 * a->accumulate applies as it does to stats; the block partials (4096 x
 * XH_VEXT_COUNT doubles) are allocated at the first call with ext_stats and
 * freed with the venv.  The sums cover THIS venv's rows only.
 *
 * XH_ERR_INVALID: a null venv; with ent_coef_dev == NULL an ent_coef that is
 * negative or not finite; v_old without a->values_new; v_old with a vclip that
 * is not finite and positive; legal_dev with masked == 0; and whatever
 * xh_venv_policy_loss[_masked] refuses, with its code. */
enum { XH_VEXT_ROWS = 0, XH_VEXT_ENTROPY_SUM, XH_VEXT_VCLIP_ROWS,
       XH_VEXT_VLOSS_SUM, XH_VEXT_COUNT };
typedef struct {
  int masked;                  /* != 0: premask as xh_venv_policy_loss_masked */
  const uint32_t *legal_dev;   /* with masked: the caller's words, NULL: the record's */
  float ent_coef;              /* >= 0, finite; the bonus's weight ...        */
  const float *ent_coef_dev;   /* ... or, where not NULL, one device float read
                                  by the kernel (a schedule with no host trip) */
  const float *v_old;          /* [total] indexed by q, the values at collection
                                  time; NULL: no value clipping                */
  float vclip;                 /* > 0, finite, with v_old                      */
  double *ext_stats;           /* device [XH_VEXT_COUNT] out or NULL           */
} xh_venv_loss_ext;            /* xh_struct_size("xh_venv_loss_ext") */
int xh_venv_policy_loss_ex(xh_venv *v, const xh_venv_loss *a,
                           const xh_venv_loss_ext *x);
/* kl_ppo_learner's beta rule (policy_gradient.h:76-80, 310-335) on the device:
 * one asynchronous single-thread launch on the context's stream.
 *   d = (float)(kl_stats_dev[XH_VKL_KL_SUM] / kl_stats_dev[XH_VKL_ROWS])
 *   beta halves where fabsf(d) < d_targ / 1.5f, doubles where fabsf(d) >
 *   d_targ * 1.5f, and is then clamped to [1e-25f, 0.1f].
 * A NaN d -- ROWS == 0 gives one -- compares false twice and leaves beta
 * unchanged apart from the clamp.  log_dev, where not NULL, receives {beta
 * before, d, beta after}.  The caller runs an epoch's minibatches with
 * accumulate (the first one without) and calls this once per epoch: the
 * reference's full-batch rule; the epoch's gradients used the beta from
 * before the update.  It is not bracketed by xh_venv_set_timing.
 * XH_ERR_INVALID: a null venv, kl_stats_dev or beta_dev; a d_targ that is not
 * finite or not positive. */
int xh_venv_kl_beta(xh_venv *v, const double *kl_stats_dev, float d_targ,
                    float *beta_dev, float *log_dev);
/* Logit tables: act and train on (bin state, item) instead of per-bin rows.
 *
 * A per-bin logit (xh_net's policy, or any network of the caller's that
 * shares its weights over the bins) depends on (bins[b][0..D), item[0..D))
 * alone.  Every bin value a venv stores lies in [0, capacity[d]] -- the launch
 * that takes a bin below zero resets the env -- and the item is one of the
 * set's K shapes, so the policy is a function on
 *   E = K * prod_d (capacity[d] + 1)
 * points: 162 for the reference's instance at D = 2, against N * B per-bin
 * rows per env step.  The domain (csrc/xh_venv_table.h):
 *   side[d] = capacity[d] + 1, S = prod_d side[d],
 *   s = (b0 * side[1] + b1) * side[2] + b2 with the unused dims dropped,
 *   e = k * S + s, k the first shape of the set equal to the item,
 * laid out as R = ceil(E / B) observation rows of B per-bin rows each, so the
 * network's own forward and backward run on it: flat per-bin row e of [R][B]
 * is entry e, the tail from E on is padding.  A venv created without a set
 * has xh_item_set_default's domain.  E is at most XH_VTAB_MAX_ENTRIES (a 3-D
 * venv at capacity 8 with 16 items has 11664): a set past it is
 * XH_ERR_INVALID, with a message that names E, from every call below, and such
 * a venv keeps the per-row chain.
 *
 * xh_item_set_table_info: host only, no device (as xh_item_set_thresholds):
 *   the domain of a valid set at dims / bins.  xh_venv_table_info: the same
 *   for the venv's present set.
 * xh_venv_table_obs: obs_dev [R][B][2 dims] f32, 16-byte aligned: row e is
 *   entry e's observation, float(b[d]) / float(capacity[d]) and float(item[d])
 *   / float(capacity[d]) as IEEE f32 divisions (OBS's expressions and bits);
 *   the rows from E on are zero.  xh_net_forward(n, obs_dev, R, table_dev)
 *   then leaves the table in table_dev's [R * B] floats.
 * xh_venv_act_table: xh_venv_act(XH_ACT_LOGITS, mode) on the row z[b] =
 *   table_dev[e(bins[b], item)], gathered inside the launch from the int8 bins
 *   the kernel holds anyway; no policy row is read.  Everything after the row
 *   is xh_venv_act's, bit for bit: the mask, the softmax, the sampler or the
 *   first maximum, apply, REWARD / DONE, the reset, the record's slot, the
 *   distribution record, the legal words, the episode counters and OBS; and so
 *   are its argument rules (policy_draws == 2 for XH_ACT_SAMPLE, XH_ERR_STATE
 *   on a full record).  table_dev: at least E floats, 4-byte aligned.
 * xh_venv_table_gather: out_dev [count][B] (16-byte aligned) = the logits of
 *   `count` rows of the record's XH_VOBS_STATE view, what xh_venv_policy_loss
 *   takes as XH_ACT_LOGITS.  rows_dev / first / count, the alignment rule and
 *   a bad index (its output row left untouched, XH_ERR_INVALID at the next
 *   xh_venv_synchronize) are xh_venv_record_obs's.
 * xh_venv_table_grad: g_dev [R * B] f32 (16-byte aligned) receives G[e] = the
 *   sum of dout_dev[j][b] ([count][B], 16-byte aligned, e.g. the loss head's
 *   grad) over the minibatch's (row, bin) pairs whose entry is e; entries no
 *   row touches and the tail from E on are 0.  accumulate != 0: g[e] += G[e],
 *   one f32 add per entry.  xh_net_backward(n, table_obs, R, g_dev, 0) then
 *   gives the parameter gradient of the whole minibatch -- or of an epoch
 *   accumulated into g_dev.  count >= 1.
 *   The sum is exact integer arithmetic (no floating-point atomics; the same
 *   bits from any grid and any order): with n = count * B, L the least integer
 *   with 2^L >= n, m = max |dout| over the count * B floats and ex the integer
 *   with 2^(ex-1) <= m < 2^ex: s = 62 - L - ex, q = llrint((double)dout * 2^s)
 *   (the product exact, the rounding to nearest even), the q of an entry added
 *   as 64-bit integers, G[e] = (float)((double)sum * 2^-s), both conversions to
 *   nearest even; m = 0 gives G = 0.  The error of an entry with n_e addends is
 *   at most n_e * 2^(-s-1) plus the two final roundings.
 *
 * Out-of-domain input never reads outside the table: an entry is formed only
 * from values that passed the checks.  A bin outside [0, capacity[d]]
 * (possible after xh_venv_apply without a reset, or xh_venv_set) or an item
 * that is none of the present set's shapes (possible after
 * xh_venv_set_item_set): xh_venv_act_table refuses the env as a bad policy row
 * is refused (untouched, DONE[e] = 0, the record's entries of a refused row),
 * gather and grad skip the row as a bad index is skipped, and a NaN or an
 * infinity in dout_dev leaves g_dev untouched; each is XH_ERR_INVALID at the
 * next xh_venv_synchronize / get.
 * A table stays valid while the set's shapes and capacities do: a curriculum
 * that only changes weights (zero weights included: a zero-weight item is a
 * legal shape that is never drawn) needs no new table; new weights of the
 * network need a new forward. */
#define XH_VTAB_MAX_ENTRIES 16384
struct xh_venv_table_info {      /* xh_struct_size("xh_venv_table_info")    */
  int entries;                   /* E                                       */
  int states;                    /* S                                       */
  int items;                     /* K                                       */
  int rows;                      /* R = ceil(E / bins)                      */
  int side[4];                   /* capacity[d] + 1; 1 past dims            */
};
int xh_item_set_table_info(const xh_item_set *s, int dims, int bins,
                           struct xh_venv_table_info *out);
int xh_venv_table_info(const xh_venv *v, struct xh_venv_table_info *out);
int xh_venv_table_obs(xh_venv *v, float *obs_dev);
int xh_venv_act_table(xh_venv *v, const float *table_dev, int mode,
                      int write_obs);
int xh_venv_table_gather(xh_venv *v, const float *table_dev,
                         const int32_t *rows_dev, long first, long count,
                         float *out_dev);
int xh_venv_table_grad(xh_venv *v, const int32_t *rows_dev, long first,
                       long count, const float *dout_dev, float *g_dev,
                       int accumulate);
/* environment::apply(ACTIONS[e], e) for the envs selected by MASK (all if
 * use_mask == 0), no reset; DONE[e] = game_over after the apply, 0 for the
 * envs this call did not apply (masked out, or an out-of-range action). */
int xh_venv_apply(xh_venv *v, int use_mask);
/* environment::reset(e) for the envs selected by MASK (all if use_mask == 0). */
int xh_venv_reset(xh_venv *v, int use_mask);
/* observation::to_vector of every env into OBS. */
int xh_venv_observe(xh_venv *v);
/* Waits for the venv's work; XH_ERR_INVALID if an action was out of range,
 * xh_venv_act refused a policy row or xh_venv_record_obs /
 * xh_venv_policy_loss met an index (the loss: or an action) outside its
 * range. */
int xh_venv_synchronize(xh_venv *v);
/* Kernel timing: on != 0 brackets every later step / act / apply / reset /
 * observe launch with HIP events on the context's stream (and drops the
 * events recorded so far); xh_venv_kernel_time returns their accumulated
 * milliseconds and the launch count.  xh_venv_record_obs and
 * xh_venv_record_ends are one bracket each; xh_venv_advantages is one
 * bracket around the scan (venv_gae_kernel) alone -- its statistics and
 * normalisation launches are not timed; xh_venv_policy_loss is one bracket
 * around the loss launch (venv_policy_loss_kernel) -- the one-wave launch
 * that reduces its statistics is not timed. */
int xh_venv_set_timing(xh_venv *v, int on);
int xh_venv_kernel_time(xh_venv *v, double *ms, long *launches);
/* Episode statistics, counted on the device (opt-in; off at creation, and
 * while off every launch computes and writes what it did without them and
 * nothing is allocated).  With them on, the xh_venv_step / xh_venv_act /
 * xh_venv_apply launches themselves count, per env, the steps of the episode
 * in flight -- every step of an env the call applied; an env that was masked
 * out, or whose action or policy row was refused, took no step and is not
 * counted.  Where the step ended the episode (DONE[e] = 1) the finished
 * length, the overflowing step included (what XH_STAT_EPLEN_SUM counts), goes
 * into the env's window accumulators, into the env's first-episode length if
 * it is the env's first since the switch-on, and the running length restarts
 * at 0.  xh_venv_apply does not reset the env, but it ends the episode where
 * it reports game over, so the caller's xh_venv_reset that follows changes
 * no count.  An episode's return in this env is its length - 1
 * (bin_packing.h:102-106), so no float is tracked.
 *
 * xh_venv_episode_row appends one row of XH_VEP_COUNT doubles to a device
 * ring of history_rows rows, asynchronously on the context's stream (a
 * reduction over the envs and a one-wave launch; fixed order, no atomics:
 * every entry is an exact integer, bit-identical from run to run), and clears
 * the window accumulators -- not the running lengths, not the first-episode
 * lengths:
 *   XH_VEP_ROW        rows taken since the switch-on (this row's index)
 *   XH_VEP_CALLS      step / act / apply launches counted into this row
 *   XH_VEP_EPISODES   episodes that ended in this row's span
 *   XH_VEP_LEN_SUM, XH_VEP_LEN_SQSUM   the sum of their lengths, of the squares
 *   XH_VEP_LEN_MIN, XH_VEP_LEN_MAX     NaN where EPISODES is 0
 *   XH_VEP_ENVS_FINISHED   envs with at least one finished episode since the
 *                     switch-on (cumulative)
 *   XH_VEP_FIRST_LEN_SUM, XH_VEP_FIRST_LEN_SQSUM   over those envs, each env's
 *                     first episode (cumulative): one episode per env, the
 *                     unbiased evaluation protocol of a vector env ("the
 *                     first K episodes to finish" over-represents short ones)
 *   XH_VEP_RUNNING_SUM, XH_VEP_RUNNING_MAX   the episodes in flight at the row
 * A row covers this venv's envs only: nothing is all-reduced.
 *
 * xh_venv_set_episode_stats: history_rows in [1, 2^20] gives a fresh ring and
 *   fresh per-env blocks -- every running length 0, every first length -1,
 *   the row counter 0 -- also when statistics are on already; 0 turns them
 *   off and frees everything.  An episode in flight at the switch-on is
 *   counted from that call on: switch on after xh_venv_create or a reset.
 * xh_venv_episode_count: rows taken so far.  xh_venv_get_episode_rows
 *   synchronises and copies rows [first, first + count) to out; XH_ERR_INVALID
 *   for a row that is overwritten or not yet written.  All three ring calls
 *   return XH_ERR_STATE while statistics are off.
 * The per-env state: XH_VEPS_RUNNING int32 [N], XH_VEPS_FIRST int32 [N] (-1:
 *   none yet).  xh_venv_episode_bytes is an array's size (0 while off),
 *   xh_venv_episode_ptr its device address (NULL while off), xh_venv_episode_
 *   get / _set copy from / to host memory (synchronising; `bytes` must be the
 *   array's size).  _set exists so that a run resumed from xh_venv_get / set
 *   of BINS / ITEMS / RNG continues its counts: take a row before saving (the
 *   window accumulators are not part of the saved state), and set BINS before
 *   the episode state.
 * State rules: xh_venv_reset zeroes the running length of the envs it resets
 *   (the abandoned episode is not counted); xh_venv_set(XH_VENV_BINS) zeroes
 *   every running length; XH_VENV_ITEMS, XH_VENV_RNG and xh_venv_record_rewind
 *   change no count.  xh_venv_destroy frees everything.  With xh_venv_set_
 *   timing on, xh_venv_episode_row is one bracket around its two launches. */
enum { XH_VEP_ROW = 0, XH_VEP_CALLS, XH_VEP_EPISODES, XH_VEP_LEN_SUM,
       XH_VEP_LEN_SQSUM, XH_VEP_LEN_MIN, XH_VEP_LEN_MAX, XH_VEP_ENVS_FINISHED,
       XH_VEP_FIRST_LEN_SUM, XH_VEP_FIRST_LEN_SQSUM, XH_VEP_RUNNING_SUM,
       XH_VEP_RUNNING_MAX, XH_VEP_COUNT };  /* xh_struct_size("xh_vep_row") */
enum { XH_VEPS_RUNNING = 0, XH_VEPS_FIRST, XH_VEPS_COUNT };
int xh_venv_set_episode_stats(xh_venv *v, int history_rows);
int xh_venv_episode_row(xh_venv *v);
int xh_venv_episode_count(xh_venv *v, long *total_rows);
int xh_venv_get_episode_rows(xh_venv *v, long first, int count, double *out);
size_t xh_venv_episode_bytes(const xh_venv *v, int which);
void *xh_venv_episode_ptr(xh_venv *v, int which);
int xh_venv_episode_get(xh_venv *v, int which, void *host, size_t bytes);
int xh_venv_episode_set(xh_venv *v, int which, const void *host, size_t bytes);

/* ------------------------------------------------------ model::eval -- */
/* xylo::model::eval (nn.h:473-479) of a layer chain on the device: rows x
 * cols host floats in, rows x out_cols host floats out.  Layers (nn.h):
 * full_layer (60-110) and convolution1d_1_layer (113-194, the same Dense
 * over each of the cols / in points of a row), relu (350-377), softmax
 * (379-422, no max shift) and softmax_cross_entropy (424-431, forward =
 * softmax).  params: the flat model::parameters() layout (nn.h:499-508).
 * Synchronous; for host-side callers of model::eval (the drop-in layer's
 * policies on host states, evaluation tools). */
enum { XH_LAYER_FULL = 0, XH_LAYER_CONV1D_1 = 1, XH_LAYER_RELU = 2,
       XH_LAYER_SOFTMAX = 3, XH_LAYER_SOFTMAX_XENT = 4 };
typedef struct {
  int kind;
  int in, out; /* dense layers: input / output features (per point) */
} xh_layer;
int xh_model_eval(xh_ctx *ctx, const xh_layer *layers, int nlayers,
                  const float *params, size_t nparams, const float *x,
                  int rows, int cols, float *out, size_t out_cap,
                  int *out_cols);

/* ------------------------------------- layer / model / optimizer / loss -- */
/* The reference's generic training API on the device, for callers that
 * assemble their own learner from its pieces (the drop-in layer's
 * xylo::layer / model / optimizer / loss functions, include/xylo_compat).
 * Synchronous; host arrays in and out; layers and the flat parameter layout
 * as xh_model_eval.
 *
 * xh_model_forward: model::forward (nn.h:481-488) -- the input and every
 * layer's output, each rows x widths[l], concatenated into acts (widths[0] =
 * cols, widths[nlayers] = the output's).  acts_cap floats; widths has
 * nlayers + 1 entries. */
int xh_model_forward(xh_ctx *ctx, const xh_layer *layers, int nlayers,
                     const float *params, size_t nparams, const float *x,
                     int rows, int cols, float *acts, size_t acts_cap,
                     int *widths);
/* model::gradient (nn.h:510-528): `inputs` = the first nlayers matrices of
 * model::forward, concatenated as xh_model_forward writes them; target =
 * dL/d(output), rows x target_cols.  Backpropagates from the last layer
 * (layer::gradient then layer::backward per layer, layer 0 gradient only)
 * into grad[nparams] (model::parameters() layout). */
int xh_model_gradient(xh_ctx *ctx, const xh_layer *layers, int nlayers,
                      const float *params, size_t nparams, const float *inputs,
                      int rows, int cols, const float *target, int target_cols,
                      float *grad);
/* layer::backward / layer::gradient (nn.h:20-33) of one layer: input rows x
 * cols, backprop rows x bp_cols (the layer's output width).  backward ->
 * out rows x cols (full / conv1d_1: backprop . A; relu: gated by input > 0;
 * softmax: the Jacobian product; softmax_cross_entropy: backprop itself);
 * gradient -> grad[ngrad], the layer's [dA (out x in), db (out)] (ngrad = 0
 * for activations). */
int xh_layer_backward(xh_ctx *ctx, const xh_layer *layer, const float *params,
                      size_t nparams, const float *input, int rows, int cols,
                      const float *backprop, int bp_cols, float *out);
int xh_layer_gradient(xh_ctx *ctx, const xh_layer *layer, const float *input,
                      int rows, int cols, const float *backprop, int bp_cols,
                      float *grad, size_t ngrad);
/* The discrete-action loss gradients of a batch of `rows` actions over
 * `range` choices, out[rows][range] (rl.h:33-74 per row):
 *   XH_LOSS_GRADIENT_LOG          discrete_action::gradient_log
 *   XH_LOSS_SOFTMAX_GRADIENT_LOG  softmax_gradient_log = policy_loss
 *                                 (policy_gradient.h:24-34)
 *   XH_LOSS_CLIPPED               clipped_gradient = surrogate_loss
 *                                 (:36-46), param = epsilon (0.2)
 *   XH_LOSS_KL_REGULATED          the gradient of kl_regulated_loss (:55-74):
 *                                 softmax_gradient_log + param (beta) times
 *                                 (probs - distrib); the beta adaptation is
 *                                 the caller's
 * choice[rows], advantage[rows], probs = the model's output rows (the
 * reference's orig_action_matrix), distrib = each action's sampling
 * distribution [rows][range] (unused by SOFTMAX_GRADIENT_LOG, may be NULL
 * there). */
enum { XH_LOSS_GRADIENT_LOG = 0, XH_LOSS_SOFTMAX_GRADIENT_LOG = 1,
       XH_LOSS_CLIPPED = 2, XH_LOSS_KL_REGULATED = 3 };
int xh_action_loss_grad(xh_ctx *ctx, int kind, int rows, int range,
                        const int32_t *choice, const float *distrib,
                        const float *advantage, const float *probs, float param,
                        float *out);
/* optimizer::next_parameters (nn.h:616-698) of n parameters in place:
 * XH_OPT_SGD p (1 - wd) - g lr; XH_OPT_MOMENTUM v = 0.9 v + g, p - v lr (m =
 * v); XH_OPT_ADAM moments m, v, bias-corrected with step t (1, 2, ...),
 * p - m^ lr / (sqrt(v^) + 1e-7).  m / v: the caller's state arrays (NULL for
 * sgd). */
int xh_optimizer_apply(xh_ctx *ctx, int kind, float lr, float weight_decay,
                       float beta1, float beta2, float t, float *params,
                       const float *grad, float *m, float *v, size_t n);
/* Global-norm clipping for a learner assembled from these pieces (next to
 * xh_optimizer_apply): the kernels and the formula of
 * xh_trainer_set_grad_clip with r = 1 on n host floats, scaled in place;
 * synchronous.  max_norm > 0 and finite.  *norm = sqrt(sum g[i]^2), *scale =
 * the factor applied (either may be NULL). */
int xh_clip_grad_norm(xh_ctx *ctx, float *grad, size_t n, float max_norm,
                      double *norm, float *scale);
/* replay_buffer::forget() (rl.h:274-291) after a learn() that did not run on
 * this trainer (a learner assembled from the pieces above consumed the
 * batch): the batch's final states become the next rollout's start states. */
int xh_trainer_forget(xh_trainer *t);

/* ------------------------------------ device-resident nets (xh_net) ---- */
/* The reference's two networks as device objects a venv learner calls: the
 * policy is the per-bin conv1d_1 chain 2D -> h1 -> relu -> h2 -> relu -> 1
 * (kind XH_NET_POLICY), the value net the full-layer MLP 2BD -> h1 -> relu ->
 * h2 -> relu -> 1 (XH_NET_VALUE), both in the flat model::parameters() layout
 * a trainer of the same shape uses, so parameters move between an
 * xh_trainer, a weights file and a net unchanged.  A net lives on a context
 * and is not bound to a venv: the item set and the capacities reach it only
 * through the observations.
 *
 * Shapes: bins in {8, 16, 32, 64, 128}, dims in {1, 2, 3}; policy widths
 * (h1, h2) in {(128,128), (128,64), (64,64), (64,32)}, value widths >= 1;
 * anything else is XH_ERR_INVALID at create.
 *
 * obs_dev: [rows][bins][2 dims] f32, what XH_VENV_OBS and xh_venv_record_obs
 * write.  Policy out_dev: [rows][bins] logits (no softmax: xh_venv_act with
 * XH_ACT_LOGITS and the loss head own it); value out_dev: [rows].  dout_dev
 * has out's shape and may be the block the loss head wrote in place.
 * xh_net_backward writes the parameter gradient of sum(dout * out) into
 * XH_NET_GRAD: accumulate = 0 overwrites, accumulate = 1 adds this call's
 * reduced sum to what is there (one f32 add per entry).  Layer 0 gets no data
 * gradient.  The policy runs fused (net_policy_fwd_kernel /
 * net_policy_bwd_kernel: exact f32 MFMA, per-workgroup slabs summed in a
 * fixed order, no floating-point atomics, the same bits from run to run); the
 * value net runs the layer launches of xh_model_forward / xh_model_gradient.
 * XH_NET_POLICY_LAYERS is the policy run through those layer launches as well
 * (conv1d_1 / relu / conv1d_1 / relu / conv1d_1 over rows * bins points, any
 * widths >= 1): every activation is materialised, rows * bins * (2 h1 + 2 h2)
 * floats of scratch and as much again for the backward.  It is the
 * comparator the fused kernels are measured against (tools/venv_net_time.py),
 * not a path to train on.
 *
 * xh_net_step: global-norm clipping when max_norm > 0 (the launches of
 * xh_trainer_set_grad_clip with r = 1; {norm, (double)scale} go to
 * clip_log_dev where that is not NULL), then the optimizer set by
 * xh_net_set_optimizer (sgd, lr 0 until then) on XH_NET_GRAD; max_norm = 0:
 * the optimizer launch alone, clip_log_dev untouched.  The step counter t
 * counts the steps taken (adam's bias correction uses t + 1);
 * xh_net_set_optimizer zeroes the moments and t.
 *
 * forward, backward and step are asynchronous on the context's stream and
 * neither synchronise nor allocate, except that the first call with more rows
 * than any before grows the net's scratch (one synchronisation then).
 * xh_net_get / xh_net_set copy n = xh_net_num_params floats and wait.
 * xh_net_set_grid_cap: test only, at most `cap` workgroups per policy launch
 * (0: the default).  xh_net_info: a JSON object {"kind", "kernels", "grid",
 * "grid_cap", "lds", "slabs"} describing the last forward / backward. */
typedef struct xh_net xh_net;
enum { XH_NET_POLICY = 0, XH_NET_VALUE = 1, XH_NET_POLICY_LAYERS = 2 };
enum { XH_NET_PARAMS = 0, XH_NET_GRAD, XH_NET_M, XH_NET_V, XH_NET_COUNT };
int xh_net_create(xh_ctx *ctx, int kind, int bins, int dims, int h1, int h2,
                  xh_net **out);
int xh_net_destroy(xh_net *n);
size_t xh_net_num_params(const xh_net *n);
int xh_net_get(xh_net *n, int which, float *host, size_t count);
int xh_net_set(xh_net *n, int which, const float *host, size_t count);
float *xh_net_device_ptr(xh_net *n, int which);
int xh_net_get_step(xh_net *n, long *t);
int xh_net_set_step(xh_net *n, long t);
int xh_net_forward(xh_net *n, const float *obs_dev, long rows, float *out_dev);
int xh_net_backward(xh_net *n, const float *obs_dev, long rows,
                    const float *dout_dev, int accumulate);
int xh_net_set_optimizer(xh_net *n, int kind, float lr, float weight_decay,
                         float beta1, float beta2);
int xh_net_step(xh_net *n, float max_norm, double *clip_log_dev);
int xh_net_set_grid_cap(xh_net *n, int cap);
int xh_net_info(xh_net *n, char *buf, size_t cap);

/* The value net read straight from a venv's recorded window (opt-in; fused:
 * net_value_fwd_kernel / net_value_bwd_kernel, exact f32 MFMA).
 * xh_net_forward_record(n, v, view, rows_dev, first, count, out_dev) replaces
 * xh_net_forward on the block xh_venv_record_obs(v, view, rows_dev, first,
 * count, obs) writes, call for call: view, rows_dev, first and count mean what
 * they mean there (XH_VOBS_STATE over (P + 1) N rows with slot P the present
 * state, XH_VOBS_NEXT over P N rows: the successor, or the terminal view where
 * the transition ended), output row j is the row record_obs writes as row j,
 * and each observation has record_obs's bits ((float)v / (float)capacity[d] of
 * the venv's item set, the default one without a set) -- formed in registers
 * from the int8 record: no f32 observation and no activation is written.
 * xh_net_backward_record is xh_net_backward on the same rows: the parameter
 * gradient of sum(dout * out) into XH_NET_GRAD, accumulate as there;
 * per-workgroup slabs summed in a fixed order, no floating-point atomics, the
 * same bits from run to run.  An index outside the view leaves out_dev[j]
 * untouched / adds nothing to the gradient and raises the venv's error bit
 * that xh_venv_record_obs raises (XH_ERR_INVALID at the next
 * xh_venv_synchronize).  Both are asynchronous on the context's stream; the
 * first backward allocates the slabs (one synchronisation then).
 * xh_net_set_grid_cap caps these launches too and xh_net_info describes them
 * ("kernels" names them once one has run).
 * XH_ERR_INVALID: n is not XH_NET_VALUE, its widths are not (64, 32), its bins
 * or dims are not the venv's, net and venv live on different contexts, count <
 * 0, out_dev / dout_dev NULL, or what xh_venv_record_obs refuses; XH_ERR_STATE:
 * the venv has no record.  count = 0 does nothing (a backward without
 * accumulate then zeroes XH_NET_GRAD).  Other widths keep the layer path
 * through xh_venv_record_obs. */
int xh_net_forward_record(xh_net *n, xh_venv *v, int view,
                          const int32_t *rows_dev, long first, long count,
                          float *out_dev);
int xh_net_backward_record(xh_net *n, xh_venv *v, int view,
                           const int32_t *rows_dev, long first, long count,
                           const float *dout_dev, int accumulate);

/* ---------------------------------------------------------- tensor ---- */
/* xylo/tensor.{h,cc} on the device, for the drop-in tensor type
 * (include/xylo_compat/xylo/tensor.h): tensors created with on_device = true
 * live in HBM (the reference's memory_blob on_device bit with its gpu_alloc /
 * gpu_dealloc stubs, tensor.cc:38-39, 78-102, made real), and their
 * arithmetic runs here; large operations on host tensors (GEMMs, long
 * reductions) stage through the device.  Every call is synchronous on the
 * context's stream.
 *
 * xh_tensor_alloc / free: n floats of device memory, zero-filled (NULL for
 * n = 0).
 * xh_tensor_copy: n floats, kind XH_COPY_H2D | XH_COPY_D2H | XH_COPY_D2D. */
enum { XH_COPY_H2D = 0, XH_COPY_D2H = 1, XH_COPY_D2D = 2 };
int xh_tensor_alloc(xh_ctx *ctx, size_t n, float **out);
int xh_tensor_free(xh_ctx *ctx, float *p);
int xh_tensor_copy(xh_ctx *ctx, float *dst, const float *src, size_t n,
                   int kind);
/* Elementwise, device arrays (tensor.cc:256-317 and the compound operators
 * :338-398): out[i] = a[i] + b[i] | a - b | a * b | a / b (XH_T_ADD ..
 * XH_T_DIVIDE); a[i] + s | a - s | a * s | a / s (XH_T_*_S); fabsf / sinf /
 * expf / logf / sqrtf of a[i]; XH_T_FILL: out[i] = s (vector::operator=(float),
 * tensor.cc:128); XH_T_RMINUS_S s - a[i] and XH_T_RDIVIDE_S s / a[i] (the
 * reference's compound v -= s and v /= s, whose bind_front puts the scalar
 * first: tensor.cc:378-380, 392-394).  out may alias a or b. */
enum { XH_T_ADD = 0, XH_T_MINUS = 1, XH_T_MULTIPLY = 2, XH_T_DIVIDE = 3,
       XH_T_ADD_S = 4, XH_T_MINUS_S = 5, XH_T_MULTIPLY_S = 6,
       XH_T_DIVIDE_S = 7, XH_T_ABS = 8, XH_T_SIN = 9, XH_T_EXP = 10,
       XH_T_LOG = 11, XH_T_SQRT = 12, XH_T_FILL = 13, XH_T_RMINUS_S = 14,
       XH_T_RDIVIDE_S = 15 };
int xh_tensor_map(xh_ctx *ctx, int op, const float *a, const float *b,
                  float scalar, float *out, size_t n);
/* Reductions over n floats (device arrays if on_device, else host arrays
 * staged for the call), accumulated in double and returned unrounded:
 * XH_R_SUM sum a (tensor.cc:434-438), XH_R_DOT sum a*b (:427-432), XH_R_SQDEV
 * sum (a - s)^2 (variance's sum about the mean s, :442-451), XH_R_MAX max a
 * (:462), XH_R_ARGMAX its first index (:464-466) in *index (may be NULL
 * otherwise).  max / argmax of n = 0 is XH_ERR_INVALID. */
enum { XH_R_SUM = 0, XH_R_DOT = 1, XH_R_SQDEV = 2, XH_R_MAX = 3,
       XH_R_ARGMAX = 4 };
int xh_tensor_reduce(xh_ctx *ctx, int op, const float *a, const float *b,
                     float scalar, size_t n, int on_device, double *value,
                     int64_t *index);
/* out[m][n] = sum_k a[m][k] b(n, k), f32 MFMA: XH_GEMM_NT b is [n][k]
 * (matmul_transposed, tensor.cc:218-227), XH_GEMM_NN b is [k][n] (matmul,
 * :228-230).  Row-major, no aliasing of out with a or b. */
enum { XH_GEMM_NT = 0, XH_GEMM_NN = 1 };
int xh_tensor_gemm(xh_ctx *ctx, int layout, const float *a, const float *b,
                   float *out, int m, int n, int k, int on_device);
/* out[cols][rows] = in[rows][cols]^T (transpose, tensor.cc:209-216). */
int xh_tensor_transpose(xh_ctx *ctx, const float *in, float *out, int rows,
                        int cols, int on_device);

/* sizeof of the ABI structs ("xh_config", "xh_eval", "xh_layer"; 0 if
 * unknown), so a
 * foreign-language binding can check its mirror of them.  "xh_stat_row": the
 * bytes of one statistics row, XH_STAT_COUNT * 8; "xh_upd_row": of one
 * update-diagnostics row, XH_UPD_COUNT * 8.  "xh_state_header" (144) and
 * "xh_state_section" (32): the fixed parts of a state blob. */
size_t xh_struct_size(const char *name);

/* Kernel timing with HIP events on the trainer's stream (off by default).
 * on = 1: every launch (the phase breakdown; the events themselves cost
 * about 2 us per launch of wall time); on = XH_TIMING_TRAIN (2): the policy
 * train launches only (the dominant kernel's average duration, nearly free). */
#define XH_TIMING_TRAIN 2
int xh_trainer_set_timing(xh_trainer *t, int on);
/* name: "rollout_step" | "policy_train" | "value" | "reduce_sgd" | "allreduce"
 * | "stats" (the statistics launches of xh_trainer_set_stats; their
 * all-reduces count under "allreduce") | "probe" (the three launches of a
 * probed learn(), xh_trainer_set_update_diag; its all-reduce counts under
 * "allreduce").
 * Returns accumulated milliseconds and launch count since the last reset. */
int xh_trainer_kernel_time(xh_trainer *t, const char *name, double *ms,
                           long *launches);
int xh_trainer_reset_timing(xh_trainer *t);
/* Which kernels the trainer's last rollout step and last policy epoch
 * launched, and their arithmetic, as a JSON object written NUL-terminated
 * into buf[cap]:
 *   {"rollout_step": K, "policy_train": K, "value": V, "train_grid": G,
 *    "train_grid_cap": C, "overrides": {...}}
 *   K = {"kernel": name | null (not launched yet),
 *        "math": one of
 *          "f32_mfma"             f32-input MFMA / f32 VALU: peak 157.3
 *          "bf16_split"           bf16 MFMA on exact three-part splits: 4
 *                                 products per f32 product in the train epoch
 *                                 (variant library only): peak 2500 / 4
 *          "f16_pair"             the split rollouts' layer 2 on scaled f16
 *                                 pairs, 3 products per f32 product: 2500 / 3
 *          "f16_pair_bf16_split"  the train epochs: layer 2 three f16
 *                                 products, dH1 two, dW2 three bf16 (8 per 3
 *                                 f32 products, equal FLOPs): 2500 / (8/3),
 *        "products_per_f32_product": p (null for f32_mfma),
 *        "bf16_products_per_f32_product": p for "bf16_split", else null,
 *        "peak_tflops": the dense MFMA peak of that arithmetic on MI355X
 *        (2500 / p, or 157.3)}
 *   policy_train_spec8_kernel (64 bins, 2-D, [128,128]; PPO / actor-critic)
 *   runs dW2 on scaled f16 pairs as well, two products: it keeps the
 *   "f16_pair_bf16_split" entries above (the yardstick its `frac` has been
 *   printed against) and adds "dw2_math": "f16_pair_per_feature_scale",
 *   "issued_math": "f16_pair_train", "issued_products_per_f32_product": 7/3
 *   and "issued_peak_tflops": 2500 / (7/3), what it actually issues.
 *   The "rollout_step" entry also carries "logit_table": true when the last
 *   rollout launch read its logits from the launch's table of (bin state,
 *   item) logits instead of running the forward per row (rollout_split_kernel
 *   at 64 bins, 2-D, [128,128]; off with XH_ROLLOUT_TABLE=0, for a launch
 *   that writes PPO's epoch-0 records, and for a trainer whose slot 0 has
 *   held a bin below -capacity); the same kernel name and arithmetic either
 *   way, and the same bits.  "envs_per_wave": the envs a wave of the
 *   register-stepping rollout steps at once -- 8 where the table launch runs
 *   (its packed kernel; XH_ROLLOUT_TABLE=1 selects the one-env-per-wave table
 *   launch, 1), 1 for rollout_split_kernel's other 64-bin launches, 2 at 32
 *   bins, 0 for any other kernel.
 *   V ="vnet_bf16" (the Fin -> 64 -> 32 -> 1 value net on exact bf16
 *   splits: two forwards and one fused backward per update, B*D % 16 == 0,
 *   B*D + D < 416), "mlp3_fused" (the same net on the f32 fused kernels:
 *   XH_VALUE_KERNEL=mlp3, or shapes the bf16 kernels do not take) or "gemm"
 *   (layer by layer: other widths, XH_VALUE_KERNEL=gemm),
 *   G = the train grid (workgroups, = gradient slabs), C = xh_config
 *   train_grid_cap.
 * "overrides" lists the diagnostic environment variables that steer kernel
 * selection (XH_TRAIN_KERNEL, XH_ROLLOUT_KERNEL, XH_VALUE_KERNEL) with their
 * values, or null when unset. */
int xh_trainer_kernel_info(xh_trainer *t, char *buf, size_t cap);

/* Tests and diagnostics only (synchronises the stream): how the last learn()
 * ran the 64-bin 2-D [128,128] PPO / actor-critic epochs over the packed batch
 * (duplicate rows of an env-step computed once): env-steps that ran packed
 * (at most 16 distinct bin states: a 16-row segment, four to a group),
 * env-steps that ran unpacked in the same launches (a 64-row group each) and
 * the groups each epoch's launch ran.  All three are 0 when the last learn()
 * did not run packed (XH_SP8_PACK=0, another shape or algorithm, a kernel
 * override, a wide slot) or none has run yet. */
int xh_trainer_pack_stats(xh_trainer *t, long *packed, long *unpacked, long *groups);

/* Tests only (synchronises the stream): the packed batch of the last learn()
 * as the compaction pass wrote it.  hdr: its 8 header ints (env-steps per
 * class NA, NB, UA, UB, packed groups GA, GB, all groups, 0); records, when
 * not NULL: the hdr[6] group records of 256 bytes each, in group order
 * (XH_ERR_INVALID when cap is smaller).  XH_ERR_STATE when the last learn()
 * did not run packed or none has run yet. */
int xh_trainer_pack_read(xh_trainer *t, int *hdr, void *records, size_t cap);

/* Tests and diagnostics only (synchronises the stream): whether the last
 * learn() ran its packed epochs ON THE TABLE -- a forward over the 578 (bin
 * state, item) points, one streaming pass over the packed batch that sums the
 * loss gradient per point, a backward over the 578 points -- (*ran = 1), the
 * rows of its packed batch whose state lay outside the table (clamped to the
 * nearest entry; 0 wherever the gate holds) and the groups of the table batch
 * (10, also where the table's launches run on their own 16-entry tiles and
 * read no table batch).  All three are 0 when it did not (XH_TRAIN_TABLE=0,
 * no packed learn(), KL-PPO, a slot of this trainer has held a bin below
 * -capacity) or none has run yet. */
int xh_trainer_table_stats(xh_trainer *t, int *ran, long *out_of_domain, long *groups);

#ifdef __cplusplus
}
#endif
#endif /* XYLO_HIP_H_ */
