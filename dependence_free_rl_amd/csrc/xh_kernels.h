// xh_kernels.h -- kernel argument blocks and launch entry points shared by the
// host runtime (the .cpp units) and the HIP kernel files.  No torch types.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xh {

enum Algo { kPPO = 0, kAC = 1, kKLPPO = 2 };
enum Heuristic { kHeurRandom = 0, kHeurFirstfit = 1, kHeurBestfit = 2,
                 kHeurMinwaste = 3 };

// Flat parameter offsets of the per-bin policy, in the reference layout
// model::parameters() (nn.h:499-508): conv1d_1(F0->H1), relu,
// conv1d_1(H1->H2), relu, conv1d_1(H2->1), head.  Each dense layer stores
// [A(out x in) row-major, b(out)].
struct PolicyLayout {
  int F0, H1, H2;
  __host__ __device__ int oW1() const { return 0; }
  __host__ __device__ int ob1() const { return H1 * F0; }
  __host__ __device__ int oW2() const { return ob1() + H1; }
  __host__ __device__ int ob2() const { return oW2() + H2 * H1; }
  __host__ __device__ int ow3() const { return ob2() + H2; }
  __host__ __device__ int ob3() const { return ow3() + H2; }
  __host__ __device__ int size() const { return ob3() + 1; }
};

// Value net: full(Fin->V1), relu, full(V1->V2), relu, full(V2->1)
// (ppo_training.cc:19-26).
struct ValueLayout {
  int Fin, V1, V2;
  __host__ __device__ int oW1() const { return 0; }
  __host__ __device__ int ob1() const { return V1 * Fin; }
  __host__ __device__ int oW2() const { return ob1() + V1; }
  __host__ __device__ int ob2() const { return oW2() + V2 * V1; }
  __host__ __device__ int ow3() const { return ob2() + V2; }
  __host__ __device__ int ob3() const { return ow3() + V2; }
  __host__ __device__ int size() const { return ob3() + 1; }
};

// Environment description (bin_packing.h:46-85, generalised to D dims).
struct EnvDesc {
  int B, D;
  int item_a[3], item_b[3];
  double p_a;
};

// Per-iteration trajectory storage (device).  Slot t of `bins`/`items` is the
// state S_t before step t; slot T is the state after the last step (the next
// iteration's S_0).  Terminal states E_t are recomputed from S_t + action.
struct Batch {
  int N, T;
  int8_t *bins;     // [T+1][N][B*D]
  int8_t *items;    // [T+1][N][4]
  int32_t *action;  // [T][N]
  float *pold;      // [T][N]   distrib[choice] at sampling time (rl.h:29)
  uint8_t *done;    // [T][N]
  uint32_t *rng;    // [N]      per-env minstd_rand0 state (reference order)
};

struct RolloutArgs {
  EnvDesc env;
  Batch b;
  int t;              // step index within the iteration
  uint32_t jump_mul;  // a^(4T(Nglobal-1)) mod m, applied after step T-1
  const float *params;
  const int32_t *forced;  // optional [T][N] actions (teacher forcing)
  float *logits_out;      // optional [N][B] (debug / parity)
  float *probs_out;       // optional [N][B]
  float *qold_out;        // KL-PPO: [T][N][B] the sampled distribution
  int wide;  // slot t holds a bin below -capacity (the f16-pair rollouts
             // bound |bins / capacity| by 1) or an item outside the item
             // table (they fold the item into per-entry biases): the f32
             // kernels run that slot
  int wide_seen;  // a slot 0 of this trainer has held a bin below -capacity.
                  // Such a bin stays until an action takes it (the reset that
                  // follows clears it), and only slot t is described by
                  // `wide`: later slots and windows may still hold it, so the
                  // logit table (xh_logit_table.h) is not used
  int src_slot;  // > 0 (with t == 0): slot 0 := slot src_slot first
                 // (replay_buffer::forget keeping the open trajectories), done
                 // by the register-stepping kernels as they fetch, else by
                 // copies before the launch; 0 / -1: slot 0 as it is
  int nsteps;  // slots t .. t + nsteps - 1 (0 = 1); logits_out / probs_out
               // receive the last one's.  launch_rollout_step runs them in
               // one launch where the kernel steps in registers
               // (rollout_split_kernel), else one launch per slot
  // Optional, both or neither: the forward outputs PPO's first policy epoch
  // reuses (policy_train_spec8_e0_kernel).  e0_p [T][N][64]: every step's
  // distribution, the values qold_out receives (launch_rollout_step passes it
  // as qold_out when that is null).  e0_mask [T][N] records of 1 KB: the bits
  // [layer-2 pre-activation > 0] (spec8_e0_layout.h), written only by the
  // 64-bin one-env-per-wave rollout_split_kernel; any other kernel leaves
  // them alone.
  float *e0_p;
  uint32_t *e0_mask;
};

// policy_train_spec8_e0_kernel's arguments: PPO's epoch 0 on the rollout's
// own layer-2 relu masks and distributions (the policy parameters are the
// ones the rollout ran with)
struct PolicyTrainE0Args {
  const float *e0_p;        // [T][N][64]
  const uint32_t *e0_mask;  // [T][N] records (spec8_e0_layout.h)
};

struct PolicyTrainArgs {
  EnvDesc env;
  Batch b;
  int algo;
  float clip_eps;
  const float *params;
  const float *adv;  // [T][N]
  // device scalar G >= |g| of every row of the launch, g the loss gradient on
  // the logits (launch_g_bound, once per learn(): the advantages and p_old
  // are the same in every epoch); policy_train_spec8_kernel scales dW2's f16
  // operand by it.  PPO / actor-critic only.
  const float *g_bound;
  float *slab;       // [gridDim.x][slab_stride]
  int slab_stride;
  int wide;          // a slot of the batch holds a bin below -capacity: the
                     // f32-MFMA kernels run (RolloutArgs::wide)
  int ablate;        // diagnostic build only (XH_ABLATE, make diag): bit0 skip
                     // dW2, bit1 skip dH1/dW1, bit2 skip layer-2 fwd, bit3
                     // skip softmax/loss; folded away in the product build
  // KL-PPO (kl_regulated_loss): every row of the learner's state matrix,
  // i.e. the T*N transitions, the open trajectories' end rows (slot T) and
  // the terminal end rows E_t listed in end_list.
  const float *qold;     // [T][N][B] old distributions
  const float *beta;     // device scalar (adapted between epochs)
  const int *end_list;   // [n_end] t*N + env of terminal transitions
  const int *n_end;      // device scalar
  double *kl_part;       // [gridDim.x] sum over rows of KL(q || p)
  // diagnostic build only (XH_PHASE_TRACE): per-wave cycle stamps at the
  // 8-wave train kernel's phase boundaries, [4 blocks][32 groups][8 waves][8]
  long long *trace;
  // the packed batch of the 64-bin 2-D [128,128] epoch (spec8_pack_layout.h;
  // launch_spec8_pack, once per learn()): both set = the PPO / actor-critic
  // epoch runs policy_train_spec8_kernel's packed build over it
  const uint8_t *pk;   // the groups' records
  const int *pk_hdr;   // device header: env-steps and groups per class
};
constexpr int kTraceBlocks = 4, kTraceGroups = 32, kTraceSlots = 8;

// End-row bookkeeping: the ended transitions (KL-PPO end rows, the value
// step's terminal views).
struct EndListArgs {
  const uint8_t *done;   // [T][N]
  int N, T;
  int *end_list;         // [T*N] env-major, t ascending
  int *n_end;            // scalar
  int *n_open;           // scalar: envs whose last step is not terminal
  int *rows_out;         // optional: *rows_out = rows_base + n_end
  int rows_base;
};
// end_list / n_end / n_open (scratch: end_list_scratch_ints(N) ints).
int end_list_scratch_ints(int N);
// dst[list[j]] = src[j] for j < *n (terminal-view values to transition rows)
hipError_t launch_scatter_list(const int *list, const int *n, const float *src,
                               float *dst, int max_n, hipStream_t s);

// TD targets and GAE around the value net (the net itself runs on the Dense
// GEMMs, MlpArgs).
struct ValueArgs {
  EnvDesc env;
  Batch b;
  float *v_state;        // [T+1][N]   V(S_t)
  float *v_term;         // [T][N]     V(E_t) (terminal view of step t)
  float *row_g;          // [T*N] dL/dV = V - target (targets kernel), or null
};

// Deterministic (argmax) evaluation, policy_gradient_deterministic_policy
// (policy_gradient.h:356-373) as used by deep_agent.cc and the drivers'
// every-100-iterations evaluation: `episodes` whole episodes per env, env e
// on its own minstd stream starting at jump(x0, e * stream_stride).
struct EvalArgs {
  EnvDesc env;
  const float *params;
  int n_envs;
  int episodes;
  int argmax_probs;  // 1: argmax over softmax output, 0: over raw logits
  uint32_t x0;
  uint64_t stream_stride;
  long max_steps;     // safety bound per env
  const int *init_items;  // [n_envs][D] device, or nullptr: construct
  double *total;      // [n_envs] summed rewards
  long *steps;        // [n_envs] env steps taken
  int *final_items;   // [n_envs][D]
  uint32_t *rng_out;  // [n_envs]
  int *trace;         // env 0's actions [trace_cap] or nullptr
  long trace_cap;
};

// Heuristic agents (heuristic_kernels.hip): same stream / output convention
// as EvalArgs.
struct HeuristicArgs {
  EnvDesc env;
  int n_envs;
  int episodes;
  uint32_t x0;
  uint64_t stream_stride;
  long max_steps;
  const int *init_items;
  double *total;
  long *steps;
  int *final_items;
  uint32_t *rng_out;
  int *trace;
  long trace_cap;
};
// Full MLP (full_layer / relu chain, nn.h:60-110, 350-377) over a batch of
// rows whose input is the observation of (slot, env) states
// (dense_kernels.hip).  Layer l maps w[l] -> w[l+1]; relu after every layer
// but the last.  act[l] / grad[l]: [max_rows][w[l+1]] outputs and
// dL/d(pre-activation) of layer l.
struct MlpArgs {
  EnvDesc env;
  const int8_t *bins, *items;  // Batch state layout
  const int *list;             // row -> slot * N + env (nullptr: env = row)
  int N, slot;                 // slot used when list == nullptr
  const int32_t *action;       // non-null: rows >= term_from are the terminal
  int term_from;               //   views E_t of transition row - term_from
  const int *term_list;        //   (or of transition term_list[row - term_from])
  const int *rows;             // device row count (nullptr: max_rows)
  int max_rows;
  // optional [w[1]][B*D + D] scratch: layer 0 on the reduced observation
  // (bins, then the item once -- its B copies' weights pre-summed)
  float *w0red;
  int nlayers;
  int w[4];
  const float *params;  // flat model::parameters() layout
  float *act[3];
  float *grad[3];
  // optional with term_list: the output of row term_from + j also goes to
  // v_term[term_list[j]] for j < *term_n (the terminal views' values onto
  // their transition rows)
  float *v_term;
  const int *term_n;
  // the bf16 value-net kernels (value_net_kernels.hip): scratch for W0's
  // three-part fragments (vnet_frag_bytes), and the rows whose activations
  // the forward stores for the backward (0: all, -1: none)
  void *w0frag;
  int act_rows;
  // 1: w0frag already holds the fragments of these parameters (the trainer
  // knows they did not change since the last forward prepared them): the
  // forward skips its preparation launch
  int w0frag_ready;
};
hipError_t mlp_forward(const MlpArgs &a, hipStream_t s);
// Weight gradients of every layer into slab[split] (flat layout), data
// gradients down to layer 1 (layer 0 gets no backward, nn.h:516-526).
hipError_t mlp_backward(const MlpArgs &a, float *slab, int stride, int splits,
                        hipStream_t s);
// update_value_model's backward (policy_gradient.h:196-218) over the
// a.max_rows transition rows: TD targets and dL/dV = V - target
// (value_targets_kernel, into targets and a.grad[last]), then mlp_backward.
// The Fin -> 64 -> 32 -> 1 value net runs fused (two launches, the same
// bits) unless XH_VALUE_KERNEL=gemm.
hipError_t value_backward(const MlpArgs &a, const ValueArgs &va, float gamma,
                          float *targets, float *slab, int stride, int splits,
                          hipStream_t s);
// The kernels mlp_forward / value_backward run for a value net:
//   "vnet_bf16"  value_net_kernels.hip (Fin -> 64 -> 32 -> 1, B*D % 16 == 0,
//                B*D + D < 416, w0frag set): the default
//   "mlp3_fused" the f32 fused kernels (the same shape; XH_VALUE_KERNEL=mlp3)
//   "gemm"       layer by layer (any shape; XH_VALUE_KERNEL=gemm)
const char *value_kernel_name(const MlpArgs &a);
// true: the value kernels write layer 0's gradient on the reduced
// observation (bin 0's item columns only: slab_reduce needs SlabAlias)
bool value_reduced_slab(const MlpArgs &a);
bool vnet_shape_ok(const MlpArgs &a);
size_t vnet_frag_bytes(const EnvDesc &e);
hipError_t vnet_forward(const MlpArgs &a, hipStream_t s);
hipError_t vnet_backward(const MlpArgs &a, const ValueArgs &va, float gamma,
                         float *targets, float *slab, int stride, int splits,
                         hipStream_t s);

// model::eval of a described layer chain (dense_kernels.hip, xh_model_eval).
enum LayerKind { kLayerFull = 0, kLayerConv1d = 1, kLayerRelu = 2,
                 kLayerSoftmax = 3, kLayerSoftmaxXent = 4 };
struct ModelLayer {
  int kind, in, out;
};
hipError_t model_forward(const ModelLayer *layers, int nl, const float *params,
                         const float *x, int rows, int cols, float *a, float *b,
                         const float **out, int *out_cols, hipStream_t s);
// One layer of the reference's layer interface (nn.h:20-33) on device
// buffers: forward (y: rows x output width), backward (out: rows x cols, the
// data gradient), gradient (grad: the layer's flat parameter gradient, via
// layer_gradient_splits(...) slabs of `stride` floats; activations: none).
hipError_t layer_forward(const ModelLayer &L, const float *W, const float *x,
                         int rows, int cols, float *y, hipStream_t s);
hipError_t layer_backward(const ModelLayer &L, const float *W, const float *x,
                          int rows, int cols, const float *bp, float *out,
                          hipStream_t s);
int layer_gradient_splits(const ModelLayer &L, int rows, int cols);
hipError_t layer_gradient(const ModelLayer &L, const float *x, int rows,
                          int cols, const float *bp, float *slab, int stride,
                          float *grad, hipStream_t s);
// The discrete-action loss gradients of a batch (rl.h:33-74 row by row;
// policy_gradient.h:24-85): out [rows][range].
enum LossKind { kLossGradientLog = 0, kLossSoftmaxGradientLog = 1,
                kLossClipped = 2, kLossKlRegulated = 3 };
hipError_t launch_action_loss(int kind, int rows, int range,
                              const int32_t *choice, const float *distrib,
                              const float *adv, const float *probs, float param,
                              float *out, hipStream_t s);

// REINFORCE (pg_kernels.hip).  Batch.T = the per-iteration step bound.
struct PgStepArgs {
  EnvDesc env;
  Batch b;
  int t, episodes;
  const float *logits;    // [N][B] of slot t
  const int32_t *forced;  // [T][N] or nullptr
  int *ep_done, *len, *active;
};
struct PgLearnArgs {
  int N, B, episodes;
  float gamma;
  const int *len;
  int *row_off, *list, *nrows;
  const uint8_t *done;
  const int32_t *action;
  float *rtg;       // [rows]
  double *ep_part;  // [N]
  double *stats;    // [2]: sum of slot-0 returns, trajectories
  const float *logits;
  float *dlogits;
  float *adv_grid;  // [T][N] advantages for introspection
};
hipError_t launch_pg_env_init(const EnvDesc &env, Batch b, uint32_t x0,
                              int env_offset, uint64_t stride, hipStream_t s);
hipError_t launch_pg_seed(Batch b, uint32_t x, int env_offset, uint64_t stride,
                          hipStream_t s);
hipError_t launch_pg_begin(int N, int *active, int *ep_done, int *len,
                           hipStream_t s);
hipError_t launch_pg_step(const PgStepArgs &a, hipStream_t s);
hipError_t launch_pg_rows(const PgLearnArgs &a, hipStream_t s);
hipError_t launch_pg_adv(const PgLearnArgs &a, hipStream_t s);
hipError_t launch_pg_loss(const PgLearnArgs &a, int max_rows, hipStream_t s);

// Vectorised environment for callers with their own policy (xh_venv_*,
// venv_kernels.hip): bins int8 [N][B*D], items int8 [N][4], rng u32 [N].
enum VenvOp { kVenvStep = 0, kVenvReset = 1, kVenvObserve = 2 };
// Episode statistics (xh_venv_set_episode_stats, venv_episode_kernels.hip):
// an env's window accumulators, 32 bytes, touched only by the step that ends
// an episode of the env (its bin-0 lane) and by the row kernel, which clears
// them (count 0, sums 0, len_min INT32_MAX, len_max 0).
struct VenvEpAcc {
  int32_t count;             // episodes ended since the last row
  int32_t len_min, len_max;  // of their lengths
  int32_t pad;
  int64_t len_sum;
  uint64_t len_sqsum;
};
static_assert(sizeof(VenvEpAcc) == 32, "one env's accumulators are 32 bytes");
struct VenvArgs {
  EnvDesc env;
  int N;
  int8_t *bins, *items;
  uint32_t *rng;
  const int32_t *action;  // [N] chosen bins
  const uint8_t *mask;    // [N] or nullptr (all envs)
  float *reward;          // [N] (step)
  uint8_t *done;          // [N] game_over after the apply
  float *obs;             // [N][B][2D] or nullptr
  int *err;               // device flag: an action was out of range
  int mode;               // 0 environment::apply, 1 agent::step minus react
  uint32_t skip_mul;      // a^policy_draws (step)
  uint32_t jump_mul;      // a^(k (Nglobal - 1)) after a step (reference order)
  // episode statistics: all three null while off.  ep_running is read and
  // written by every live env step; the other two only where a step ends an
  // episode
  int32_t *ep_running;    // [N] steps of the episode in flight
  int32_t *ep_first;      // [N] the env's first finished length, -1 until then
  VenvEpAcc *ep_acc;      // [N] the window accumulators
};
// xh_venv_act: react's sampling + agent::step in one launch (venv_act_kernel).
struct VenvActArgs {
  VenvArgs v;             // mode 1; v.action unused (the kernel writes action)
  const float *policy;    // [N][B] probabilities or logits
  int32_t *action;        // [N] the chosen bin (out)
  float *pchoice;         // [N] probability of the chosen bin (out)
  int logits;             // the rows are logits: f32 softmax with a max shift
  int argmax;             // first maximum instead of a sample (no draws)
  // the trajectory record's slot (null: record off); slot = the cursor
  int32_t *rec_action;    // [T][N]
  float *rec_pchoice;     // [T][N]
  float *rec_reward;      // [T][N]
  uint8_t *rec_done;      // [T][N]
  int8_t *rec_bins;       // [T][N][B][D] the state before the step, or null
  int8_t *rec_items;      // [T][N][4]
  int slot;
  // invalid-action masking (xh_venv_set_action_mask): legal != 0 picks the
  // MASK instantiation, which replaces the row's entries outside the env's
  // legal set before anything reads them
  int legal;
  float *rec_distrib;     // [T][N][B] the p[] sampled from, or null
                          // (xh_venv_set_record_distrib)
  uint32_t *rec_legal;    // [T][N][W] the words it masked with (legal), or null
};
// the packed legal set: W = max(1, B / 32) uint32 words per env, bit b % 32
// of word b / 32 is bin b
inline int venv_legal_words(int B) { return B >= 32 ? B / 32 : 1; }
// A general item set (xh_item_set, xh_venv_create_ex / xh_venv_set_item_set):
// the general kernels' second argument, so it travels in the kernel arguments
// (uniform loads, no device table to keep in step with the stream) and the
// builtin kernels' arguments are what they were.  thr[k] = c_k, the K-way
// draw's thresholds, 1.0 from the last item of positive weight on (and past
// K); shape[k] = item k's int8 x 4 as
// the ITEMS word, 0 past K; cap[d] the capacity of dim d, 1 past D.
constexpr int kVenvItemsMax = 16;
struct VenvItemTable {
  double thr[kVenvItemsMax];
  uint32_t shape[kVenvItemsMax];
  int32_t cap[4];
};
bool venv_shape_supported(int B, int D);
// items == nullptr: the builtin instantiations (make_env's two items, capacity
// kCapacity); otherwise the general ones (venv_gen_kernels.o)
hipError_t launch_venv(const VenvArgs &a, int op, hipStream_t s,
                       const VenvItemTable *items = nullptr);
hipError_t launch_venv_act(const VenvActArgs &a, hipStream_t s,
                           const VenvItemTable *items = nullptr);
hipError_t launch_venv_gen(const VenvArgs &a, int op, hipStream_t s,
                           const VenvItemTable &items);
hipError_t launch_venv_act_gen(const VenvActArgs &a, hipStream_t s,
                               const VenvItemTable &items);
// xh_venv_act_heuristic (venv_heur_kernel, venv_heur_kernels.hip): the act
// launch with the row formed in registers from the env's own state.  a.policy,
// a.logits, a.argmax and a.rec_distrib are not read; heur is a Heuristic, the
// same for every lane.  items as in launch_venv_act.
struct VenvHeurArgs {
  VenvActArgs a;
  int heur;
};
hipError_t launch_venv_heur(const VenvHeurArgs &h, hipStream_t s,
                            const VenvItemTable *items = nullptr);
hipError_t launch_venv_heur_gen(const VenvHeurArgs &h, hipStream_t s,
                                const VenvItemTable &items);
// Logit tables (xh_venv_table_*, venv_table_kernels.hip; the domain:
// xh_venv_table.h).  Every launch takes the item table by reference: a venv
// without a set passes the default set's.
struct VenvTabDomain {
  int D, K;       // dims, the set's items
  int side[4];    // capacity[d] + 1, 1 past D
  int states;     // S = prod side[d]
  long entries;   // E = K S, 1 .. XH_VTAB_MAX_ENTRIES
};
// observations of the table's `total` = R B per-bin rows, [R][B][2D]
hipError_t launch_venv_table_obs(const VenvTabDomain &m,
                                 const VenvItemTable &t, long total,
                                 float *obs, hipStream_t s);
// xh_venv_act_table (venv_act_table_kernel): the act launch with the row
// gathered from `table` ([>= E] floats) inside it.  a.policy and a.logits are
// not read (the rows are logits); a.argmax and a.rec_distrib as in the act.
struct VenvTabActArgs {
  VenvActArgs a;
  VenvTabDomain m;
  const float *table;
};
hipError_t launch_venv_act_table(const VenvTabActArgs &h, hipStream_t s,
                                 const VenvItemTable &t);
// `count` rows of the record's STATE view (VenvObsArgs' addressing): the
// gather reads table and writes out; the gradient sum reads dout and adds
// into acc through maxbits.
struct VenvTabRowArgs {
  int B, D, N;
  int P;                      // the record's cursor
  VenvTabDomain m;
  const int8_t *rec_bins;     // [P][N][B][D]
  const int8_t *rec_items;    // [P][N][4]
  const int8_t *cur_bins;     // [N][B][D]
  const int8_t *cur_items;    // [N][4]
  const int32_t *rows;        // index list or nullptr (rows first ..)
  long first, count;
  const float *table;         // [>= E] (gather)
  float *out;                 // [count][B], 16-byte aligned (gather)
  const float *dout;          // [count][B], 16-byte aligned (grad)
  uint32_t *maxbits;          // one word, zeroed before the launch (grad)
  unsigned long long *acc;    // [E] int64 sums, zeroed before the launch (grad)
  int *err;                   // bit 4: an index outside the view's rows; bit
                              // 8: a state outside the domain, a NaN / inf dout
};
hipError_t launch_venv_table_gather(const VenvTabRowArgs &a, hipStream_t s,
                                    const VenvItemTable &t);
// G into g [total = R B floats] (added where accumulate): three launches
hipError_t launch_venv_table_grad(const VenvTabRowArgs &a, long total,
                                  int accumulate, float *g, hipStream_t s,
                                  const VenvItemTable &t);
// xh_venv_legal: out [N][W], the legal set (all bins where it is empty) of
// every env's current state; reads a.bins / a.items only
hipError_t launch_venv_legal(const VenvArgs &a, uint32_t *out, hipStream_t s);
hipError_t launch_venv_init(const VenvArgs &a, uint32_t x0, int env_offset,
                            int n_global, int k, hipStream_t s,
                            const VenvItemTable *items = nullptr);
hipError_t launch_venv_init_gen(const VenvArgs &a, uint32_t x0, int env_offset,
                                int n_global, int k, hipStream_t s,
                                const VenvItemTable &items);

// Episode statistics of a venv (venv_episode_kernels.hip).
// running 0, first -1, the accumulators cleared
hipError_t launch_venv_ep_init(int N, int32_t *running, int32_t *first,
                               VenvEpAcc *acc, hipStream_t s);
// One row of XH_VEP_COUNT doubles from the per-env blocks, which it clears:
// workgroup partials psum [venv_ep_grid(N)][kVepSums] and pext
// [venv_ep_grid(N)][kVepExts] (min length, max length, max running), then
// one wave's fixed-order sum into row.
constexpr int kVepSums = 7;
constexpr int kVepExts = 3;
int venv_ep_grid(int N);
hipError_t launch_venv_ep_row(int N, const int32_t *running,
                              const int32_t *first, VenvEpAcc *acc,
                              double *psum, double *pext, double row_index,
                              double calls, double *row, hipStream_t s);

// The learner's side of a recorded window (xh_venv_record_obs /
// xh_venv_advantages, venv_learn_kernels.hip).
// observation::to_vector of `count` rows of the record: row q = t N + e is
// slot t of env e (slot P = the present state); next != 0 gives the successor
// row of transition q (S_t+1, or the terminal view E_t where done[q]).
struct VenvObsArgs {
  int B, D, N;
  int P;                      // the record's cursor
  int next;                   // XH_VOBS_NEXT
  const int8_t *rec_bins;     // [P][N][B][D]
  const int8_t *rec_items;    // [P][N][4]
  const int8_t *cur_bins;     // [N][B][D] the state after slot P - 1's step
  const int8_t *cur_items;    // [N][4]
  const int32_t *rec_action;  // [P][N] (next)
  const uint8_t *rec_done;    // [P][N] (next)
  const int32_t *rows;        // index list or nullptr (rows first ..)
  long first, count;
  float *obs;                 // [count][B][2D], 16-byte aligned
  int *err;                   // bit 4: an index outside the view's rows
};
// cap == nullptr: capacity kCapacity; otherwise the D capacities of a general
// item set (the general instantiation: IEEE f32 divisions by them)
hipError_t launch_venv_record_obs(const VenvObsArgs &a, hipStream_t s,
                                  const int32_t *cap = nullptr);
// GAE, TD(0) targets and lambda returns of a window with explicit rewards:
// gae_kernel's and value_targets_kernel's arithmetic, one env per lane.
struct VenvGaeArgs {
  int N, T;
  const float *values;    // [T+1][N]
  const float *v_term;    // [T][N] or nullptr (0)
  const float *reward;    // [T][N]
  const uint8_t *done;    // [T][N]
  float gamma, lambda;
  float *adv;             // [T][N]
  float *td_target;       // [T][N] or nullptr
  float *lambda_return;   // [T][N] or nullptr
  double *part;           // [venv_gae_grid(N)][2] sum A, sum A^2, or nullptr
  int *end_part;          // [venv_gae_grid(N)] ended rows (with part)
};
int venv_gae_grid(int N);
hipError_t launch_venv_gae(const VenvGaeArgs &a, hipStream_t s);
// stats[2] = rows, stats[3] = the sum of end_part (one wave, fixed order)
hipError_t launch_venv_adv_counts(const int *end_part, int nparts, double rows,
                                  double *stats, hipStream_t s);
// xh_venv_policy_loss (venv_loss_kernels.hip): the loss head of the caller's
// network on `count` rows of a recorded window, row j's index q = rows[first
// + j] or first + j.
constexpr int kVenvLossMaxBlocks = 4096;
struct VenvLossArgs {
  int B;
  int logits;                 // XH_ACT_LOGITS: venv_act_kernel's softmax first
  int loss;                   // kLossSoftmaxGradientLog / kLossClipped /
                              // kLossKlRegulated (with distrib)
  const float *policy;        // [count][B], 16-byte aligned; may equal grad
  const int32_t *rows;        // index list or nullptr
  long first, count, total;   // q in [0, total)
  long tiles;                 // set by the launcher
  const float *adv;           // [total]
  const int32_t *action;      // [total]
  const float *p_old;         // [total]
  float eps, scale;
  const float *values_new;    // [count] or nullptr (no value head)
  const float *target;        // [total] (with values_new)
  float value_scale;
  float *grad;                // [count][B], 16-byte aligned
  float *dvalue;              // [count] (with values_new)
  float *probs_out;           // [count][B], 16-byte aligned, or nullptr
  double *part;               // [venv_loss_grid][XH_VLOSS_COUNT] or nullptr
  int *err;                   // bit 4: an index or an action out of range
  const float *distrib;       // [total][B] sampling distributions, 16-byte
                              // aligned, or nullptr (no KL code)
  float beta;                 // kLossKlRegulated: the regulation's weight ...
  const float *beta_dev;      // ... or, where not null, one device float
  double *kl_part;            // [venv_loss_grid][XH_VKL_COUNT] or nullptr
  const uint32_t *legal;      // [total][W] the rows' legal words (a row of
                              // zeros: unmasked), or nullptr (no mask code)
  // xh_venv_policy_loss_ex's extension; ext != 0 picks the instantiation
  // that holds it, the other one reads none of these
  int ext;
  float ent_coef;             // the entropy bonus's weight (0: none) ...
  const float *ent_coef_dev;  // ... or, where not null, one device float
  const float *v_old;         // [total] the values at collection time, or
                              // nullptr (no value clipping)
  float vclip;                // with v_old
  double *ext_part;           // [venv_loss_grid][XH_VEXT_COUNT] or nullptr
};
int venv_loss_grid(int B, long count);
hipError_t launch_venv_policy_loss(VenvLossArgs a, hipStream_t s);
// stats[k] = (accumulate ? stats[k] : 0) + the sum of part[nparts][k]
hipError_t launch_venv_loss_reduce(const double *part, int nparts,
                                   int accumulate, double *stats,
                                   hipStream_t s);
// the same for kl_part[nparts][XH_VKL_COUNT] -> kl_stats
hipError_t launch_venv_kl_reduce(const double *part, int nparts, int accumulate,
                                 double *kl_stats, hipStream_t s);
// the same for ext_part[nparts][XH_VEXT_COUNT] -> ext_stats
hipError_t launch_venv_ext_reduce(const double *part, int nparts,
                                  int accumulate, double *ext_stats,
                                  hipStream_t s);

// The per-bin policy net of a venv learner (xh_net, net_kernels.hip): the
// conv1d_1 chain F0 -> H1 -> relu -> H2 -> relu -> 1 over the R = rows * B flat
// per-bin rows of an observation block, fused; tiles of 64 flat rows, `grid`
// persistent workgroups (1 <= grid <= net_policy_tiles(R)).
struct NetPolicyArgs {
  int F0, H1, H2;
  const float *params;  // PolicyLayout
  const float *obs;     // [R][F0]
  long R;
  float *logits;        // forward: [R] (out)
  const float *dout;    // backward: [R] dL/dlogit
  float *slab;          // backward: [grid][slab_stride] (out), PolicyLayout
  int slab_stride;
};
bool net_policy_shape_supported(int F0, int H1, int H2);
long net_policy_tiles(long R);
int net_policy_lds_bytes(int F0, int H1, int H2, int backward);
hipError_t launch_net_policy_fwd(const NetPolicyArgs &a, int grid, hipStream_t s);
hipError_t launch_net_policy_bwd(const NetPolicyArgs &a, int grid, hipStream_t s);

// The value net 2BD -> 64 -> relu -> 32 -> relu -> 1 read straight from a
// venv's recorded window (xh_net_forward_record / xh_net_backward_record,
// net_value_kernels.hip): `rec` addresses the rows as xh_venv_record_obs does
// (rec.obs is not used), the observation is formed in registers from the int8
// state with IEEE f32 divisions by float(cap[d]); tiles of 64 rows, `grid`
// persistent workgroups (1 <= grid <= net_value_tiles(rec.count)).
struct NetValueArgs {
  VenvObsArgs rec;
  int32_t cap[4];       // the venv's per-dim capacities
  const float *params;  // ValueLayout{2BD, 64, 32}
  float *out;           // forward: [count] (out); rows outside the view untouched
  const float *dout;    // backward: [count] dL/dvalue
  float *slab;          // backward: [grid][slab_stride] (out), ValueLayout
  int slab_stride;
};
constexpr int kNetValueV1 = 64, kNetValueV2 = 32;
long net_value_tiles(long count);
int net_value_lds_bytes(int backward);
hipError_t launch_net_value_fwd(const NetValueArgs &a, int grid, hipStream_t s);
hipError_t launch_net_value_bwd(const NetValueArgs &a, int grid, hipStream_t s);

// 1 when the kernels were built with the phase-ablation switches
// (make diag, -DXH_DIAG_ABLATE=1), 0 in the product library.
int diag_build();

bool heuristic_shape_supported(int B, int D);
hipError_t launch_heuristic(const HeuristicArgs &a, int kind, hipStream_t s);

// Launchers (return hipError_t of the launch). `variant` selects the
// <B,D,H1,H2> instantiation; returns hipErrorInvalidValue when unsupported.
bool policy_shape_supported(int B, int D, int H1, int H2);
hipError_t launch_env_init(const EnvDesc &env, Batch b, uint32_t x0,
                           int env_offset, int n_global, hipStream_t s);
hipError_t launch_env_seed(Batch b, uint32_t x, int env_offset,
                           hipStream_t s);
hipError_t launch_end_list(const EndListArgs &a, int *scratch, hipStream_t s);
// beta <- adapt(beta, mean KL) (policy_gradient.h:68-80); kl_sum[0] = the
// (all-reduced) KL sum, rows[0] the (all-reduced) row count.
hipError_t launch_kl_reduce(const double *kl_part, int nparts, const int *n_end,
                            const int *n_open, double rows_main,
                            double *kl_sum, hipStream_t s);
hipError_t launch_kl_beta_update(const double *kl_sum, float *beta,
                                 float d_targ, float *log, hipStream_t s);
// What a launch entry point ran, recorded by the trainer for
// xh_trainer_kernel_info: the kernel's name and its arithmetic.
enum Math {
  kMathF32Mfma = 0,       // f32-input MFMA (v_mfma_f32_32x32x2_f32) / f32 VALU
  kMathSplitTrain = 1,    // bf16 MFMA on 3-part splits: layer 2 six products per
                          // f32 product, dW2 / dH1 three (rank-1 backward)
  kMathSplitRollout = 2,  // layer 2 on f16 pairs: three f16 products per f32
                          // product (the other layers f32 MFMA)
  kMathSplitTrainF16 = 3, // layer 2 three f16 MFMAs per f32 product (scaled f16
                          // pairs), dH1 two, dW2 three bf16 (8 per 3 products)
  kMathSplitTrainF16Pair = 4  // as above with dW2 on per-feature scaled f16
                              // pairs too: two (7 per 3 products)
};
struct KernelInfo {
  const char *name = nullptr;
  int math = kMathF32Mfma;
  // launch_rollout_step: the logits came from the launch's logit table
  // (rollout_split_kernel's table build) instead of a forward per row
  bool logit_table = false;
  // launch_rollout_step: envs a wave of the register-stepping rollout steps
  // at once (0: another kernel).  1 at 64 bins, lane = bin; more on the packed
  // table kernel (rollout_pack_kernels.hip)
  int envs_per_wave = 0;
};
hipError_t launch_rollout_step(const RolloutArgs &a, int H1, int H2, int grid,
                               hipStream_t s, KernelInfo *info = nullptr);
// The 64-bin 2-D table rollout with 64 / lanes envs per wave
// (rollout_pack_kernels.hip): rollout_split_kernel's table
// launch in another lane layout, for the same RolloutArgs (no e0_mask, not
// wide / wide_seen) and with the same bits in everything it writes.  lanes per
// env: kRollPackLanes, the shipped layout, or kRollPackLanesAlt, built beside
// it for A/B runs (XH_ROLLOUT_PACK_LANES, read per rollout); cus = workgroups
// at most.
constexpr int kRollPackLanes = 8, kRollPackLanesAlt = 16;
int rollout_pack_lanes(int want);
hipError_t launch_rollout_pack(const RolloutArgs &a, int lanes, int cus, hipStream_t s);
hipError_t launch_policy_train(const PolicyTrainArgs &a, int H1, int H2,
                               int grid, hipStream_t s,
                               KernelInfo *info = nullptr);
// The f32-accurate split train kernels for the 64-bin 2-D and 128-bin 3-D
// [128,128] shapes and the 32-bin 1-D [64,64] one (dispatch in
// train_select.cpp); XH_TRAIN_KERNEL=f32 selects the f32-MFMA ones.  The
// launchers of the superseded forms (split128 / 8w / 8wp / 4p / 8wg) are
// linked only into the variant library (`make variants`).
constexpr int kSplit128Bins = 128, kSplit128Dims = 3;
constexpr int kSplit4hBins = 32;
bool train_split_enabled();
bool policy_train_split_supported(const PolicyTrainArgs &a, int H1, int H2);
hipError_t launch_policy_train_split(const PolicyTrainArgs &a, int grid,
                                     hipStream_t s, KernelInfo *info);
hipError_t launch_policy_train_split128(const PolicyTrainArgs &a, int grid,
                                        hipStream_t s);
hipError_t launch_policy_train_split8w(const PolicyTrainArgs &a, int grid,
                                       hipStream_t s);
hipError_t launch_policy_train_split8wp(const PolicyTrainArgs &a, int grid,
                                        hipStream_t s);
hipError_t launch_policy_train_split4p(const PolicyTrainArgs &a, int grid,
                                       hipStream_t s);
hipError_t launch_policy_train_split8wh(const PolicyTrainArgs &a, int grid,
                                        hipStream_t s);
// its KL-PPO build (policy_split8wh_kl_kernels.o; called by
// launch_policy_train_split8wh)
hipError_t launch_policy_train_split8wh_kl(const PolicyTrainArgs &a, int grid,
                                           hipStream_t s);
// the wave-specialised config-3 / config-4 epoch (policy_spec8_kernels.hip)
hipError_t launch_policy_train_spec8(const PolicyTrainArgs &a, int grid, hipStream_t s);
// its KL-PPO build (policy_spec8_kl_kernels.o)
hipError_t launch_policy_train_spec8_kl(const PolicyTrainArgs &a, int grid, hipStream_t s);
// PPO's epoch 0 on the rollout's masks and distributions
// (policy_spec8_e0_kernels.o); the trainer decides when they are valid
hipError_t launch_policy_train_spec8_e0(const PolicyTrainArgs &a, const PolicyTrainE0Args &ea,
                                        int grid, hipStream_t s);
// its packed build over the batch's distinct rows
// (policy_spec8_pack_kernels.o; a.pk / a.pk_hdr from launch_spec8_pack)
hipError_t launch_policy_train_spec8_pack(const PolicyTrainArgs &a, int grid, hipStream_t s);
// the compaction pass (spec8_pack_kernels.hip, layout spec8_pack_layout.h):
// classify, scan, write; integer work, no host synchronisation
struct PackArgs {
  EnvDesc env;
  Batch b;
  const float *adv;  // [T][N] the final advantages
  uint8_t *pk;       // [pk_max_groups(T N)] group records
  int *hdr;          // [kPkHdrInts]
  uint8_t *cls;      // [T N] scratch: the env-steps' classes
  int *blk;          // [pk_scratch_ints(T N)] scratch: per chunk of 64 env-steps
                     // the classes' counts, then their offsets
};
// loop: classify and write find an env-step's duplicate states with the former
// wave-uniform loop (XH_SP8_PACK_DEDUP=loop) instead of the LDS lane masks;
// the same bytes either way
hipError_t launch_spec8_pack(const PackArgs &a, bool loop, hipStream_t s);
// The epoch on the table (spec8_table_layout.h): the per-bin
// net's activations depend on the table entry (bin state, item) alone and
// every parameter gradient is linear in the rows' loss gradient g, so an epoch
// is a forward over the table, one streaming pass over the packed batch that
// sums g per entry, and a backward over the table weighted by the sums.  The
// table's two launches are table_mm_kernels.hip's (TableFwdArgs / TableBwdArgs
// below); XH_TRAIN_TABLE=spec8 keeps the former ones:
// the spec8 kernel's table build (policy_spec8_tab_kernels.o), a.pk = the table
// batch, grid <= tb::kGroups; backward: a.g_bound = the bound on |G|
struct PolicyTrainTabArgs {
  float *logits;   // [lt::kEntries] forward: the entries' logits (out)
  const float *G;  // [lt::kEntries] backward: the sums of g per entry
  int forward;
};
hipError_t launch_policy_train_spec8_tab(const PolicyTrainArgs &a, const PolicyTrainTabArgs &ta,
                                         int grid, hipStream_t s);
// the streaming pass and its reduce (spec8_table_kernels.hip): per env-step
// of the packed batch the count-weighted softmax over the table's logits and
// the PPO / actor-critic loss gradient per distinct state, summed per entry;
// no float atomic, every sum in a fixed order
struct TableStreamArgs {
  const uint8_t *pk;    // the packed batch (launch_spec8_pack)
  const int *pk_hdr;
  const float *logits;  // [lt::kEntries]
  int algo;             // kPPO / kAC
  float clip_eps;
  double *part;         // [grid][lt::kEntries] scratch: the workgroups' sums
  float *G;             // [lt::kEntries] out (the reduce's)
  float *gmax;          // out: max_s |G_s| (the reduce's; the stream zeroes it)
  int *ood;             // += rows whose state lies outside the table (null: not counted)
};
// reduce = false: the stream alone, `part` left for table_bwd_kernel, which
// forms G itself; G is not written and *gmax is unused
hipError_t launch_table_stream(const TableStreamArgs &a, int grid, hipStream_t s,
                               bool reduce = true);
// The table's forward and backward on the exact f32 MFMA (table_mm_kernels.hip;
// tiles: table_tile_layout.h), tt::kTiles workgroups each, whatever the stream's
// grid: forward -> the entries' logits and H2; backward: G from the stream's
// `part` (table_reduce_kernel's order), the backward products, one slab per
// tile in the slab layout.  No scale, no bound on |G|.
struct TableFwdArgs {
  EnvDesc env;
  const float *params;
  float *logits;   // [lt::kEntries] out
  float *h2;       // [tt::kRows][128] out: relu(layer 2), f32
  int *zero_ood;   // non-null: workgroup 0 zeroes it (the stream's counter)
};
struct TableBwdArgs {
  EnvDesc env;
  const float *params;
  const float *h2;     // the forward's
  const double *part;  // [nparts][lt::kEntries] the stream's
  int nparts;          // the stream's grid, >= 1
  float *G;            // [lt::kEntries] out
  float *slab;         // [tt::kTiles][slab_stride] out
  int slab_stride;
};
hipError_t launch_table_fwd(const TableFwdArgs &a, hipStream_t s);
hipError_t launch_table_bwd(const TableBwdArgs &a, hipStream_t s);
// its earlier form, dW2 on the three-part bf16 split (the variant library
// only: XH_TRAIN_KERNEL=spec8_3p)
hipError_t launch_policy_train_spec8_3p(const PolicyTrainArgs &a, int grid, hipStream_t s);
// the wave-specialised config-2 epoch (policy_spec4_kernels.hip, opt-in by
// XH_TRAIN_KERNEL=spec4; one 8-wave workgroup per CU: train_spec4_default
// says when the grid is one per CU)
hipError_t launch_policy_train_spec4(const PolicyTrainArgs &a, int grid, hipStream_t s);
bool train_spec4_default(int B, int D, int H1, int H2, int kl);
hipError_t launch_policy_train_split8wg(const PolicyTrainArgs &a, int grid,
                                       hipStream_t s);
hipError_t launch_policy_train_split4h(const PolicyTrainArgs &a, int grid,
                                       hipStream_t s);
// its KL-PPO build (policy_split4h_kl_kernels.o; called by
// launch_policy_train_split4h)
hipError_t launch_policy_train_split4h_kl(const PolicyTrainArgs &a, int grid,
                                          hipStream_t s);
hipError_t launch_policy_train_split8x(const PolicyTrainArgs &a, int grid,
                                       hipStream_t s);
// its KL-PPO build (policy_split8x_kl_kernels.o; called by
// launch_policy_train_split8x)
hipError_t launch_policy_train_split8x_kl(const PolicyTrainArgs &a, int grid,
                                          hipStream_t s);
int policy_train_grid(int B, int D, int H1, int H2, int kl);
hipError_t launch_eval_argmax(const EvalArgs &a, int H1, int H2,
                              hipStream_t s);
int rollout_grid(int B, int D, int H1, int H2);

bool value_shape_supported(int V1, int V2);
hipError_t launch_value_targets(const ValueArgs &a, float gamma, float *targets,
                                hipStream_t s);
// GAE; part != nullptr also writes per-block (sum, sum of squares) of the
// advantages for the opt-in normalisation ([gae_grid(N)][2] doubles).
int gae_grid(int N);
hipError_t launch_gae(const ValueArgs &a, float gamma, float lambda, float *adv,
                      double *part, hipStream_t s);
hipError_t launch_adv_stats(const double *part, int nparts, double *stats,
                            hipStream_t s);
hipError_t launch_adv_normalize(float *adv, long n, const double *stats,
                                double count, hipStream_t s);
// *out = G, a bound on |g| (the loss gradient on the logits) over the n
// transitions: PPO max_t |A_t| max(1 + clip_eps, 1 / p_old_t) (|ig| <= max(
// ratio, 1 + eps) |A|, ratio <= 1 / p_old, |g_r| <= |ig|), actor-critic
// max_t |A_t|.  A NaN among the terms gives a NaN.  No host synchronisation.
hipError_t launch_g_bound(const float *adv, const float *pold, long n, int ppo,
                          float clip_eps, float *out, hipStream_t s);

// On-device training statistics (stats_kernels.hip; xh_trainer_set_stats):
// double sums, one partial per workgroup ([gae_grid(N)][S] doubles), summed in
// a fixed order by one wave into the iteration's row of XH_STAT_COUNT doubles.
constexpr int kStatEpisodeSums = 4;  // episodes, len, len^2, -log p_old
constexpr int kStatEpisodeSummed = 5;  // row entries EPISODES .. NEGLOGP_SUM
constexpr int kStatLearnerSums = 6;  // row entries VERR_SUM .. ADV_SQSUM
// episode part: ep_len[N] carries every env's running episode length
hipError_t launch_episode_stats(const uint8_t *done, const float *pold, int N,
                                int T, int *ep_len, double *part,
                                hipStream_t s);
// opens `row`: episode part from the partials, NaN in the learner part
hipError_t launch_episode_row(const double *part, int nparts, double iter,
                              double transitions_global,
                              double transitions_local, double *row,
                              hipStream_t s);
// learner part: sums of target - V0, target and the advantage, and squares
hipError_t launch_learner_stats(const float *v0, const float *targets,
                                const float *adv, int N, int T, double *part,
                                hipStream_t s);
// squared L2 norms of the first / last policy gradient and the value gradient
hipError_t launch_grad_norms(const float *g_first, const float *g_last, int np,
                             const float *gv, int nv, double *out,
                             hipStream_t s);
// kl_last: the last epoch's XH_BUF_KL record, or nullptr (not KL-PPO).
// pclip / vclip: this learn()'s clip logs ([psteps][2] and [1][2] of {norm,
// scale}, launch_clip_step), or nullptr while clipping is off for that net
hipError_t launch_learner_row(const double *part, int nparts,
                              const double *norms, const float *kl_last,
                              const double *pclip, int psteps,
                              const double *vclip, double *row, hipStream_t s);
// PPO update diagnostics (xh_trainer_set_update_diag, opt-in): a forward of
// the updated policy over the batch's T * N transitions that leaves one
// record per (slot, env) (policy_kernels.hip: policy_diag_kernel, f32 MFMA,
// every shape; policy_diag_split_kernel, f16 pairs, the shapes
// rollout_split_kernel serves), then their sums into a row of XH_UPD_COUNT
// doubles (diag_kernels.hip), in double, fixed order, no floating-point
// atomics.
struct DiagArgs {
  EnvDesc env;
  Batch b;
  const float *params;  // the policy after the update
  const float *q;       // [T][N][B] the sampling distributions, or nullptr
  float *p_new;         // [T][N] probability of the action taken
  double *ent;          // [T][N] entropy of the row's distribution
  double *kl;           // [T][N] KL(q || p); NaN without q
};
constexpr int kUpdSums = 7;  // row entries LOGR_SUM .. KL_SUM
// wide: a slot of the batch holds a bin below -capacity (RolloutArgs::wide):
// the f32 form runs, as it does under XH_ROLLOUT_KERNEL=f32 / =4
hipError_t launch_policy_diag(const DiagArgs &a, int H1, int H2, int wide,
                              int grid, hipStream_t s, KernelInfo *info);
// part[gae_grid(N)][kUpdSums]: the workgroup partials of the xh_diag.h terms
// of every row (p_new, pold, adv) and of the entropy and KL records
hipError_t launch_update_diag_sum(const float *p_new, const float *pold,
                                  const float *adv, const double *ent,
                                  const double *kl, int N, int T, float clip_eps,
                                  double *part, hipStream_t s);
// their fixed-order sum (this rank's share) into row[XH_UPD_LOGR_SUM ..], with
// row[XH_UPD_LEARN] = learn and row[XH_UPD_ROWS] = rows_global
hipError_t launch_update_diag_row(const double *part, int nparts, double learn,
                                  double rows_global, double *row,
                                  hipStream_t s);

// Slab entries the value net's reduced layer 0 leaves unwritten: the item
// columns of bins b > 0 of its first [rows][in] block, whose sums equal bin
// 0's (EpSlabRed).  B = 0: none.
struct SlabAlias {
  int rows, in, B, D;
};
hipError_t launch_slab_reduce(const float *slab, int nslab, int stride, int n,
                              float *out, hipStream_t s,
                              SlabAlias al = SlabAlias{0, 0, 0, 0});
hipError_t launch_sgd(float *params, const float *grad, int n, float lr,
                      float wd, hipStream_t s);
// momentum_optimizer (kind 1) / adam_optimizer (kind 2), nn.h:630-698: state
// m (velocity / first moment) and v (second moment); c1, c2 = adam's bias
// corrections 1 - beta^t computed on the host as the reference does.
struct OptStep {
  int kind;  // XH_OPT_SGD / XH_OPT_MOMENTUM / XH_OPT_ADAM
  float lr, beta1, beta2, c1, c2;
  float wd;  // sgd weight decay
};
hipError_t launch_opt(float *params, const float *grad, float *m, float *v,
                      int n, OptStep o, hipStream_t s);
// Single-rank fusion of launch_slab_reduce and the optimizer step: the same
// fixed-order slab sum (written to out) and the same per-element update.
hipError_t launch_slab_reduce_opt(const float *slab, int nslab, int stride,
                                  int n, float *out, float *params, float *m,
                                  float *v, OptStep o, hipStream_t s,
                                  SlabAlias al = SlabAlias{0, 0, 0, 0});

// Global-norm gradient clipping (clip_kernels.hip; xh_trainer_set_grad_clip,
// xh_clip_grad_norm).  launch_clip_sumsq: part[clip_parts(n)] = the workgroup
// partials of sum g[i]^2 in double (clip_parts(n) <= kClipMaxParts, a function
// of n only).  launch_clip_step: their fixed-order sum ss, norm = sqrt(ss) *
// r, scale (xh_clip.h), then the optimizer update o on g[i] * scale; with
// scaled != nullptr it writes g[i] * scale there and steps nothing.
// log[0..2) = {norm, (double)scale}.  g is not modified.
constexpr int kClipMaxParts = 256;
int clip_parts(int n);
hipError_t launch_clip_sumsq(const float *g, int n, double *part,
                             hipStream_t s);
hipError_t launch_clip_step(const double *part, double r, float max_norm,
                            const float *g, float *params, float *m, float *v,
                            int n, OptStep o, float *scaled, double *log,
                            hipStream_t s);

// The state digest of up to kDigestMaxEntries device arrays in one launch
// pair (digest_kernels.hip; xh_trainer_state_digest, xh_trainer_load_state):
// out[k] = sum_i splitmix64((i << 32) | word_i) mod 2^64 over the 32-bit words
// of e[k] (xh_digest.h), 0 for an empty entry.  An entry may start at any byte
// address and have any byte count; nothing outside [ptr, ptr + bytes) is read.
// ws: kDigestWsWords uint64 of device workspace -- the workgroup partials
// [kDigestMaxEntries][kDigestBlocks], then the kDigestMaxEntries results.
constexpr int kDigestMaxEntries = 10;  // XH_DIG_COUNT
constexpr int kDigestBlocks = 128;
constexpr int kDigestWsWords = kDigestMaxEntries * (kDigestBlocks + 1);
struct DigestTable {
  struct {
    const void *ptr;
    unsigned long long bytes;
  } e[kDigestMaxEntries];
  int n;
};
inline unsigned long long *digest_results(unsigned long long *ws) {
  return ws + kDigestMaxEntries * kDigestBlocks;
}
hipError_t launch_digest(const DigestTable &tab, unsigned long long *ws,
                         hipStream_t s);

// xylo/tensor.{h,cc} arithmetic on device arrays (tensor_kernels.hip; the
// drop-in tensor type's device tensors and large host operations).
enum TensorMapOp {
  kTensorAdd = 0, kTensorMinus = 1, kTensorMultiply = 2, kTensorDivide = 3,
  kTensorAddS = 4, kTensorMinusS = 5, kTensorMultiplyS = 6, kTensorDivideS = 7,
  kTensorAbs = 8, kTensorSin = 9, kTensorExp = 10, kTensorLog = 11,
  kTensorSqrt = 12, kTensorFill = 13, kTensorRMinusS = 14, kTensorRDivideS = 15
};
enum TensorReduceOp {
  kTensorSum = 0, kTensorDot = 1, kTensorSqDev = 2, kTensorMax = 3,
  kTensorArgmax = 4
};
// out[i] = op(a[i], b[i], s) for i < n (b: the binary ops; s: the scalar ops
// and fill)
hipError_t launch_tensor_map(int op, const float *a, const float *b, float s,
                             float *out, long n, hipStream_t st);
// workgroup partials of a reduction over n elements; scratch holds
// tensor_reduce_parts(n) + 1 records of 16 bytes, the result (double value,
// int64 index) in the last
int tensor_reduce_parts(long n);
hipError_t launch_tensor_reduce(int op, const float *a, const float *b, float s,
                                long n, void *scratch, hipStream_t st);
hipError_t launch_tensor_transpose(const float *in, float *out, int rows,
                                   int cols, hipStream_t st);
// C[m][n] = sum_k A[m][k] B(n, k): b_nk = B is [N][K] (matmul_transposed,
// tensor.cc:218-227), else B is [K][N] (matmul, :228-230); the Dense f32-MFMA
// GEMM (dense_kernels.hip)
hipError_t launch_tensor_gemm(bool b_nk, const float *A, const float *B,
                              float *C, int M, int N, int K, hipStream_t st);

}  // namespace xh
