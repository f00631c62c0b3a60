// venv_kernels.hip -- N bp::environment instances stepped by ONE kernel per
// call, for callers that bring their own policy (xh_venv_*, include/
// xylo_hip.h).  Reference: bp::environment::apply/view/reset
// (bin_packing.h:53-70, get_item :76-81), bp::agent::game_over/get_reward
// (:94-106), xylo::agent::step minus the policy's react (rl.h:325-349),
// observation::to_vector (bin_packing.h:31-40); generalised to B bins and D
// dims as the trainer's env (xh_host.h make_env).
//
// Layout in HBM: bins int8 [N][B][D], items int8 [N][4], rng u32 [N] (one
// minstd_rand0 state per env).  A lane owns one (env, bin) pair (two bins per
// lane at B = 128), so a wave covers 64 / B envs with fully coalesced int8
// row loads; the env's verdicts (game over = any bin negative) are segment
// ballots and the item / RNG / reward record is written by the env's bin-0
// lane.  HBM-bound: 2 * B * D + 4 + 4 + 4 + 1 bytes per env step (+ 8 with
// episode statistics on: the env's running length, venv_ep_count).
// venv_act_kernel (xh_venv_act) picks the action from the caller's policy
// row first -- react's sampling -- and writes the trajectory record.
// The instance (item shapes, their probabilities, the capacity) is make_env's
// at compile time, or -- the general instantiations, with a VenvItemTable as
// a second kernel argument -- an xh_item_set's: K <= 16 shapes drawn by a
// K-way threshold search on the same canonical(x), a capacity per dim.
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_seg.h"
#include "xh_venv_device.h"
#include "xh_vstore.h"

namespace xh {

// The step / act layout (VStepShape), the instance helpers (venv_cap,
// venv_capf, venv_draw), xcd_block, venv_ep_count, the legal-set helpers and
// the first-maximum pick are in xh_venv_device.h, the sampled pick in
// xh_venv_sample.inc: shared with venv_heur_kernels.hip.
template <int B, int D>
struct VShape {
  static constexpr int BPL = B > 64 ? B / 64 : 1;  // bins per lane
  static constexpr int LPE = B / BPL;               // lanes per env
  static constexpr int EPW = 64 / LPE;              // envs per wave
  static constexpr int BD = B * D;
};

template <int B, int D, class... IT>
__device__ __forceinline__ void venv_obs_row(const int8_t *bp, const int8_t *ip,
                                             float *o, const IT &...t) {
#pragma unroll
  for (int d = 0; d < D; ++d) {
    o[d] = (float)bp[d] / venv_capf(d, t...);
    o[D + d] = (float)ip[d] / venv_capf(d, t...);
  }
}

// mode 0: environment::apply for every (masked) env -- bins[a] -= item; a new
// item (2 draws) unless that bin went negative; done[e] = game_over after it.
// mode 1: agent::step minus react -- skip the policy's draws, apply, reward =
// game_over ? 0 : 1, reset (2 draws) on game over, then the env's stream
// jumps over the other envs' draws of this step (reference order).
// Every global load is issued first and unconditionally (an out-of-range
// lane reads env 0's words; a masked or refused env's values are not used),
// so their latencies overlap: one HBM round trip before the arithmetic
// instead of three dependent ones (action -> item / bins -> stream state).
template <int B, int D, bool EP, class... IT>
__global__ __launch_bounds__(256) void venv_step_kernel(VenvArgs a, IT... t) {
  using S = VStepShape<B, D>;
  const int lane = threadIdx.x & 63;
  const int wave = (xcd_block() * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int env = wave * S::EPW + el;
  const int seg0 = el * S::LPE;
  const bool in_range = env < a.N;
  const size_t ec = in_range ? (size_t)env : 0;
  int8_t *bp = a.bins + ec * S::BD;
  int8_t *ip = a.items + ec * 4;
  const int act_raw = a.action[ec];
  const bool masked_in = !a.mask || a.mask[ec];
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);
  uint32_t x = a.rng[ec];
  [[maybe_unused]] int run = 0;  // the episode in flight (EP)
  if constexpr (EP) run = a.ep_running[ec];
  // this lane's bins li BPL .. li BPL + BPL - 1: NW words, byte k D + d =
  // bin k, dim d
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) wv[q] = wp[q];
  int v[S::BPL][D];
#pragma unroll
  for (int k = 0; k < S::BPL; ++k)
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = k * D + d;
      v[k][d] = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
    }

  const bool on = in_range && masked_in;
  int act = on ? act_raw : 0;
  if (on && (act < 0 || act >= B)) {  // refuse the env, flag the call
    if (li == 0) atomicOr(a.err, 1);
    act = -1;
  }
  const bool live = on && act >= 0;
  int item[D];
#pragma unroll
  for (int d = 0; d < D; ++d) item[d] = live ? (int)(signed char)((itw >> (8 * d)) & 0xff) : 0;
  int nb[S::BPL][D];
  int neg_any = 0, neg_chosen = 0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    const int bin = li * S::BPL + k;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int vv = live ? v[k][d] : 0;
      nb[k][d] = bin == act ? vv - item[d] : vv;
      neg_any |= nb[k][d] < 0;
      if (bin == act) neg_chosen |= nb[k][d] < 0;
    }
  }
  // segment verdicts (every lane of the env gets them)
  unsigned long long segmask = S::LPE == 64 ? ~0ull
                                            : ((1ull << S::LPE) - 1ull) << seg0;
  const bool over = (__ballot(neg_any) & segmask) != 0;
  const bool chosen_over = (__ballot(neg_chosen) & segmask) != 0;
  if (!live) {
    // an env not applied (masked out, or its action refused) reports no game
    // over for this call: DONE holds this call's verdicts only
    if (in_range && li == 0 && a.done) a.done[env] = 0;
    return;
  }
  if (a.mode == 1) x = mstd_mulmod(x, a.skip_mul);  // the policy's draws
  const bool reset = a.mode == 1 && over;
  {
    uint32_t ow[S::NW];
#pragma unroll
    for (int q = 0; q < S::NW; ++q) ow[q] = 0u;
#pragma unroll
    for (int k = 0; k < S::BPL; ++k)
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int j = k * D + d;
        ow[j >> 2] |= (uint32_t)((reset ? venv_cap(d, t...) : nb[k][d]) & 0xff) << (8 * (j & 3));
      }
    uint32_t *op = reinterpret_cast<uint32_t *>(
        __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
#pragma unroll
    for (int q = 0; q < S::NW; ++q) op[q] = ow[q];
  }
  // every lane of the env draws the same item (redundant, register-only: no
  // cross-lane hand-off of the new item); the bin-0 lane writes the record
  int8_t nit[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) nit[d] = d < D ? (int8_t)item[d] : 0;
  if (!chosen_over) venv_draw(a.env, x, nit, t...);  // apply's get_item
  if (reset) venv_draw(a.env, x, nit, t...);         // reset's get_item
  if (a.mode == 1) x = mstd_mulmod(x, a.jump_mul);
  if (li == 0) {
    *reinterpret_cast<unsigned *>(ip) = (unsigned)(uint8_t)nit[0] |
                                        ((unsigned)(uint8_t)nit[1] << 8) |
                                        ((unsigned)(uint8_t)nit[2] << 16) |
                                        ((unsigned)(uint8_t)nit[3] << 24);
    if (a.mode == 1 && a.reward) a.reward[env] = over ? 0.0f : 1.0f;
    if (a.done) a.done[env] = (uint8_t)over;
    a.rng[env] = x;
    if constexpr (EP) venv_ep_count(a, env, run, over);
  }
  if (a.obs) {  // observation::to_vector of the resulting state
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) {
      const int bin = li * S::BPL + k;
      float *o = a.obs + ((size_t)env * B + bin) * 2 * D;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        o[d] = (float)(reset ? venv_cap(d, t...) : nb[k][d]) / venv_capf(d, t...);
        o[D + d] = (float)nit[d] / venv_capf(d, t...);
      }
    }
  }
}

// ------------------------------------------------------------------ act --
// xh_venv_act: policy_gradient_policy::react's pick (policy_gradient.h:343-350,
// discrete_action::from_vector rl.h:27-30) from the caller's policy row, then
// agent::step with it (rl.h:325-349) -- venv_step_kernel's mode 1 with the
// action produced here instead of read.
//
// Layout: the step kernel's (VStepShape): a lane owns XH_VENV_BPL (16)
// consecutive bins of one env -- their int8 words and their 16 policy floats,
// read as 16-byte loads -- so B / 16 lanes (at most 8) share an env.  Every
// global load (row, bins, item, stream state) is issued first and
// unconditionally, as in venv_step_kernel; an out-of-range lane reads env
// 0's and a refused env's values are not used.
//
// The pick.  std::discrete_distribution (or_discrete) divides each double
// p_j by the sequential double sum, accumulates the quotients sequentially,
// sets the last entry to 1.0 and takes the lower bound of u.  Here the lane
// keeps its bins' partial sums unnormalised, C_k = (sum of the env's earlier
// lanes) + p_first + .. + p_k in double (the lane's own terms sequentially,
// the lanes' totals by a scan and an xor butterfly), and counts C_k < u sd,
// sd the env's sum: no division per bin.  C_k / sd differs from the
// reference's k-th boundary only by rounding -- the two summation orders of
// at most 128 non-negative terms, one division per term, and the product u
// sd: under (3 B + 2) 2^-53 < 5e-14 relative to a table that ends at 1 -- so
// the counts can differ only when a boundary lies that close to u.  Whenever
// some |C_k - u sd| < 1e-9 sd the env's lanes restate the table in the
// reference's order (the row's floats shuffled in bin order) and take that
// pick.
//
// Logits: p_j = e_j / se with e_j = expf(z_j - m), m the row's maximum, all
// f32; se adds the lane's e_j in bin order, then the env's lanes' sums by
// seg_sum's xor butterfly (partners 1, 2, 4): seg_softmax (xh_seg.h), the
// text venv_policy_loss_kernel compiles too.
//
// A row is refused (env untouched, DONE 0, error bit 2) when a probability is
// NaN or negative or the double-precision sum is zero or not finite.
//
// RD: the instantiation that also records the distribution (a.rec_distrib,
// xh_venv_set_record_distrib): row slot N + env of [T][N][B] receives the p[]
// the pick was made from, zeros for a refused env.  A lane's 16 floats are one
// 64-byte run and the wave's envs are consecutive, so the wave's block is
// contiguous: vloss_store (xh_vstore.h), the LDS exchange into whole-line
// nontemporal stores.  Its barriers stand BEFORE the kernel's first early
// return, where every lane of the workgroup still runs; lanes past N store
// nothing.  -DXH_VACT_OWNER_STORES=1 (make variant VSRC=venv_kernels) stores
// 16-byte pieces from the owning lanes instead; the two times are in
// DESIGN.md 3.2.  The other instantiation holds none of this.
#ifndef XH_VACT_OWNER_STORES
#define XH_VACT_OWNER_STORES 0
#endif
constexpr bool kVActOwner = XH_VACT_OWNER_STORES != 0;

// Legal sets (invalid-action masking): venv_legal_bits / venv_eff_bits /
// venv_legal_words / venv_store_words, xh_venv_device.h.
//
// xh_venv_legal: eff of every env's current state, out [N][W].  The act
// kernel's layout and decode; reads bins and items, writes nothing else.
template <int B, int D>
__global__ __launch_bounds__(256) void venv_legal_kernel(VenvArgs a,
                                                         uint32_t *out) {
  using S = VStepShape<B, D>;
  const int lane = threadIdx.x & 63;
  const int wave = (xcd_block() * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int env = wave * S::EPW + el;
  const int seg0 = el * S::LPE;
  const bool in_range = env < a.N;
  const size_t ec = in_range ? (size_t)env : 0;
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(a.bins + ec * S::BD + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) wv[q] = wp[q];
  const unsigned itw = *reinterpret_cast<const unsigned *>(a.items + ec * 4);
  const unsigned long long segmask =
      S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
  const uint32_t eb =
      venv_eff_bits<B, D>(venv_legal_bits<B, D>(wv, itw), segmask);
  uint32_t wd[VLegal<B>::W];
  venv_legal_words<B, D>(eb, seg0, wd);
  if (in_range && li == 0)
    venv_store_words<VLegal<B>::W>(out + (size_t)env * VLegal<B>::W, wd);
}

// MASK (a.legal, xh_venv_set_action_mask): entry k of the row outside eff(e)
// is replaced right after the loads, before anything reads it -- by -inf
// under logits, by +0.0f under probabilities, in both pick modes -- so the
// call does bit for bit what the other instantiation does on the premasked
// rows: expf(-inf - m) is exactly 0, m is the maximum of the legal entries,
// and adding zeros changes no sum.  A NaN in a replaced entry is not seen; a
// probability row whose legal entries sum to zero is refused as a zero-sum
// row.  The words it masked with go to a.rec_legal's slot (where not null),
// also for a refused env: they are a function of the state before the step.
// The other instantiation holds none of this.
template <int B, int D, bool RD, bool MASK, bool EP, class... IT>
__global__ __launch_bounds__(256) void venv_act_kernel(VenvActArgs a,
                                                       IT... t) {
  using S = VStepShape<B, D>;
  static_assert(S::BPL % 4 == 0, "the lane's floats as 16-byte loads");
  static_assert(!RD || (S::BPL == VLossShape<B>::BPL && S::EPW ==
                                                          VLossShape<B>::RPW),
                "the distribution record is stored in vloss_store's layout");
  const int lane = threadIdx.x & 63;
  const int wave = (xcd_block() * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int env = wave * S::EPW + el;
  const int seg0 = el * S::LPE;
  const bool in_range = env < a.v.N;
  const size_t ec = in_range ? (size_t)env : 0;
  int8_t *bp = a.v.bins + ec * S::BD;
  int8_t *ip = a.v.items + ec * 4;
  // every load first
  float z[S::BPL];
  {
    const float4 *zp = reinterpret_cast<const float4 *>(
        __builtin_assume_aligned(a.policy + ec * B + li * S::BPL, 16));
#pragma unroll
    for (int q = 0; q < S::BPL / 4; ++q) {
      const float4 t = zp[q];
      z[4 * q] = t.x;
      z[4 * q + 1] = t.y;
      z[4 * q + 2] = t.z;
      z[4 * q + 3] = t.w;
    }
  }
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) wv[q] = wp[q];
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);
  uint32_t x = a.v.rng[ec];
  [[maybe_unused]] int run = 0;  // the episode in flight (EP)
  if constexpr (EP) run = a.v.ep_running[ec];

  [[maybe_unused]] uint32_t eb = 0u;  // the lane's bits of eff(e) (MASK)
  if constexpr (MASK) {
    // the premasked row: everything below reads z[] as if the caller had
    // passed it this way
    const unsigned long long sm =
        S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
    eb = venv_eff_bits<B, D>(venv_legal_bits<B, D>(wv, itw), sm);
    const float out = a.logits ? -INFINITY : 0.0f;
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) z[k] = (eb >> k) & 1u ? z[k] : out;
  }

  // the row's probabilities
  float p[S::BPL];
  if (a.logits) {
    seg_softmax<S::LPE, S::BPL>(z, p);  // xh_seg.h
  } else {
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) p[k] = z[k];
  }
  bool bad = false;
  double lsum = 0.0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    bad |= !(p[k] >= 0.0f);  // NaN or negative
    lsum += (double)p[k];
  }
  const double sd = seg_sum_d<S::LPE>(lsum);
  bad |= !(sd > 0.0 && sd < (double)INFINITY);
  const unsigned long long segmask =
      S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
  const bool refused = (__ballot(bad) & segmask) != 0;

  // the pick (all lanes: the cross-lane steps need the whole wave)
  int choice;
  if (a.argmax) {  // first maximum of the values as given (tensor.cc:464-466)
    choice = venv_pick_argmax<B, D>(z, li);
    x = mstd_mulmod(x, a.v.skip_mul);  // the venv's policy draws, unused
  } else  // the sampled pick's statements, shared with venv_heur_kernel
#include "xh_venv_sample.inc"
  choice = refused ? 0 : choice & (B - 1);
  float pmine = p[0];
#pragma unroll
  for (int k = 1; k < S::BPL; ++k) pmine = k == (choice % S::BPL) ? p[k] : pmine;
  const float pc = wave_shfl(pmine, seg0 + choice / S::BPL);
  if constexpr (RD) {
    // every lane of the workgroup is still here (the first return is below)
    __shared__ vl_f4 stage[4][64 * VLossShape<B>::F4];
    float pr[S::BPL];
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) pr[k] = refused ? 0.0f : p[k];
    const size_t wo =
        ((size_t)a.slot * a.v.N + (size_t)wave * S::EPW) * (B / 4);
    vloss_store<B, kVActOwner>(
        pr, stage[threadIdx.x >> 6], lane, __ballot(in_range),
        reinterpret_cast<vl_f4 *>(__builtin_assume_aligned(a.rec_distrib, 16)) +
            wo);
  }

  int v[S::BPL][D];
#pragma unroll
  for (int k = 0; k < S::BPL; ++k)
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = k * D + d;
      v[k][d] = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
  const bool live = in_range && !refused;
  int item[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    item[d] = live ? (int)(signed char)((itw >> (8 * d)) & 0xff) : 0;
  int nb[S::BPL][D];
  int neg_any = 0, neg_chosen = 0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    const int bin = li * S::BPL + k;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int vv = live ? v[k][d] : 0;
      nb[k][d] = bin == choice ? vv - item[d] : vv;
      neg_any |= nb[k][d] < 0;
      if (bin == choice) neg_chosen |= nb[k][d] < 0;
    }
  }
  const bool over = (__ballot(neg_any) & segmask) != 0;
  const bool chosen_over = (__ballot(neg_chosen) & segmask) != 0;
  [[maybe_unused]] uint32_t lw[VLegal<B>::W];  // the env's words (every lane
                                               // takes part in the shuffles)
  if constexpr (MASK) venv_legal_words<B, D>(eb, seg0, lw);
  if (!in_range) return;

  // the record's slot: the state before the step (also of a refused env)
  const size_t ro = (size_t)a.slot * a.v.N + env;
  if constexpr (MASK) {
    if (a.rec_legal && li == 0)
      venv_store_words<VLegal<B>::W>(a.rec_legal + ro * VLegal<B>::W, lw);
  }
  if (a.rec_bins) {
    uint32_t *rp = reinterpret_cast<uint32_t *>(__builtin_assume_aligned(
        a.rec_bins + ro * S::BD + li * S::BPL * D, S::ALIGN));
#pragma unroll
    for (int q = 0; q < S::NW; ++q) rp[q] = wv[q];
    if (li == 0) *reinterpret_cast<unsigned *>(a.rec_items + ro * 4) = itw;
  }
  if (refused) {
    if (li == 0) {
      atomicOr(a.v.err, 2);
      a.v.done[env] = 0;
      if (a.rec_action) {
        a.rec_action[ro] = 0;
        a.rec_pchoice[ro] = 0.0f;
        a.rec_reward[ro] = 0.0f;
        a.rec_done[ro] = 0;
      }
    }
    return;
  }
  const bool reset = over;
  {
    uint32_t ow[S::NW];
#pragma unroll
    for (int q = 0; q < S::NW; ++q) ow[q] = 0u;
#pragma unroll
    for (int k = 0; k < S::BPL; ++k)
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int j = k * D + d;
        nb[k][d] = reset ? venv_cap(d, t...) : nb[k][d];
        ow[j >> 2] |= (uint32_t)(nb[k][d] & 0xff) << (8 * (j & 3));
      }
    uint32_t *op = reinterpret_cast<uint32_t *>(
        __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
#pragma unroll
    for (int q = 0; q < S::NW; ++q) op[q] = ow[q];
  }
  // every lane of the env draws the same item (register-only), as in the
  // step kernel; the bin-0 lane writes the record
  int8_t nit[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) nit[d] = d < D ? (int8_t)item[d] : 0;
  if (!chosen_over) venv_draw(a.v.env, x, nit, t...);  // apply's get_item
  if (reset) venv_draw(a.v.env, x, nit, t...);         // reset's get_item
  x = mstd_mulmod(x, a.v.jump_mul);
  if (li == 0) {
    const float rew = over ? 0.0f : 1.0f;
    *reinterpret_cast<unsigned *>(ip) = (unsigned)(uint8_t)nit[0] |
                                        ((unsigned)(uint8_t)nit[1] << 8) |
                                        ((unsigned)(uint8_t)nit[2] << 16) |
                                        ((unsigned)(uint8_t)nit[3] << 24);
    a.action[env] = choice;
    a.pchoice[env] = pc;
    a.v.reward[env] = rew;
    a.v.done[env] = (uint8_t)over;
    a.v.rng[env] = x;
    if (a.rec_action) {
      a.rec_action[ro] = choice;
      a.rec_pchoice[ro] = pc;
      a.rec_reward[ro] = rew;
      a.rec_done[ro] = (uint8_t)over;
    }
    if constexpr (EP) venv_ep_count(a.v, env, run, over);
  }
  if (a.v.obs) {  // observation::to_vector of the resulting state
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) {
      float *o = a.v.obs + ((size_t)env * B + li * S::BPL + k) * 2 * D;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        o[d] = (float)nb[k][d] / venv_capf(d, t...);
        o[D + d] = (float)nit[d] / venv_capf(d, t...);
      }
    }
  }
}

// environment::reset for every (masked) env: bins at capacity, get_item.
template <int B, int D, class... IT>
__global__ __launch_bounds__(256) void venv_reset_kernel(VenvArgs a, IT... t) {
  using S = VShape<B, D>;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int env = wave * S::EPW + el;
  if (env >= a.N || (a.mask && !a.mask[env])) return;
  int8_t *bp = a.bins + (size_t)env * S::BD;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k)
#pragma unroll
    for (int d = 0; d < D; ++d)
      bp[(k * 64 + li) * D + d] = (int8_t)venv_cap(d, t...);
  if (li == 0) {
    uint32_t x = a.rng[env];
    venv_draw(a.env, x, a.items + (size_t)env * 4, t...);
    a.rng[env] = x;
    // the abandoned episode is not counted
    if (a.ep_running) a.ep_running[env] = 0;
  }
}

// observation::to_vector of every env: obs [N][B][2D] f32.
template <int B, int D, class... IT>
__global__ __launch_bounds__(256) void venv_observe_kernel(VenvArgs a,
                                                           IT... t) {
  using S = VShape<B, D>;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int env = wave * S::EPW + el;
  if (env >= a.N) return;
  const int8_t *bp = a.bins + (size_t)env * S::BD;
  const int8_t *ip = a.items + (size_t)env * 4;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    const int bin = k * 64 + li;
    venv_obs_row<B, D>(bp + bin * D, ip,
                       a.obs + ((size_t)env * B + bin) * 2 * D, t...);
  }
}

// Construction (bin_packing.h:50-52): env g (global) draws its item at engine
// position 2g (envs constructed one after another), then its stream moves to
// its first step position 2 Ng + k g (k = draws per env per step).
template <class... IT>
__global__ void venv_init_kernel(VenvArgs a, uint32_t x0, int env_offset,
                                 int n_global, int k, IT... t) {
  const int BD = a.env.B * a.env.D;
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < a.N;
       env += gridDim.x * blockDim.x) {
    const uint64_t g = (uint64_t)env_offset + env;
    uint32_t x = mstd_jump(x0, 2 * g);
    for (int i = 0; i < BD; ++i)
      a.bins[(size_t)env * BD + i] = (int8_t)venv_cap(i % a.env.D, t...);
    venv_draw(a.env, x, a.items + (size_t)env * 4, t...);
    const uint64_t target = 2ull * n_global + (uint64_t)k * g;
    a.rng[env] = mstd_jump(x, target - (2 * g + 2));
  }
}

// ------------------------------------------------------------- launchers --
// A kernel exists in the object whose launcher names it: the builtin ones in
// venv_kernels.o, the general ones in venv_gen_kernels.o (this file with
// -DXH_VENV_GEN_TU=1, so the two sets of act instantiations compile side by
// side).  This object's launches, generic in the pack: t is nothing, or the
// item table.
#ifndef XH_VENV_GEN_TU
#define XH_VENV_GEN_TU 0
#endif
#if !XH_VENV_GEN_TU
bool venv_shape_supported(int B, int D) {
#define X(XB, XD) if (B == XB && D == XD) return true;
  XH_VENV_SHAPES(X)
#undef X
  return false;
}
#endif

static dim3 venv_grid(int N, int B) {
  const int epw = B >= 64 ? 1 : 64 / B;
  const long waves = (N + epw - 1) / epw;
  return dim3((unsigned)((waves + 3) / 4));
}

template <class... IT>
static hipError_t venv_launch_inst(const VenvArgs &a, int op, hipStream_t s,
                                   const IT &...t) {
  const int B = a.env.B, D = a.env.D;
  if (a.N <= 0) return hipSuccess;
#define X(XB, XD)                                                            \
  if (B == XB && D == XD) {                                                  \
    if (op == kVenvStep && a.ep_running)                                     \
      hipLaunchKernelGGL((venv_step_kernel<XB, XD, true, IT...>),            \
                         venv_step_grid(a.N, B), dim3(256), 0, s, a, t...);  \
    else if (op == kVenvStep)                                                \
      hipLaunchKernelGGL((venv_step_kernel<XB, XD, false, IT...>),           \
                         venv_step_grid(a.N, B), dim3(256), 0, s, a, t...);  \
    else if (op == kVenvReset)                                               \
      hipLaunchKernelGGL((venv_reset_kernel<XB, XD, IT...>),                 \
                         venv_grid(a.N, B), dim3(256), 0, s, a, t...);       \
    else                                                                     \
      hipLaunchKernelGGL((venv_observe_kernel<XB, XD, IT...>),               \
                         venv_grid(a.N, B), dim3(256), 0, s, a, t...);       \
    return hipGetLastError();                                                \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

// RD where the call records its distributions, MASK where it masks, EP where
// it counts episodes
template <int B, int D, bool RD, bool MASK, class... IT>
static void vact_launch_ep(const VenvActArgs &a, hipStream_t s,
                           const IT &...t) {
  const dim3 grid = venv_step_grid(a.v.N, B);
  if (a.v.ep_running)
    hipLaunchKernelGGL((venv_act_kernel<B, D, RD, MASK, true, IT...>), grid,
                       dim3(256), 0, s, a, t...);
  else
    hipLaunchKernelGGL((venv_act_kernel<B, D, RD, MASK, false, IT...>), grid,
                       dim3(256), 0, s, a, t...);
}

template <int B, int D, class... IT>
static void vact_launch(const VenvActArgs &a, hipStream_t s, const IT &...t) {
  if (a.legal) {
    if (a.rec_distrib)
      vact_launch_ep<B, D, true, true>(a, s, t...);
    else
      vact_launch_ep<B, D, false, true>(a, s, t...);
  } else {
    if (a.rec_distrib)
      vact_launch_ep<B, D, true, false>(a, s, t...);
    else
      vact_launch_ep<B, D, false, false>(a, s, t...);
  }
}

template <class... IT>
static hipError_t venv_act_launch_inst(const VenvActArgs &a, hipStream_t s,
                                       const IT &...t) {
  const int B = a.v.env.B, D = a.v.env.D;
  if (a.v.N <= 0) return hipSuccess;
#define X(XB, XD)                                                            \
  if (B == XB && D == XD) {                                                  \
    vact_launch<XB, XD>(a, s, t...);                                         \
    return hipGetLastError();                                                \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

#if XH_VENV_GEN_TU
hipError_t launch_venv_gen(const VenvArgs &a, int op, hipStream_t s,
                           const VenvItemTable &items) {
  return venv_launch_inst(a, op, s, items);
}

hipError_t launch_venv_act_gen(const VenvActArgs &a, hipStream_t s,
                               const VenvItemTable &items) {
  return venv_act_launch_inst(a, s, items);
}

hipError_t launch_venv_init_gen(const VenvArgs &a, uint32_t x0, int env_offset,
                                int n_global, int k, hipStream_t s,
                                const VenvItemTable &items) {
  hipLaunchKernelGGL((venv_init_kernel<VenvItemTable>),
                     dim3((a.N + 255) / 256), dim3(256), 0, s, a, x0,
                     env_offset, n_global, k, items);
  return hipGetLastError();
}
#else
hipError_t launch_venv(const VenvArgs &a, int op, hipStream_t s,
                       const VenvItemTable *items) {
  if (items) return launch_venv_gen(a, op, s, *items);
  return venv_launch_inst(a, op, s);
}

hipError_t launch_venv_act(const VenvActArgs &a, hipStream_t s,
                           const VenvItemTable *items) {
  if (items) return launch_venv_act_gen(a, s, *items);
  return venv_act_launch_inst(a, s);
}

hipError_t launch_venv_legal(const VenvArgs &a, uint32_t *out, hipStream_t s) {
  const int B = a.env.B, D = a.env.D;
  if (a.N <= 0) return hipSuccess;
#define X(XB, XD)                                                            \
  if (B == XB && D == XD) {                                                  \
    hipLaunchKernelGGL((venv_legal_kernel<XB, XD>), venv_step_grid(a.N, B),  \
                       dim3(256), 0, s, a, out);                             \
    return hipGetLastError();                                                \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t launch_venv_init(const VenvArgs &a, uint32_t x0, int env_offset,
                            int n_global, int k, hipStream_t s,
                            const VenvItemTable *items) {
  if (items)
    return launch_venv_init_gen(a, x0, env_offset, n_global, k, s, *items);
  hipLaunchKernelGGL((venv_init_kernel<>), dim3((a.N + 255) / 256), dim3(256),
                     0, s, a, x0, env_offset, n_global, k);
  return hipGetLastError();
}
#endif

}  // namespace xh
