// venv_heur_kernels.hip -- xh_venv_act_heuristic: the reference's four
// heuristic agents as an act of the venv, one launch per env step
// (include/xylo_hip.h).  random_policy (rl.h:305-316), firstfit_agent.cc:10-28,
// bestfit_agent.cc:10-30, minwaste_agent.cc:10-39, generalised to B bins, D
// dims, a capacity per dim and items with zero entries; then agent::step with
// the pick, exactly as venv_act_kernel (venv_kernels.hip) does it.
//
// Layout: the act kernel's (VStepShape, xh_venv_device.h): a lane owns 16
// consecutive bins of one env (all of them at 8 bins), B / 16 lanes share an
// env, up to 64 envs a wave; every global load (bins, item, stream state, the
// running length) is issued first and unconditionally; XCD-aware block order;
// the env's bin-0 lane is the only writer of the per-env records.  No policy
// row is loaded: the lane forms its bins' scores in registers from the int8
// words it holds anyway.  HBM: 2 B D + 13 bytes per env step -- the act
// launch's minus its 4 B -- + 8 with episode statistics, + 4 W with the mask
// record.
//
// Scores, bin b of env e, fits = bins[b][d] >= item[d] for every d < D (the
// lane's bits of venv_legal_bits):
//   first-fit  fits ? 1 : 0
//   best-fit   fits ? the f32 sum over d = 0 .. D - 1, in that order, of
//              (item[d] == 0 ? +0 : float(item[d]) / float(bins[b][d])) : -1;
//              the quotient is the IEEE f32 division (a reciprocal multiply
//              gives other bits at bins that are no power of two).  The
//              zero-entry rule is this library's: the reference's expression
//              would form 0 / 0 on an xh_item_set's zero entry
//   min-waste  fits ? (exactly one d has r_d == capacity[d] / 2 and every
//              other d has r_d == 0, r_d = bins[b][d] - item[d] ? 0 : 1) : -1
// and the pick is their first maximum (venv_pick_argmax: the lane's own, then
// the env's lanes by the xor butterfly where the lower index wins on
// equality); no draws, the venv's policy_draws are skipped, PCHOICE = 1.
// The heuristic is a kernel argument, the same for every lane (a scalar
// branch), not a template parameter: four kinds, one instantiation.
//
// Random: the constant row p = (float)(1.0 / B) through the act kernel's
// sampler (xh_venv_sample.inc: the same statements, so the pick is
// xh_venv_act(XH_ACT_PROBS, XH_ACT_SAMPLE)'s on that row bit for bit, its
// near-boundary restatement included); MASK: the premasked constant row,
// entries outside eff(e) +0.0f.
//
// MASK (the action mask is on) and EP (episode statistics are on) are
// instantiations of their own, as in the act kernel, so the plain launch
// carries neither.  MASK changes no deterministic pick -- in all three kinds
// a fitting bin outscores every other, and where nothing fits eff(e) is every
// bin -- it only writes eff(e)'s words into the record.
// No env is refused: there is no caller row.
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_seg.h"
#include "xh_venv_device.h"

namespace xh {

template <int B, int D, bool MASK, bool EP, class... IT>
__global__ __launch_bounds__(256) void venv_heur_kernel(VenvHeurArgs h,
                                                        IT... t) {
  using S = VStepShape<B, D>;
  const VenvActArgs &a = h.a;
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
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) wv[q] = wp[q];
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);
  uint32_t x = a.v.rng[ec];
  [[maybe_unused]] int run = 0;  // the episode in flight (EP)
  if constexpr (EP) run = a.v.ep_running[ec];

  const unsigned long long segmask =
      S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
  // bit k: the lane's k-th bin takes the item
  const uint32_t lb = venv_legal_bits<B, D>(wv, itw);
  [[maybe_unused]] uint32_t eb = 0u;  // the lane's bits of eff(e) (MASK)
  if constexpr (MASK) eb = venv_eff_bits<B, D>(lb, segmask);

  // the pick (all lanes: the cross-lane steps need the whole wave)
  int choice;
  float pc;
  if (h.heur == kHeurRandom) {
    const float u1 = (float)(1.0 / B);
    float p[S::BPL];
    double lsum = 0.0;
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) {
      p[k] = !MASK || ((eb >> k) & 1u) ? u1 : 0.0f;
      lsum += (double)p[k];
    }
    const double sd = seg_sum_d<S::LPE>(lsum);
#include "xh_venv_sample.inc"
    choice &= B - 1;
    float pmine = p[0];
#pragma unroll
    for (int k = 1; k < S::BPL; ++k)
      pmine = k == (choice % S::BPL) ? p[k] : pmine;
    pc = wave_shfl(pmine, seg0 + choice / S::BPL);
  } else {
    int iv[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
      iv[d] = (int)(signed char)((itw >> (8 * d)) & 0xff);
    float z[S::BPL];
    if (h.heur == kHeurBestfit) {
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        float s = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int j = k * D + d;
          const int bv = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
          const float term = iv[d] == 0 ? 0.0f : (float)iv[d] / (float)bv;
          s = d == 0 ? term : s + term;
        }
        z[k] = (lb >> k) & 1u ? s : -1.0f;
      }
    } else if (h.heur == kHeurMinwaste) {
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        int half = 0, zero = 0;  // dims at half the capacity; others at 0
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int j = k * D + d;
          const int bv = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
          const int r = bv - iv[d];
          const bool is_half = r == venv_cap(d, t...) / 2;
          half += is_half;
          zero += !is_half && r == 0;
        }
        const float sc = half == 1 && zero == D - 1 ? 0.0f : 1.0f;
        z[k] = (lb >> k) & 1u ? sc : -1.0f;
      }
    } else {  // first-fit
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) z[k] = (lb >> k) & 1u ? 1.0f : 0.0f;
    }
    choice = venv_pick_argmax<B, D>(z, li) & (B - 1);
    x = mstd_mulmod(x, a.v.skip_mul);  // the venv's policy draws, unused
    pc = 1.0f;
  }

  // agent::step with the pick, venv_act_kernel's with no env refused.  The
  // bins after the apply are packed as they are formed: NW words, not BPL D
  // ints, live across the verdicts' ballots and to the kernel's end (the
  // observation unpacks them again).  An out-of-range lane computes on env
  // 0's words; its ballot bits belong to no env in range and it returns
  // before the first store.
  int item[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    item[d] = (int)(signed char)((itw >> (8 * d)) & 0xff);
  uint32_t ow[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) ow[q] = 0u;
  int neg_any = 0, neg_chosen = 0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    const int bin = li * S::BPL + k;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = k * D + d;
      const int bv = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
      const int nv = bin == choice ? bv - item[d] : bv;
      neg_any |= nv < 0;
      if (bin == choice) neg_chosen |= nv < 0;
      ow[j >> 2] |= (uint32_t)(nv & 0xff) << (8 * (j & 3));
    }
  }
  const bool over = (__ballot(neg_any) & segmask) != 0;
  const bool chosen_over = (__ballot(neg_chosen) & segmask) != 0;
  [[maybe_unused]] uint32_t lw[VLegal<B>::W];  // the env's words (every lane
                                               // takes part in the shuffles)
  if constexpr (MASK) venv_legal_words<B, D>(eb, seg0, lw);
  if (!in_range) return;

  // the record's slot: the state before the step
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
  const bool reset = over;
  if (reset) {  // every bin at capacity: the same words for every lane
#pragma unroll
    for (int q = 0; q < S::NW; ++q) {
      uint32_t cw = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        cw |= (uint32_t)(venv_cap((4 * q + b) % D, t...) & 0xff) << (8 * b);
      ow[q] = cw;
    }
  }
  {
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
        const int j = k * D + d;
        const int nv = (int)(signed char)((ow[j >> 2] >> (8 * (j & 3))) & 0xff);
        o[d] = (float)nv / venv_capf(d, t...);
        o[D + d] = (float)nit[d] / venv_capf(d, t...);
      }
    }
  }
}

// ------------------------------------------------------------- launchers --
// As venv_kernels.hip: the builtin instantiations in venv_heur_kernels.o, the
// general ones in venv_heur_gen_kernels.o (this file with -DXH_VENV_GEN_TU=1).
#ifndef XH_VENV_GEN_TU
#define XH_VENV_GEN_TU 0
#endif

// MASK where the call masks, EP where it counts episodes
template <int B, int D, class... IT>
static void vheur_launch(const VenvHeurArgs &h, hipStream_t s,
                         const IT &...t) {
  const dim3 grid = venv_step_grid(h.a.v.N, B);
  if (h.a.legal) {
    if (h.a.v.ep_running)
      hipLaunchKernelGGL((venv_heur_kernel<B, D, true, true, IT...>), grid,
                         dim3(256), 0, s, h, t...);
    else
      hipLaunchKernelGGL((venv_heur_kernel<B, D, true, false, IT...>), grid,
                         dim3(256), 0, s, h, t...);
  } else {
    if (h.a.v.ep_running)
      hipLaunchKernelGGL((venv_heur_kernel<B, D, false, true, IT...>), grid,
                         dim3(256), 0, s, h, t...);
    else
      hipLaunchKernelGGL((venv_heur_kernel<B, D, false, false, IT...>), grid,
                         dim3(256), 0, s, h, t...);
  }
}

template <class... IT>
static hipError_t venv_heur_launch_inst(const VenvHeurArgs &h, hipStream_t s,
                                        const IT &...t) {
  const int B = h.a.v.env.B, D = h.a.v.env.D;
  if (h.a.v.N <= 0) return hipSuccess;
#define X(XB, XD)                                                            \
  if (B == XB && D == XD) {                                                  \
    vheur_launch<XB, XD>(h, s, t...);                                        \
    return hipGetLastError();                                                \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

#if XH_VENV_GEN_TU
hipError_t launch_venv_heur_gen(const VenvHeurArgs &h, hipStream_t s,
                                const VenvItemTable &items) {
  return venv_heur_launch_inst(h, s, items);
}
#else
hipError_t launch_venv_heur(const VenvHeurArgs &h, hipStream_t s,
                            const VenvItemTable *items) {
  if (items) return launch_venv_heur_gen(h, s, *items);
  return venv_heur_launch_inst(h, s);
}
#endif

}  // namespace xh
