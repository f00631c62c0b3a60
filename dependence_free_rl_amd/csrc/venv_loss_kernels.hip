// venv_loss_kernels.hip -- the PPO / actor-critic loss head of a caller's own
// network on a window xh_venv_act recorded (xh_venv_policy_loss, include/
// xylo_hip.h): from the network's output rows of a minibatch to dL/d(output)
// in one launch, without leaving HBM:
//   venv_policy_loss_kernel  per output row j: the index q (a shuffle list's
//                            entry or first + j), the gather of action[q],
//                            p_old[q], adv[q] (and target[q]), venv_act_kernel's
//                            softmax of a row of logits (seg_softmax, xh_seg.h:
//                            one text, so p[choice] has the record's bits while
//                            the parameters have not moved), policy_loss
//                            (rl.h:44-52) or clipped_gradient (rl.h:54-74) in
//                            action_loss_kernel's expressions, softmax_layer::
//                            backward (nn.h:393-416) on the one-hot backprop for
//                            logits, square_loss_grad (nn.h:548-550) for the
//                            value head, and the row's diagnostics (diag_terms,
//                            xh_diag.h) in double;
//   venv_loss_reduce_kernel  the call's totals from the block partials, one
//                            wave, fixed order; no floating-point atomics.
// HBM-bound.  Bytes per row: 4 B read (the output row), 4 B written (the
// gradient), another 4 B with probs_out, and about 20 gathered (the index,
// action, p_old, adv, target; + 8 with the value head's values_new / dvalue);
// with XH_LOSS_KL_REGULATED or kl_stats another 4 B gathered (the row's
// sampling distribution); with legal words (xh_venv_policy_loss_masked)
// another 4 W, W = max(1, B / 32); with xh_venv_policy_loss_ex's value clip
// another 4 (v_old) -- its entropy bonus moves no byte.
#include "xh_device.h"
#include "xh_diag.h"
#include "xh_kernels.h"
#include "xh_seg.h"
#include "xh_sums.h"
#include "xh_vstore.h"
#include "../../include/xylo_hip.h"

namespace xh {

// venv_act_kernel's layout (VStepShape): a lane owns 16 consecutive bins of a
// row (all 8 at 8 bins) -- their floats as 16-byte loads in and 16-byte stores
// out -- so B / 16 lanes share a row and a wave covers 64 / (B / 16) rows.
// The stores are vloss_store's (xh_vstore.h): the wave's block exchanged
// through LDS and stored as whole lines, nontemporal (the gradient is read
// once, by the caller's backward).  -DXH_VLOSS_OWNER_STORES=1 (make variant
// VSRC=venv_loss_kernels) stores from the owning lanes instead; the two times
// are in DESIGN.md 3.2.
#ifndef XH_VLOSS_OWNER_STORES
#define XH_VLOSS_OWNER_STORES 0
#endif
constexpr bool kVLossOwner = XH_VLOSS_OWNER_STORES != 0;

// A tile is the 4 RPW consecutive rows of a workgroup's four waves; the
// workgroups stride over the tiles, so a wave reads all RPW rows of its block
// before it stores any of them and no other wave touches them: grad may be
// policy itself.  Lanes past the last row load nothing and store nothing.
// STATS: the instantiation that forms the statistics (a.part != nullptr); the
// other one carries neither the double-precision logarithms nor the sums'
// registers.
// KL: 0 the code without a sampling distribution; 1 each row's distribution
// q = distrib[q] is gathered too (16 more floats per lane) for XH_LOSS_
// KL_REGULATED's gradient (kl_regulated_loss, policy_gradient.h:56-75, in
// action_loss_kernel's expressions); 2 also the row's exact KL(q || p) in
// double for kl_stats (a.kl_part != nullptr; diag_bin_terms' form: a term
// with q_k == 0 is 0, nothing else is masked), under any loss kind.
// MASK (a.legal != nullptr, xh_venv_policy_loss_masked): the row's W = max(1,
// B / 32) legal words are gathered through q beside action[q] -- each lane
// its own half-word (a lane's 16 bins; all 8 bits at 8 bins), 4 W more bytes
// per row, in the round trip of the row's other gathers -- and entry k outside the set is replaced right after the row is
// loaded, by -inf under logits and by +0.0f under probabilities, before
// anything reads it: the launch does bit for bit what the other instantiation
// does on the premasked rows, as venv_act_kernel's MASK does.  A row whose
// words are all zero is left as it is.  The other instantiation holds none of
// this.
// EXT (a.ext != 0, xh_venv_policy_loss_ex): the entropy bonus, PPO2's clipped
// value loss and ext_stats, in the order include/xylo_hip.h gives.  The bonus
// is f32 throughout -- logf, not a double logarithm: sixteen of those per lane
// would move an HBM-bound kernel onto the fp64 pipe, as STATS' do -- on the
// probabilities the row already holds in registers, its row sum S by the
// softmax's own segment reduction.  Whether a call has the bonus (ent_on),
// the value clip (a.v_old) or the sums (a.ext_part) is uniform, as
// a.values_new is.  The other instantiation holds none of this.
template <int B, bool STATS, int KL, bool MASK, bool EXT>
__global__ __launch_bounds__(256) void venv_policy_loss_kernel(VenvLossArgs a) {
#pragma clang fp contract(off)
  using S = VLossShape<B>;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int seg0 = el * S::LPE;
  __shared__ vl_f4 stage[4][64 * S::F4];
  // the lane's sums and what their additions lost (sum2)
  double st[XH_VLOSS_COUNT], sc[XH_VLOSS_COUNT];
#pragma unroll
  for (int k = 0; k < XH_VLOSS_COUNT; ++k) st[k] = sc[k] = 0.0;
  double kt[XH_VKL_COUNT], kc[XH_VKL_COUNT];
#pragma unroll
  for (int k = 0; k < XH_VKL_COUNT; ++k) kt[k] = kc[k] = 0.0;
  float beta = 0.0f;  // the regulation's weight, before this epoch's update
  if constexpr (KL > 0) beta = a.beta_dev ? *a.beta_dev : a.beta;
  [[maybe_unused]] double xt[XH_VEXT_COUNT], xc[XH_VEXT_COUNT];
  [[maybe_unused]] float entc = 0.0f;  // the bonus's weight
  [[maybe_unused]] bool ent_on = false;
  if constexpr (EXT) {
#pragma unroll
    for (int k = 0; k < XH_VEXT_COUNT; ++k) xt[k] = xc[k] = 0.0;
    entc = a.ent_coef_dev ? *a.ent_coef_dev : a.ent_coef;
    ent_on = a.ent_coef_dev || a.ent_coef > 0.0f;
  }

  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long wbase = (tile * 4 + wib) * S::RPW;
    const long j = wbase + el;
    const bool in_range = j < a.count;
    float z[S::BPL];
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) z[k] = 0.0f;
    int ch = 0, ok = 0;
    long long qrow = 0;
    float q_old = 0.0f, A = 0.0f, tg = 0.0f, vn = 0.0f;
    [[maybe_unused]] uint32_t hw = 0u;  // the lane's legal half-word (MASK)
    [[maybe_unused]] float vo = 0.0f;   // v_old[q] (EXT)
    if (in_range) {
      const vl_f4 *zp = reinterpret_cast<const vl_f4 *>(
          __builtin_assume_aligned(a.policy + (size_t)j * B + li * S::BPL, 16));
#pragma unroll
      for (int w = 0; w < S::F4; ++w) {
        const vl_f4 t = zp[w];
        z[4 * w] = t.x;
        z[4 * w + 1] = t.y;
        z[4 * w + 2] = t.z;
        z[4 * w + 3] = t.w;
      }
      if constexpr (MASK) {
        // every lane of the row reads the index itself (one address per row:
        // no more traffic) and gathers its own word beside action[q], in the
        // same round trip -- not a third one behind a shuffle of q
        constexpr int W = B >= 32 ? B / 32 : 1;
        const long qr = a.rows ? (long)a.rows[a.first + j] : a.first + j;
        const long q = qr >= 0 && qr < a.total ? qr : 0;  // a bad index reads
        hw = a.legal[(size_t)q * W + li / 2];             // row 0's
      }
      if (li == 0) {  // the row's gathers: one lane, 4-byte loads
        const long qr = a.rows ? (long)a.rows[a.first + j] : a.first + j;
        const bool qok = qr >= 0 && qr < a.total;
        const long q = qok ? qr : 0;
        ch = a.action[q];
        q_old = a.p_old[q];
        A = a.adv[q];
        if (a.values_new) {
          tg = a.target[q];
          vn = a.values_new[j];
          if constexpr (EXT)
            if (a.v_old) vo = a.v_old[q];
        }
        ok = qok && ch >= 0 && ch < B;
        qrow = q;
        if (!ok) atomicOr(a.err, 4);  // row j of every output stays untouched
      }
    }
    if constexpr (S::LPE > 1) {  // to the row's other lanes
      ch = __shfl(ch, seg0, kWave);
      ok = __shfl(ok, seg0, kWave);
      q_old = wave_shfl(q_old, seg0);
      A = wave_shfl(A, seg0);
    }
    const bool valid = in_range && ok;
    const int chc = valid ? ch : 0;
    if constexpr (KL > 0 && S::LPE > 1) qrow = __shfl(qrow, seg0, kWave);
    if constexpr (MASK) {
      hw = (hw >> (16 * (li & 1))) & ((1u << S::BPL) - 1u);
      const unsigned long long segmask =
          S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
      const bool any = (__ballot(hw != 0u) & segmask) != 0;
      const float out = a.logits ? -INFINITY : 0.0f;
#pragma unroll
      for (int k = 0; k < S::BPL; ++k)
        z[k] = !any || ((hw >> k) & 1u) ? z[k] : out;
    }
    float qd[S::BPL];  // the row's sampling distribution (KL > 0)
    if constexpr (KL > 0) {
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) qd[k] = 0.0f;
      if (in_range) {  // a bad index reads row 0's, as the other gathers do
        const vl_f4 *dp = reinterpret_cast<const vl_f4 *>(
            __builtin_assume_aligned(
                a.distrib + (size_t)qrow * B + li * S::BPL, 16));
#pragma unroll
        for (int w = 0; w < S::F4; ++w) {
          const vl_f4 t = dp[w];
          qd[4 * w] = t.x;
          qd[4 * w + 1] = t.y;
          qd[4 * w + 2] = t.z;
          qd[4 * w + 3] = t.w;
        }
      }
    }

    float p[S::BPL];
    if (a.logits) {
      seg_softmax<S::LPE, S::BPL>(z, p);
    } else {
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) p[k] = z[k];
    }
    float pmine = p[0];
#pragma unroll
    for (int k = 1; k < S::BPL; ++k) pmine = k == (chc % S::BPL) ? p[k] : pmine;
    const float p_ch = wave_shfl(pmine, seg0 + chc / S::BPL);
    // a row xh_venv_act refused: its record entries are zero
    const bool skipped = !(q_old > 0.0f);

    float g[S::BPL];
    if (a.loss == kLossSoftmaxGradientLog) {
      // output = input * advantage; output[choice] -= advantage (rl.h:44-52);
      // through softmax_cross_entropy the same row is the logits' gradient
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        float v = p[k] * A;
        if (li * S::BPL + k == chc) v = v - A;
        g[k] = v;
      }
    } else if (KL > 0 && a.loss == kLossKlRegulated) {
      // softmax_gradient_log + (p - q) * beta (policy_gradient.h:69-73)
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        float v = p[k] * A;
        if (li * S::BPL + k == chc) v = v - A;
        const float reg = (p[k] - qd[k]) * beta;
        v = v + reg;
        g[k] = v;
      }
    } else {  // rl.h:54-74 in action_loss_kernel's expressions
      const float ratio = p_ch / q_old;
      float clipped = ratio;
      if (ratio > 1.0f + a.eps)
        clipped = 1.0f + a.eps;
      else if (ratio < 1.0f - a.eps)
        clipped = 1.0f - a.eps;
      const float x = clipped * A, y = ratio * A;
      const float imp = (y < x ? y : x) * -1.0f;
      const float d = imp / p_ch;
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        const bool mine = li * S::BPL + k == chc;
        if (a.logits) {  // softmax_layer::backward's column `choice` times d
          const float quad = p[k] * p_ch;
          const float pd = (mine ? p[k] : 0.0f) - quad;
          g[k] = pd * d;
        } else {
          g[k] = mine ? d : 0.0f;
        }
      }
    }
    [[maybe_unused]] float psum = 0.0f;  // S = sum_k p_k log p_k of the row
    if constexpr (EXT) {
      if (ent_on) {  // g_k += the gradient of -c H
        float l[S::BPL];
#pragma unroll
        for (int k = 0; k < S::BPL; ++k) {
          l[k] = logf(p[k]);
          const float t = p[k] * l[k];
          psum = p[k] > 0.0f ? psum + t : psum;  // the lane's, in bin order
        }
        psum = seg_sum<S::LPE>(psum);
#pragma unroll
        for (int k = 0; k < S::BPL; ++k) {
          float e;
          if (a.logits) {  // c p_k (log p_k + H)
            const float d = l[k] - psum;
            e = p[k] * d;
            e = e * entc;
          } else {  // c (log p_k + 1): the unconstrained partial
            const float d = l[k] + 1.0f;
            e = d * entc;
          }
          e = p[k] > 0.0f ? e : 0.0f;  // not 0 * -inf
          g[k] = g[k] + e;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) g[k] = skipped ? 0.0f : g[k] * a.scale;
    const float dv = vn - tg;  // square_loss_grad (nn.h:548-550)
    [[maybe_unused]] float e2 = 0.0f;     // the clipped value's error
    [[maybe_unused]] bool vzero = false;  // the clipped branch is the max
    if constexpr (EXT) {
      // the gradient of 0.5 max((v - tg)^2, (v_clip - tg)^2): the clipped
      // branch does not depend on v.  The test is on hit, not on vc != vn:
      // vo + (vn - vo) need not return vn
      if (a.v_old) {
        const float dl = vn - vo;
        const bool hit = dl > a.vclip || dl < -a.vclip;
        const float vc = vo + (dl > a.vclip ? a.vclip : -a.vclip);
        e2 = vc - tg;
        const float s1 = dv * dv, s2 = e2 * e2;
        vzero = hit && s2 > s1;
      }
      if (valid && li == 0 && a.values_new)
        a.dvalue[j] = skipped || vzero ? 0.0f : dv * a.value_scale;
    } else {
      if (valid && li == 0 && a.values_new)
        a.dvalue[j] = skipped ? 0.0f : dv * a.value_scale;
    }
    if constexpr (EXT) {
      if (a.ext_part && valid && !skipped && li == 0) {
        xt[XH_VEXT_ROWS] += 1.0;
        sum2(xt[XH_VEXT_ENTROPY_SUM], xc[XH_VEXT_ENTROPY_SUM],
             (double)(0.0f - psum));
        if (a.values_new) {
          xt[XH_VEXT_VCLIP_ROWS] += vzero ? 1.0 : 0.0;
          sum2(xt[XH_VEXT_VLOSS_SUM], xc[XH_VEXT_VLOSS_SUM],
               vzero ? (double)e2 * (double)e2 : (double)dv * (double)dv);
        }
      }
    }

    if (STATS && valid) {
      if (skipped) {
        if (li == 0) st[XH_VLOSS_SKIPPED] += 1.0;
      } else {
        double h = 0.0;  // the lane's bins of sum p log p, in bin order
#pragma unroll
        for (int k = 0; k < S::BPL; ++k)
          if (p[k] > 0.0f) h += (double)p[k] * log((double)p[k]);
        sum2(st[XH_VLOSS_ENTROPY_SUM], sc[XH_VLOSS_ENTROPY_SUM], -h);
        if (li == 0) {
          const DiagTerms t = diag_terms(p_ch, q_old, A, a.eps);
          st[XH_VLOSS_ROWS] += 1.0;
          st[XH_VLOSS_CLIPPED] += t.clipped;
          sum2(st[XH_VLOSS_LOGR_SUM], sc[XH_VLOSS_LOGR_SUM], t.logr);
          sum2(st[XH_VLOSS_LOGR_SQSUM], sc[XH_VLOSS_LOGR_SQSUM], t.logr2);
          sum2(st[XH_VLOSS_K3_SUM], sc[XH_VLOSS_K3_SUM], t.k3);
          sum2(st[XH_VLOSS_SURR_SUM], sc[XH_VLOSS_SURR_SUM], t.surr);
          if (a.values_new) {
            sum2(st[XH_VLOSS_VERR_SUM], sc[XH_VLOSS_VERR_SUM], (double)dv);
            sum2(st[XH_VLOSS_VERR_SQSUM], sc[XH_VLOSS_VERR_SQSUM],
                 (double)dv * (double)dv);
          }
        }
      }
    }

    if constexpr (KL > 1) {
      // KL(q || p) of the row: the lane's bins in bin order, then the row's
      // lanes by the xor butterfly; every lane takes part in the shuffles
      double kl = 0.0;
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        const double qk = (double)qd[k];
        const double term = qk * (log(qk) - log((double)p[k]));
        kl += qd[k] == 0.0f ? 0.0 : term;
      }
      kl = seg_sum_d<S::LPE>(kl);
      if (valid && !skipped && li == 0) {
        sum2(kt[XH_VKL_KL_SUM], kc[XH_VKL_KL_SUM], kl);
        kt[XH_VKL_ROWS] += 1.0;
        sum2(kt[XH_VKL_KL_SQSUM], kc[XH_VKL_KL_SQSUM], kl * kl);
      }
    }

    const unsigned long long rows_live = __ballot(valid);
    const size_t wo = (size_t)wbase * (B / 4);  // the wave's block, in pieces
    vloss_store<B, kVLossOwner>(g, stage[wib], lane, rows_live,
                   reinterpret_cast<vl_f4 *>(
                       __builtin_assume_aligned(a.grad, 16)) + wo);
    if (a.probs_out)
      vloss_store<B, kVLossOwner>(p, stage[wib], lane, rows_live,
                     reinterpret_cast<vl_f4 *>(
                         __builtin_assume_aligned(a.probs_out, 16)) + wo);
  }
  if constexpr (STATS) {
#pragma unroll
    for (int k = 0; k < XH_VLOSS_COUNT; ++k) st[k] += sc[k];
    block_sums<XH_VLOSS_COUNT>(st,
                               a.part + (size_t)blockIdx.x * XH_VLOSS_COUNT);
  }
  if constexpr (KL > 1) {
#pragma unroll
    for (int k = 0; k < XH_VKL_COUNT; ++k) kt[k] += kc[k];
    block_sums<XH_VKL_COUNT>(kt,
                             a.kl_part + (size_t)blockIdx.x * XH_VKL_COUNT);
  }
  if constexpr (EXT) {
    if (a.ext_part) {
#pragma unroll
      for (int k = 0; k < XH_VEXT_COUNT; ++k) xt[k] += xc[k];
      block_sums<XH_VEXT_COUNT>(
          xt, a.ext_part + (size_t)blockIdx.x * XH_VEXT_COUNT);
    }
  }
}

// stats[k] = (accumulate ? stats[k] : 0) + the column sums of part[nparts]
// [S] (S = XH_VLOSS_COUNT for stats, XH_VKL_COUNT for kl_stats, XH_VEXT_COUNT
// for ext_stats): lane l adds partials l, l + 64, ... in order, then the
// shuffle tree (wave_column_sums) -- the same bits for the same inputs.
template <int S>
__global__ __launch_bounds__(64) void venv_loss_reduce_kernel(
    const double *part, int nparts, int accumulate, double *stats) {
#pragma clang fp contract(off)
  double v[S];
  wave_column_sums<S>(part, nparts, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < S; ++k) stats[k] = accumulate ? stats[k] + v[k] : v[k];
}

// ------------------------------------------------------------- launchers --
#define XH_VLOSS_BINS(X) X(8) X(16) X(32) X(64) X(128)

int venv_loss_grid(int B, long count) {
  const int bpl = 16 < B ? 16 : B;
  const long tile = 4l * (64 / (B / bpl));  // rows per workgroup and pass
  const long tiles = (count + tile - 1) / tile;
  return (int)(tiles < 1 ? 1 : (tiles > kVenvLossMaxBlocks ? kVenvLossMaxBlocks
                                                           : tiles));
}

// the STATS instantiation where the call asks for stats (a.part), the MASK
// one where it brings legal words (a.legal), the EXT one where the extension
// is on (a.ext)
template <int B, int KL, bool MASK, bool EXT>
static void vloss_launch_x(const VenvLossArgs &a, dim3 grid, hipStream_t s) {
  if (a.part)
    hipLaunchKernelGGL((venv_policy_loss_kernel<B, true, KL, MASK, EXT>), grid,
                       dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((venv_policy_loss_kernel<B, false, KL, MASK, EXT>),
                       grid, dim3(256), 0, s, a);
}
template <int B, int KL, bool MASK>
static void vloss_launch_m(const VenvLossArgs &a, dim3 grid, hipStream_t s) {
  if (a.ext)
    vloss_launch_x<B, KL, MASK, true>(a, grid, s);
  else
    vloss_launch_x<B, KL, MASK, false>(a, grid, s);
}
template <int B, int KL>
static void vloss_launch(const VenvLossArgs &a, dim3 grid, hipStream_t s) {
  if (a.legal)
    vloss_launch_m<B, KL, true>(a, grid, s);
  else
    vloss_launch_m<B, KL, false>(a, grid, s);
}

hipError_t launch_venv_policy_loss(VenvLossArgs a, hipStream_t s) {
  if (a.count <= 0) return hipSuccess;
  if (a.total <= 0) return hipErrorInvalidValue;  // a bad index reads row 0's
  // the distribution is gathered for the KL-regulated loss and for kl_stats
  const int kl = a.kl_part ? 2 : a.loss == kLossKlRegulated ? 1 : 0;
  if (kl && !a.distrib) return hipErrorInvalidValue;
  if (!a.ext && (a.ent_coef_dev || a.ent_coef != 0.0f || a.v_old || a.ext_part))
    return hipErrorInvalidValue;  // the plain instantiation reads none of them
  if (a.v_old && !a.values_new) return hipErrorInvalidValue;
#define X(XB)                                                                \
  if (a.B == XB) {                                                           \
    const long tile = 4l * VLossShape<XB>::RPW;                              \
    a.tiles = (a.count + tile - 1) / tile;                                   \
    const dim3 grid((unsigned)venv_loss_grid(XB, a.count));                  \
    if (kl == 2)                                                             \
      vloss_launch<XB, 2>(a, grid, s);                                       \
    else if (kl == 1)                                                        \
      vloss_launch<XB, 1>(a, grid, s);                                       \
    else                                                                     \
      vloss_launch<XB, 0>(a, grid, s);                                       \
    return hipGetLastError();                                                \
  }
  XH_VLOSS_BINS(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t launch_venv_loss_reduce(const double *part, int nparts,
                                   int accumulate, double *stats,
                                   hipStream_t s) {
  hipLaunchKernelGGL(venv_loss_reduce_kernel<XH_VLOSS_COUNT>, dim3(1), dim3(64),
                     0, s, part, nparts, accumulate, stats);
  return hipGetLastError();
}

hipError_t launch_venv_kl_reduce(const double *part, int nparts, int accumulate,
                                 double *kl_stats, hipStream_t s) {
  hipLaunchKernelGGL(venv_loss_reduce_kernel<XH_VKL_COUNT>, dim3(1), dim3(64),
                     0, s, part, nparts, accumulate, kl_stats);
  return hipGetLastError();
}

hipError_t launch_venv_ext_reduce(const double *part, int nparts,
                                  int accumulate, double *ext_stats,
                                  hipStream_t s) {
  hipLaunchKernelGGL(venv_loss_reduce_kernel<XH_VEXT_COUNT>, dim3(1), dim3(64),
                     0, s, part, nparts, accumulate, ext_stats);
  return hipGetLastError();
}

}  // namespace xh
