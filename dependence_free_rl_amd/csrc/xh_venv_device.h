// xh_venv_device.h -- what the venv's per-env-step kernels share: the step
// layout (VStepShape), the instance helpers (venv_cap / venv_capf /
// venv_draw), the XCD-aware block order, the episode count, the legal-set
// helpers and the first-maximum pick (the sampled pick: xh_venv_sample.inc).
// Included by venv_kernels.hip (venv_step_kernel, venv_act_kernel,
// venv_legal_kernel) and venv_heur_kernels.hip (venv_heur_kernel); the text
// was venv_kernels.hip's and moved here unchanged, so both compile one
// statement of each.
#pragma once
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_seg.h"

namespace xh {

// The step kernel's layout: XH_VENV_BPL (16) consecutive bins per lane
// (their bytes as aligned 32-bit words: 32 bytes at D = 2), so 64 / (B / 16)
// envs share a wave (16 at 64 bins).  With one lane per (env, bin) the step
// was issue-bound, not HBM-bound: every lane of an env draws the env's item
// (two engine draws and a double-precision canonical, register-only) and
// steps its stream with 64-bit modular multiplies, so the instruction count
// per byte falls with the bins a lane carries.  Round 6, 64 bins, 2-D, 1M
// envs: one env per wave 1.27 TB/s with the traffic at its algorithmic bytes
// (counters: 25% issuing, 40% issue stalls, 35% waiting on memory); 4 / 8 /
// 16 / 32 / 64 bins per lane 2.7 / 3.9 / 4.8 / 5.3 / 4.8 TB/s; at 32768 envs
// (launch-bound) 16 is the fastest (tools/env_ab.sh, profiles/r06j-k_*).
#ifndef XH_VENV_BPL
#define XH_VENV_BPL 16
#endif
template <int B, int D>
struct VStepShape {
  // bins per lane (contiguous; at most B)
  static constexpr int BPL = XH_VENV_BPL < B ? XH_VENV_BPL : B;
  static constexpr int NW = BPL * D / 4;   // 32-bit words per lane
  // the lane's words' alignment (the env row starts at env * B * D)
  static constexpr int LOWBIT = (4 * NW) & -(4 * NW);
  static constexpr int ALIGN = LOWBIT > 16 ? 16 : LOWBIT;
  static constexpr int LPE = B / BPL;      // lanes per env
  static constexpr int EPW = 64 / LPE;     // envs per wave
  static constexpr int BD = B * D;
};

// draw one item (get_item: bernoulli(0.4) over generate_canonical<double>)
__device__ __forceinline__ void venv_item(const EnvDesc &E, uint32_t &x,
                                          int8_t *ip) {
  const bool first = canonical(x) < E.p_a;
#pragma unroll
  for (int d = 0; d < 4; ++d)
    ip[d] = d < E.D ? (int8_t)(first ? E.item_a[d] : E.item_b[d]) : 0;
}

// The problem instance a kernel runs on: its trailing arguments, the pack IT.
// Empty: the reference's -- make_env's two items drawn by venv_item, kCapacity
// in every dim, all of it compile-time; these instantiations have the
// arguments and the code they had before the general ones existed.  One
// VenvItemTable (xh_kernels.h; xh_item_set): K <= 16 shapes and per-dim
// capacities as the kernel's second argument -- it arrives in scalar
// registers, the same for every lane.  The helpers below are overloaded on it.
__device__ __forceinline__ int venv_cap(int) { return kCapacity; }
__device__ __forceinline__ int venv_cap(int d, const VenvItemTable &t) {
  return t.cap[d];
}
// the observation's divisor; entries are float(x) / float(cap), an IEEE f32
// division in the general form (at a capacity that is no power of two a
// reciprocal multiply gives other bits)
template <class... IT>
__device__ __forceinline__ float venv_capf(int d, const IT &...t) {
  return (float)venv_cap(d, t...);
}

// get_item.  General: the K-way form of venv_item's u < p_a on the same
// canonical(x) (two engine draws): the first k with u < thr[k].  thr is
// non-decreasing and 1.0 from its last used entry on, so walking all 16
// entries and taking shape[k + 1] while u >= thr[k] ends on that k: 15 double
// compares and selects on scalar operands, no loads, no branch, whatever K is.
__device__ __forceinline__ void venv_draw(const EnvDesc &E, uint32_t &x,
                                          int8_t *ip) {
  venv_item(E, x, ip);
}
__device__ __forceinline__ void venv_draw(const EnvDesc &, uint32_t &x,
                                          int8_t *ip, const VenvItemTable &t) {
  const double u = canonical(x);
  uint32_t w = t.shape[0];
#pragma unroll
  for (int k = 0; k + 1 < kVenvItemsMax; ++k)
    w = u < t.thr[k] ? w : t.shape[k + 1];
#pragma unroll
  for (int d = 0; d < 4; ++d) ip[d] = (int8_t)((w >> (8 * d)) & 0xff);
}

// XCD-aware block order: workgroups are dispatched round-robin over the 8
// XCDs (XCD = block index mod 8), each with its own L2; block b takes the
// env range of block (b mod 8) G / 8 + b / 8, so an XCD steps one contiguous
// run of envs and the 4-byte per-env records sharing a 128-byte line
// (action, item, stream state, reward) are fetched by one L2, not eight
__device__ __forceinline__ int xcd_block() {
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  return (G & 7) == 0 ? (b & 7) * (G >> 3) + (b >> 3) : b;
}

// Episode statistics (a.ep_running, xh_venv_set_episode_stats; null while
// off): EP, an instantiation of its own as MASK is -- measured as a nullable
// pointer tested in the one kernel, the act launch without statistics was 1 to
// 2% slower than the parent's at 1M envs; the other
// instantiation holds none of this.  The env's running length is loaded with
// the kernel's other loads and stored with the record by the env's bin-0
// lane, the record's only writer: 8 bytes per env and step, no atomics.
// venv_ep_count is that lane's store for a live step: len = the length with
// this step; where the step ended the episode, len goes into the env's window
// accumulators (and into first_len if it is the env's first) and the count
// restarts.  The accumulators are touched by such steps alone.
__device__ __forceinline__ void venv_ep_count(const VenvArgs &a, int env,
                                              int run, bool over) {
  const int len = run + 1;
  a.ep_running[env] = over ? 0 : len;
  if (!over) return;
  // both loads before either store (which might alias them for all the
  // compiler knows): one round trip at the kernel's tail, not two
  VenvEpAcc *ac = a.ep_acc + env;
  VenvEpAcc v = *ac;
  const int fl = a.ep_first[env];
  v.count += 1;
  v.len_min = len < v.len_min ? len : v.len_min;
  v.len_max = len > v.len_max ? len : v.len_max;
  v.len_sum += (int64_t)len;
  v.len_sqsum += (uint64_t)len * (uint64_t)len;
  *ac = v;
  if (fl < 0) a.ep_first[env] = len;
}

// ---------------------------------------------------------- legal sets --
// Invalid-action masking (xh_venv_set_action_mask, xh_venv_legal).  Bin b
// takes the item iff bins[b][d] >= item[d] for every d < D (environment::
// apply's bin stays non-negative; any other pick is game over).  legal(e) is
// that set, eff(e) = legal(e) if it is not empty, else all B bins: when
// nothing fits every pick ends the episode and the row is used as given.
//
// venv_legal_bits: the lane's bins (VStepShape: BPL consecutive ones, their
// int8 words wv[] already in registers) against the item word, bit k = the
// lane's k-th bin -- D signed byte compares per bin, no loads.
// venv_eff_bits: one segment ballot tells whether the env has a legal bin.
// venv_legal_words: the env's W = max(1, B / 32) words, bit b % 32 of word b /
// 32 = bin b.  A lane's 16 bits are one half-word: an xor-1 shuffle pairs them
// on the even lanes, W shuffles bring the pairs to every lane of the env.
// venv_store_words: one plain vector store by one lane of the env, 16 bytes at
// 128 bins (row e of an [..][W] array off a 256-byte aligned base is aligned
// to its 4 W bytes).
template <int B>
struct VLegal {
  static constexpr int W = B >= 32 ? B / 32 : 1;
};

template <int B, int D>
__device__ __forceinline__ uint32_t venv_legal_bits(
    const uint32_t (&wv)[VStepShape<B, D>::NW], unsigned itw) {
  using S = VStepShape<B, D>;
  // The words through an empty asm: the act kernel unpacks the same bytes
  // again after its pick, and merged with these extractions the BPL D
  // unpacked ints would stay live across the softmax and the pick (+16 D
  // registers, a wave per SIMD less at 64 and 128 bins); the extraction is
  // cheaper than the registers.
  uint32_t ww[S::NW];
#pragma unroll
  for (int q = 0; q < S::NW; ++q) {
    ww[q] = wv[q];
    asm("" : "+v"(ww[q]));
  }
  uint32_t lb = 0u;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    bool fits = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = k * D + d;
      const int bv = (int)(signed char)((ww[j >> 2] >> (8 * (j & 3))) & 0xff);
      const int iv = (int)(signed char)((itw >> (8 * d)) & 0xff);
      fits &= bv >= iv;
    }
    lb |= (uint32_t)fits << k;
  }
  return lb;
}

template <int B, int D>
__device__ __forceinline__ uint32_t venv_eff_bits(uint32_t lb,
                                                  unsigned long long segmask) {
  using S = VStepShape<B, D>;
  const bool any = (__ballot(lb != 0u) & segmask) != 0;
  return any ? lb : (1u << S::BPL) - 1u;
}

template <int B, int D>
__device__ __forceinline__ void venv_legal_words(uint32_t eb, int seg0,
                                                 uint32_t (&wd)[VLegal<B>::W]) {
  using S = VStepShape<B, D>;
  if constexpr (S::LPE == 1) {
    wd[0] = eb;
  } else {
    const uint32_t pair = eb | ((uint32_t)__shfl_xor((int)eb, 1, kWave) << 16);
#pragma unroll
    for (int w = 0; w < VLegal<B>::W; ++w)
      wd[w] = (uint32_t)__shfl((int)pair, seg0 + 2 * w, kWave);
  }
}

template <int W>
__device__ __forceinline__ void venv_store_words(uint32_t *dst,
                                                 const uint32_t (&wd)[W]) {
  if constexpr (W == 4)
    *reinterpret_cast<uint4 *>(__builtin_assume_aligned(dst, 16)) =
        make_uint4(wd[0], wd[1], wd[2], wd[3]);
  else if constexpr (W == 2)
    *reinterpret_cast<uint2 *>(__builtin_assume_aligned(dst, 8)) =
        make_uint2(wd[0], wd[1]);
  else
    *dst = wd[0];
}

// --------------------------------------------------------------- picks --
// The two picks of a row held VStepShape's way (a lane's BPL consecutive
// entries in registers, the env's LPE lanes side by side in the wave); every
// lane of the wave calls them (the cross-lane steps need the whole wave).
//
// venv_pick_argmax: the first maximum of the values as given (tensor.cc:
// 464-466): the lane's own first maximum, then the env's lanes by an xor
// butterfly in which the lower index wins on equality.
template <int B, int D>
__device__ __forceinline__ int venv_pick_argmax(
    const float (&z)[VStepShape<B, D>::BPL], int li) {
  using S = VStepShape<B, D>;
  float best = z[0];
  int bi = li * S::BPL;
#pragma unroll
  for (int k = 1; k < S::BPL; ++k)
    if (z[k] > best) {
      best = z[k];
      bi = li * S::BPL + k;
    }
#pragma unroll
  for (int o = 1; o < S::LPE; o <<= 1) {
    const float ov = __shfl_xor(best, o, kWave);
    const int oi = __shfl_xor(bi, o, kWave);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  return bi;
}

// The sampled pick (std::discrete_distribution on u = canonical(x)) is the
// statement fragment xh_venv_sample.inc, included by both kernels' bodies.

// every venv shape: X(bins, dims)
#define XH_VENV_SHAPES(X) \
  X(8, 1) X(8, 2) X(8, 3) X(16, 1) X(16, 2) X(16, 3) X(32, 1) X(32, 2)      \
  X(32, 3) X(64, 1) X(64, 2) X(64, 3) X(128, 1) X(128, 2) X(128, 3)

// the step layout's grid (VStepShape: XH_VENV_BPL = 16 bins per lane, at most
// B): four waves per workgroup
static inline dim3 venv_step_grid(int N, int B) {
  const int epw = 64 / (B / (XH_VENV_BPL < B ? XH_VENV_BPL : B));
  const long waves = (N + epw - 1) / epw;
  return dim3((unsigned)((waves + 3) / 4));
}

}  // namespace xh
