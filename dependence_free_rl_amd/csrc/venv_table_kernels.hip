// venv_table_kernels.hip -- logit tables for VecEnv learners (xh_venv_table_*,
// include/xylo_hip.h; the domain and the quantiser: xh_venv_table.h).  A
// per-bin logit depends on (bins[b][0..D), item) alone, and in a venv that is
// one of E = K prod_d (capacity[d] + 1) points, so a learner evaluates its
// per-bin network on the E table rows once and then
//   venv_table_obs_kernel    writes the table's observations [R][B][2D];
//   venv_act_table_kernel    is xh_venv_act(XH_ACT_LOGITS) on the row z[b] =
//                            table[e(bins[b], item)], gathered in the launch
//                            from the int8 bins it holds anyway;
//   venv_table_gather_kernel writes the logits of recorded rows [count][B], the
//                            loss head's input;
//   venv_table_max / sum / finish  sum the loss head's dout per entry: G[e],
//                            the table's dL/dlogit, in exact integer arithmetic.
// Every kernel takes the item table as an argument (a venv without a set
// passes the default set: the general kernels draw and divide bit for bit as
// the builtin ones do there), and forms an entry only from values that passed
// the domain's checks, so out-of-domain input never reads outside the table.
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_seg.h"
#include "xh_venv_device.h"
#include "xh_venv_table.h"
#include "xh_vstore.h"

namespace xh {

// the lane's BPL bins (their int8 words wv[]) against the domain: e[k] = the
// entry of bin k under item index ki (0 where the bin is outside the domain),
// returns whether every one of them is inside.  ki < 0 (the item is none of
// the set's shapes): nothing is inside.
template <int B, int D>
__device__ __forceinline__ bool vtab_entries(
    const uint32_t (&wv)[VStepShape<B, D>::NW], int ki, const VenvTabDomain &m,
    int (&e)[VStepShape<B, D>::BPL]) {
  using S = VStepShape<B, D>;
  bool all = ki >= 0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    int b[D];
    bool ok = ki >= 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = k * D + d;
      b[d] = (int)(signed char)((wv[j >> 2] >> (8 * (j & 3))) & 0xff);
      ok &= vt::bin_ok(b[d], m.side[d]);
    }
    e[k] = ok ? vt::entry(ki, m.states, vt::state_index(m.side, D, b)) : 0;
    all &= ok;
  }
  return all;
}

// ------------------------------------------------------------------ obs --
// One per-bin row per thread: row e < E is entry e's observation, written
// with OBS's expressions; the rows from E on are zero.
__global__ __launch_bounds__(256) void venv_table_obs_kernel(
    VenvTabDomain m, VenvItemTable t, long total, float *obs) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  float *o = obs + e * 2 * m.D;
  if (e >= m.entries) {
    for (int d = 0; d < 2 * m.D; ++d) o[d] = 0.0f;
    return;
  }
  vt::Domain dm{};
  dm.D = m.D;
  dm.K = m.K;
  dm.states = m.states;
  for (int d = 0; d < 4; ++d) dm.side[d] = m.side[d];
  int k, b[4] = {0, 0, 0, 0};
  vt::entry_decode(dm, (int)e, &k, b);
  const uint32_t w = t.shape[k];
  for (int d = 0; d < m.D; ++d) {
    const int iv = (int)(signed char)((w >> (8 * d)) & 0xff);
    o[d] = (float)b[d] / (float)t.cap[d];
    o[m.D + d] = (float)iv / (float)t.cap[d];
  }
}

// ------------------------------------------------------------------ act --
// venv_act_kernel (venv_kernels.hip) with a.logits and the row formed here:
// the layout, the loads, the mask, the softmax, the pick, the record and
// agent::step are its statements.  An env with a bin outside [0, capacity[d]]
// or an item that is none of the set's shapes is refused as a bad policy row
// is (error bit 8), and its lanes read entry 0.
template <int B, int D, bool RD, bool MASK, bool EP>
__global__ __launch_bounds__(256) void venv_act_table_kernel(
    VenvTabActArgs h, VenvItemTable t) {
  using S = VStepShape<B, D>;
  static_assert(!RD || (S::BPL == VLossShape<B>::BPL && S::EPW ==
                                                          VLossShape<B>::RPW),
                "the distribution record is stored in vloss_store's layout");
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
  // the row: one gather per bin, the entry from checked values only
  float z[S::BPL];
  bool outside;
  {
    int e[S::BPL];
    const int ki = vt::item_index(t.shape, h.m.K, D, itw);
    outside = !vtab_entries<B, D>(wv, ki, h.m, e);
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) z[k] = h.table[e[k]];
  }
  const bool off_domain = (__ballot(outside) & segmask) != 0;

  [[maybe_unused]] uint32_t eb = 0u;  // the lane's bits of eff(e) (MASK)
  if constexpr (MASK) {
    eb = venv_eff_bits<B, D>(venv_legal_bits<B, D>(wv, itw), segmask);
#pragma unroll
    for (int k = 0; k < S::BPL; ++k) z[k] = (eb >> k) & 1u ? z[k] : -INFINITY;
  }

  // the row's probabilities
  float p[S::BPL];
  seg_softmax<S::LPE, S::BPL>(z, p);  // xh_seg.h
  bool bad = false;
  double lsum = 0.0;
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    bad |= !(p[k] >= 0.0f);  // NaN or negative
    lsum += (double)p[k];
  }
  const double sd = seg_sum_d<S::LPE>(lsum);
  bad |= !(sd > 0.0 && sd < (double)INFINITY);
  const bool refused = off_domain || (__ballot(bad) & segmask) != 0;

  // the pick (all lanes: the cross-lane steps need the whole wave)
  int choice;
  if (a.argmax) {  // first maximum of the values as given (tensor.cc:464-466)
    choice = venv_pick_argmax<B, D>(z, li);
    x = mstd_mulmod(x, a.v.skip_mul);  // the venv's policy draws, unused
  } else  // the sampled pick's statements, shared with venv_act_kernel
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
    vloss_store<B, false>(
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
      atomicOr(a.v.err, off_domain ? 8 : 2);
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
        nb[k][d] = reset ? venv_cap(d, t) : nb[k][d];
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
  if (!chosen_over) venv_draw(a.v.env, x, nit, t);  // apply's get_item
  if (reset) venv_draw(a.v.env, x, nit, t);         // reset's get_item
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
        o[d] = (float)nb[k][d] / venv_capf(d, t);
        o[D + d] = (float)nit[d] / venv_capf(d, t);
      }
    }
  }
}

// --------------------------------------------------- the record's rows --
// Output row j of a gather / a gradient sum: its index q = rows[first + j] or
// first + j, row q = t N + e of the record's STATE view (slot P: the present
// state), as venv_record_obs_kernel (venv_learn_kernels.hip) addresses it.
// The lane's words and the item word are loaded unconditionally (row 0's for
// a lane past the last row or an index outside the view: in range whenever
// count > 0).  Returns live: the row is in range, its index valid and every
// bin and the item inside the domain; a row that is in range and not live
// raises error bit 4 (the index) or 8 (the domain).
template <int B, int D>
__device__ __forceinline__ bool vtab_row(const VenvTabRowArgs &a,
                                         const VenvItemTable &t, long j,
                                         int lane,
                                         int (&e)[VStepShape<B, D>::BPL]) {
  using S = VStepShape<B, D>;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const int seg0 = el * S::LPE;
  const bool in_range = j < a.count;
  const long jc = in_range ? j : 0;
  const long total = (long)(a.P + 1) * a.N;
  const long qr = a.rows ? (long)a.rows[a.first + jc] : a.first + jc;
  const bool valid = qr >= 0 && qr < total;
  const long q = valid ? qr : 0;
  const bool present = q >= (long)a.P * a.N;
  const long so = present ? q - (long)a.P * a.N : q;
  const int8_t *bp = (present ? a.cur_bins : a.rec_bins) + (size_t)so * S::BD;
  const int8_t *ip = (present ? a.cur_items : a.rec_items) + (size_t)so * 4;
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int w = 0; w < S::NW; ++w) wv[w] = wp[w];
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);
  const int ki = vt::item_index(t.shape, a.m.K, D, itw);
  const bool outside = !vtab_entries<B, D>(wv, ki, a.m, e);
  const unsigned long long segmask =
      S::LPE == 64 ? ~0ull : ((1ull << S::LPE) - 1ull) << seg0;
  const bool off_domain = (__ballot(outside) & segmask) != 0;
  if (in_range && li == 0) {
    if (!valid)
      atomicOr(a.err, 4);
    else if (off_domain)
      atomicOr(a.err, 8);
  }
  return in_range && valid && !off_domain;
}

// out[j][b] = table[e(row j's bin b)]: a lane's 16 floats (8 at 8 bins) as
// 16-byte stores from the lane that gathered them; a row that is not live is
// left untouched.
template <int B, int D>
__global__ __launch_bounds__(256) void venv_table_gather_kernel(
    VenvTabRowArgs a, VenvItemTable t) {
  using S = VStepShape<B, D>;
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long j = wave * S::EPW + lane / S::LPE;
  int e[S::BPL];
  const bool live = vtab_row<B, D>(a, t, j, lane, e);
  float f[S::BPL];
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) f[k] = a.table[e[k]];
  vloss_store<B, true>(
      f, nullptr, lane, __ballot(live),
      reinterpret_cast<vl_f4 *>(__builtin_assume_aligned(a.out, 16)) +
          (size_t)(wave * S::EPW) * (B / 4));
}

// ------------------------------------------------------- the entry sum --
// m = max |dout| over the count B floats, as an integer max over the bit
// patterns with the sign cleared (NaN and inf compare above every finite
// value): the lanes' maxima, the wave's by shuffles, one atomicMax per wave.
__global__ __launch_bounds__(256) void venv_table_max_kernel(const float *dout,
                                                             long n,
                                                             uint32_t *maxbits) {
  uint32_t m = 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const uint32_t b = __float_as_uint(dout[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t ov = (uint32_t)__shfl_xor((int)m, o, kWave);
    m = ov > m ? ov : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(maxbits, m);
}

// acc[e] += sum of q(dout[j][b]) over the live rows' (j, b) with entry e, as
// 64-bit integers.  LDS: the workgroup's sums first (ds_add_u64), then one
// global add per entry it touched; otherwise (a domain past kVtabLdsEntries)
// global adds.  Integer addition is associative: any grid, any order, the
// same bits.  Rows in a grid-stride loop (wave-uniform trip counts; the only
// barriers stand outside it).
constexpr int kVtabLdsEntries = 4096;

template <int B, int D, bool LDS>
__global__ __launch_bounds__(256) void venv_table_sum_kernel(VenvTabRowArgs a,
                                                             VenvItemTable t) {
  using S = VStepShape<B, D>;
  const uint32_t mb = *a.maxbits;
  if (mb == 0u || !vt::quant_finite(mb)) return;  // G = 0 / refused (finish)
  const int sh = vt::quant_shift(a.count * B, mb);
  __shared__ unsigned long long part[LDS ? kVtabLdsEntries : 1];
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < (int)a.m.entries; i += blockDim.x)
      part[i] = 0ull;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long nwaves = (a.count + S::EPW - 1) / S::EPW;
  const long stride = (long)gridDim.x * (blockDim.x >> 6);
  for (long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
       wave < nwaves; wave += stride) {
    const long j = wave * S::EPW + lane / S::LPE;
    int e[S::BPL];
    const bool live = vtab_row<B, D>(a, t, j, lane, e);
    const long jc = j < a.count ? j : 0;
    const vl_f4 *dp = reinterpret_cast<const vl_f4 *>(__builtin_assume_aligned(
        a.dout + (size_t)jc * B + (lane % S::LPE) * S::BPL, 16));
    float g[S::BPL];
#pragma unroll
    for (int q = 0; q < S::BPL / 4; ++q) {
      const vl_f4 x = dp[q];
      g[4 * q] = x.x;
      g[4 * q + 1] = x.y;
      g[4 * q + 2] = x.z;
      g[4 * q + 3] = x.w;
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < S::BPL; ++k) {
        const long long q = vt::quantise(g[k], sh);
        if (q == 0) continue;
        if constexpr (LDS)
          atomicAdd(&part[e[k]], (unsigned long long)q);
        else
          atomicAdd(&a.acc[e[k]], (unsigned long long)q);
      }
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)a.m.entries; i += blockDim.x) {
      const unsigned long long v = part[i];
      if (v) atomicAdd(&a.acc[i], v);
    }
  }
}

// g[e] = (accumulate ? g[e] : 0) + G[e] over the R B floats, G = 0 from E on;
// a non-finite dout leaves g untouched and raises error bit 8.
__global__ __launch_bounds__(256) void venv_table_finish_kernel(
    const unsigned long long *acc, const uint32_t *maxbits, long n,
    long entries, long total, int accumulate, float *g, int *err) {
  const uint32_t mb = *maxbits;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (!vt::quant_finite(mb)) {
    if (e == 0) atomicOr(err, 8);
    return;
  }
  if (e >= total) return;
  float G = 0.0f;
  if (mb != 0u && e < entries)
    G = vt::dequantise((long long)acc[e], vt::quant_shift(n, mb));
  g[e] = accumulate ? g[e] + G : G;
}

// ------------------------------------------------------------- launchers --
hipError_t launch_venv_table_obs(const VenvTabDomain &m,
                                 const VenvItemTable &t, long total,
                                 float *obs, hipStream_t s) {
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(venv_table_obs_kernel, dim3((unsigned)((total + 255) / 256)),
                     dim3(256), 0, s, m, t, total, obs);
  return hipGetLastError();
}

// RD where the call records its distributions, MASK where it masks, EP where
// it counts episodes
template <int B, int D, bool RD, bool MASK>
static void vtab_act_launch_ep(const VenvTabActArgs &h, hipStream_t s,
                               const VenvItemTable &t) {
  const dim3 grid = venv_step_grid(h.a.v.N, B);
  if (h.a.v.ep_running)
    hipLaunchKernelGGL((venv_act_table_kernel<B, D, RD, MASK, true>), grid,
                       dim3(256), 0, s, h, t);
  else
    hipLaunchKernelGGL((venv_act_table_kernel<B, D, RD, MASK, false>), grid,
                       dim3(256), 0, s, h, t);
}

template <int B, int D>
static void vtab_act_launch(const VenvTabActArgs &h, hipStream_t s,
                            const VenvItemTable &t) {
  if (h.a.legal) {
    if (h.a.rec_distrib)
      vtab_act_launch_ep<B, D, true, true>(h, s, t);
    else
      vtab_act_launch_ep<B, D, false, true>(h, s, t);
  } else {
    if (h.a.rec_distrib)
      vtab_act_launch_ep<B, D, true, false>(h, s, t);
    else
      vtab_act_launch_ep<B, D, false, false>(h, s, t);
  }
}

hipError_t launch_venv_act_table(const VenvTabActArgs &h, hipStream_t s,
                                 const VenvItemTable &t) {
  const int B = h.a.v.env.B, D = h.a.v.env.D;
  if (h.a.v.N <= 0) return hipSuccess;
  if (h.m.entries < 1 || h.m.entries > XH_VTAB_MAX_ENTRIES)
    return hipErrorInvalidValue;
#define X(XB, XD)                                                            \
  if (B == XB && D == XD) {                                                  \
    vtab_act_launch<XB, XD>(h, s, t);                                        \
    return hipGetLastError();                                                \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

static bool vtab_rows_ok(const VenvTabRowArgs &a) {
  return a.N > 0 && a.P >= 0 && a.m.entries >= 1 &&
         a.m.entries <= XH_VTAB_MAX_ENTRIES;
}

hipError_t launch_venv_table_gather(const VenvTabRowArgs &a, hipStream_t s,
                                    const VenvItemTable &t) {
  if (a.count <= 0) return hipSuccess;
  if (!vtab_rows_ok(a)) return hipErrorInvalidValue;
#define X(XB, XD)                                                             \
  if (a.B == XB && a.D == XD) {                                               \
    const long waves = (a.count + VStepShape<XB, XD>::EPW - 1) /              \
                       VStepShape<XB, XD>::EPW;                               \
    const long blocks = (waves + 3) / 4;                                      \
    if (blocks > 0x7fffffffl) return hipErrorInvalidValue;                    \
    hipLaunchKernelGGL((venv_table_gather_kernel<XB, XD>),                    \
                       dim3((unsigned)blocks), dim3(256), 0, s, a, t);        \
    return hipGetLastError();                                                 \
  }
  XH_VENV_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

// the sum's grid: a workgroup per four waves of rows, at most kVtabSumBlocks
// (each workgroup clears and flushes its E partial sums once)
constexpr long kVtabSumBlocks = 1024;

hipError_t launch_venv_table_grad(const VenvTabRowArgs &a, long total,
                                  int accumulate, float *g, hipStream_t s,
                                  const VenvItemTable &t) {
  if (a.count <= 0 || total <= 0) return hipErrorInvalidValue;
  if (!vtab_rows_ok(a) || total < a.m.entries) return hipErrorInvalidValue;
  const long n = a.count * a.B;
  {
    const long blocks = (n + 1023) / 1024;  // four floats per thread or more
    hipLaunchKernelGGL(venv_table_max_kernel,
                       dim3((unsigned)(blocks > 1024 ? 1024 : blocks)),
                       dim3(256), 0, s, a.dout, n, a.maxbits);
  }
  bool launched = false;
#define X(XB, XD)                                                             \
  if (a.B == XB && a.D == XD) {                                               \
    const long waves = (a.count + VStepShape<XB, XD>::EPW - 1) /              \
                       VStepShape<XB, XD>::EPW;                               \
    long blocks = (waves + 3) / 4;                                            \
    blocks = blocks > kVtabSumBlocks ? kVtabSumBlocks : blocks;               \
    if (a.m.entries <= kVtabLdsEntries)                                       \
      hipLaunchKernelGGL((venv_table_sum_kernel<XB, XD, true>),               \
                         dim3((unsigned)blocks), dim3(256), 0, s, a, t);      \
    else                                                                      \
      hipLaunchKernelGGL((venv_table_sum_kernel<XB, XD, false>),              \
                         dim3((unsigned)blocks), dim3(256), 0, s, a, t);      \
    launched = true;                                                          \
  }
  XH_VENV_SHAPES(X)
#undef X
  if (!launched) return hipErrorInvalidValue;
  hipLaunchKernelGGL(venv_table_finish_kernel,
                     dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     a.acc, a.maxbits, n, a.m.entries, total, accumulate, g,
                     a.err);
  return hipGetLastError();
}

}  // namespace xh
