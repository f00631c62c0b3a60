// rollout_pack_kernels.hip -- the 64-bin 2-D table rollout with several envs
// per wave (DESIGN.md §3.0g, §8 "The packed table rollout").
//
// rollout_split_kernel<S, false, true> reads a step's logit from the launch's
// logit table but keeps the forward's layout, one env per wave and lane = bin:
// the two canonical() draws, the sampler's reductions and scans, the env step
// and the record stores are issued for one env per wave-instruction.  Here a
// wave steps G = 64 / L envs (rollout_pack_layout.h): lane l holds env
// e0 + l / L and 64 / L consecutive bins of it in registers, so the per-env
// work is issued once for G envs, the first levels of every reduction run
// inside the lane and the rest inside an aligned segment of L <= 16 lanes of
// one DPP row (no LDS round trips).  The prologue (stage_split_rollout,
// build_logit_table) is the parent kernel's, by header.
//
// Every quantity keeps the parent's bits: the logit is the same table entry,
// the softmax sum is the same pairwise tree over the bin index
// (rollout_pack_layout.h), p = ex / sum, and the sample is libstdc++'s
// sequential discrete_distribution result -- partial sums in double whose
// order differs from the sequential one by rounding only, and the sequential
// restatement for every segment with a partial sum within 1e-9 of the draw,
// as sample_discrete (xh_device.h) does per wave.
#include "rollout_pack_layout.h"
#include "xh_roll_split.h"

namespace xh {
namespace {

// waves per workgroup (one workgroup per CU) and per SIMD; XH_PACK_WAVES: A/B
// builds (make variant VSRC=rollout_pack_kernels)
#ifndef XH_PACK_WAVES
#define XH_PACK_WAVES 12
#endif
constexpr int kPackWaves = XH_PACK_WAVES;
constexpr int kPackOcc = kPackWaves / 4;

// The value of the lane a DPP pattern pairs this one with (all lanes active;
// a source outside the row reads as 0: bound_ctrl).
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const int lo = dpp_i<CTRL>(__double2loint(v)), hi = dpp_i<CTRL>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
// Reductions over aligned segments of L <= 16 lanes: seg_sum's DPP patterns
// (xor 1, xor 2, then the mirror patterns, whose partner holds the same partial
// result as the xor partner).
template <int L>
__device__ __forceinline__ int seg_sum_i(int v) {
  v += dpp_i<0xB1>(v);
  v += dpp_i<0x4E>(v);
  if constexpr (L >= 8) v += dpp_i<0x141>(v);
  if constexpr (L >= 16) v += dpp_i<0x140>(v);
  return v;
}
template <int L>
__device__ __forceinline__ float seg_min_f(float v) {
  v = fminf(v, __int_as_float(dpp_i<0xB1>(__float_as_int(v))));
  v = fminf(v, __int_as_float(dpp_i<0x4E>(__float_as_int(v))));
  if constexpr (L >= 8) v = fminf(v, __int_as_float(dpp_i<0x141>(__float_as_int(v))));
  if constexpr (L >= 16) v = fminf(v, __int_as_float(dpp_i<0x140>(__float_as_int(v))));
  return v;
}
template <int L>
__device__ __forceinline__ double seg_sum_dd(double v) {
  v += dpp_d<0xB1>(v);
  v += dpp_d<0x4E>(v);
  if constexpr (L >= 8) v += dpp_d<0x141>(v);
  if constexpr (L >= 16) v += dpp_d<0x140>(v);
  return v;
}
// Exclusive prefix sum over the segment's lanes (pos = lane % L): row_shr by
// 1, 2, 4, 8 stays inside the 16-lane row, and `pos >= o` keeps a segment from
// reading its neighbour.
template <int L>
__device__ __forceinline__ double seg_scan_excl(double v, int pos) {
  double u = dpp_d<0x111>(v);
  if (pos >= 1) v += u;
  u = dpp_d<0x112>(v);
  if (pos >= 2) v += u;
  if constexpr (L >= 8) {
    u = dpp_d<0x114>(v);
    if (pos >= 4) v += u;
  }
  if constexpr (L >= 16) {
    u = dpp_d<0x118>(v);
    if (pos >= 8) v += u;
  }
  u = dpp_d<0x111>(v);
  return pos >= 1 ? u : 0.0;
}

// Bins 2k, 2k + 1 of a lane as one word of the int8 record ([bin][dim]).
template <int W>
struct alignas(W >= 4 ? 16 : 4 * W) Words {
  uint32_t w[W];
};

// The stepping of slots a.t .. a.t + nsteps - 1 for the wave groups
// g0, g0 + gstep, .. below g_end (one wave each); tab: the logit table in LDS.
template <class S, int L>
__device__ __forceinline__ void pack_step_groups(const RolloutArgs &a, const float *tab,
                                                 float b3, int g0, int g_end, int gstep) {
  static_assert(S::B == rp::kBins && S::D == 2 && S::G == 1, "64 bins, 2-D");
  using P = rp::Pack<L>;
  constexpr int B = S::B, G = P::kG, BPL = P::kBpl, NW = BPL / 2;
  const int lane = threadIdx.x & 63;
  const int pos = P::pos_of(lane), seg0 = lane - pos, bin0 = P::bin0_of(lane);
  const unsigned long long segmask = ((1ull << L) - 1ull) << seg0;
  const int N = a.b.N;
  const int t_last = a.t + (a.nsteps > 1 ? a.nsteps : 1) - 1;
  for (int g = g0; g < g_end; g += gstep) {
    // a tail wave's idle segments run along on zeros and store nothing
    const bool act = P::active(g, lane, N);
    const int env = act ? g * G + P::env_of(lane) : 0;
    const bool head = act && pos == 0;
    int bv[BPL][2], iv[2] = {0, 0};
    uint32_t x = 1u;
    {
      const int slot = a.src_slot > 0 ? a.src_slot : a.t;
      Words<NW> wd;
      uint32_t iw = 0;
#pragma unroll
      for (int k = 0; k < NW; ++k) wd.w[k] = 0;
      if (act) {
        wd = *reinterpret_cast<const Words<NW> *>(a.b.bins + ((size_t)slot * N + env) * S::BD +
                                                  bin0 * 2);
        iw = *reinterpret_cast<const uint32_t *>(a.b.items + ((size_t)slot * N + env) * 4);
        x = a.b.rng[env];
        if (a.src_slot > 0) {  // slot 0 := slot src_slot
          *reinterpret_cast<Words<NW> *>(a.b.bins + (size_t)env * S::BD + bin0 * 2) = wd;
          // (the item's bytes from D on are 0 in every slot)
          if (pos == 0) *reinterpret_cast<uint32_t *>(a.b.items + (size_t)env * 4) = iw & 0xffffu;
        }
      }
#pragma unroll
      for (int r = 0; r < BPL; ++r)
#pragma unroll
        for (int d = 0; d < 2; ++d)
          bv[r][d] = (int)(int8_t)(wd.w[r >> 1] >> (16 * (r & 1) + 8 * d));
      iv[0] = (int)(int8_t)iw;
      iv[1] = (int)(int8_t)(iw >> 8);
    }
    bool ia = iv[0] == a.env.item_a[0] && iv[1] == a.env.item_a[1];
    for (int t = a.t; t <= t_last; ++t) {
      const bool last = t == t_last;
      // the logits: one table read per bin (index clamped as the parent's)
      float z[BPL], ex[BPL], p[BPL];
#pragma unroll
      for (int r = 0; r < BPL; ++r) {
        const int e = lt::entry(ia ? 0 : 1, bv[r][0], bv[r][1]);
        z[r] = tab[min((unsigned)e, (unsigned)lt::kEntries - 1u)] + b3;
        ex[r] = expf(z[r]);
      }
      const float sum = seg_sum<L>(rp::lane_tree<BPL>(ex));
#pragma unroll
      for (int r = 0; r < BPL; ++r) p[r] = ex[r] / sum;
      if (act) {
        if (last && a.logits_out)
#pragma unroll
          for (int r = 0; r < BPL; ++r) a.logits_out[(size_t)env * B + bin0 + r] = z[r];
        if (last && a.probs_out)
#pragma unroll
          for (int r = 0; r < BPL; ++r) a.probs_out[(size_t)env * B + bin0 + r] = p[r];
        if (a.qold_out)
#pragma unroll
          for (int r = 0; r < BPL; ++r)
            a.qold_out[((size_t)t * N + env) * B + bin0 + r] = p[r];
      }

      // the sampler's draw (sample_discrete, xh_device.h), once per env
      const double u = canonical(x);
      int choice;
      if (a.forced) {
        choice = act ? a.forced[(size_t)t * N + env] : 0;
      } else {
        // partial sums of the unnormalised doubles, in the lane and then over
        // the segment's lanes, times 1 / their sum: within rounding of
        // libstdc++'s sequential sums of p / sum, which decide below
        double c[BPL];
#pragma unroll
        for (int r = 0; r < BPL; ++r) c[r] = r == 0 ? (double)p[0] : c[r - 1] + (double)p[r];
        const double sd = seg_sum_dd<L>(c[BPL - 1]);
        const double excl = seg_scan_excl<L>(c[BPL - 1], pos);
        const double rsd = 1.0 / sd;
        int cnt = 0;
        float gap = 1.0f;
#pragma unroll
        for (int r = 0; r < BPL; ++r) {
          double cp = (excl + c[r]) * rsd;
          if (r == BPL - 1 && pos == L - 1) cp = 1.0;
          cnt += cp < u ? 1 : 0;
          gap = fminf(gap, (float)fabs(cp - u));
        }
        choice = seg_sum_i<L>(cnt);
        const bool near = seg_min_f<L>(gap) < 1e-9f;
        if (__ballot(near) != 0ull) {
          // libstdc++'s order for the segments that ask: sum, p / sum, partial
          // sums, lower_bound(u) -- bin k is register k % BPL of lane k / BPL
          double s2 = 0.0;
#pragma unroll 1
          for (int j = 0; j < L; ++j)
#pragma unroll
            for (int r = 0; r < BPL; ++r) s2 += (double)__shfl(p[r], seg0 + j, kWave);
          double acc = 0.0;
          int c2 = B - 1;
#pragma unroll 1
          for (int j = 0; j < L; ++j)
#pragma unroll
            for (int r = 0; r < BPL; ++r) {
              const int k = j * BPL + r;
              const double qk = (double)__shfl(p[r], seg0 + j, kWave) / s2;
              acc = k == 0 ? qk : acc + qk;
              const double cpk = k == B - 1 ? 1.0 : acc;
              if (!(cpk < u) && k < c2) c2 = k;
            }
          if (near) choice = c2;
        }
      }
      const int cl = choice / BPL, cr = choice % BPL;  // the chosen bin's lane, register
      float ps = p[0];
#pragma unroll
      for (int r = 1; r < BPL; ++r) ps = cr == r ? p[r] : ps;
      const float pold = __shfl(ps, seg0 + cl, kWave);

      // apply: the chosen bin takes the item; game over if it does not fit
      const bool owner = cl == pos;
      bool neg = false;
#pragma unroll
      for (int r = 0; r < BPL; ++r)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const bool hit = owner && cr == r;
          bv[r][d] = hit ? bv[r][d] - iv[d] : bv[r][d];
          neg |= hit && bv[r][d] < 0;
        }
      const bool done = (__ballot(neg) & segmask) != 0ull;
      // apply -> get_item, or game over -> reset -> get_item: 2 draws either way
      const bool first = canonical(x) < a.env.p_a;
      Words<NW> wd;
#pragma unroll
      for (int k = 0; k < NW; ++k) wd.w[k] = 0;
#pragma unroll
      for (int r = 0; r < BPL; ++r)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          bv[r][d] = done ? kCapacity : bv[r][d];
          wd.w[r >> 1] |= ((uint32_t)bv[r][d] & 0xffu) << (16 * (r & 1) + 8 * d);
        }
      iv[0] = first ? a.env.item_a[0] : a.env.item_b[0];
      iv[1] = first ? a.env.item_a[1] : a.env.item_b[1];
      ia = first;
      if (act)
        *reinterpret_cast<Words<NW> *>(a.b.bins + ((size_t)(t + 1) * N + env) * S::BD + bin0 * 2) =
            wd;
      if (head) {
        *reinterpret_cast<uint32_t *>(a.b.items + ((size_t)(t + 1) * N + env) * 4) =
            ((uint32_t)iv[0] & 0xffu) | (((uint32_t)iv[1] & 0xffu) << 8);
        a.b.action[(size_t)t * N + env] = choice;
        a.b.pold[(size_t)t * N + env] = pold;
        a.b.done[(size_t)t * N + env] = (uint8_t)done;
      }
    }
    if (head) a.b.rng[env] = (t_last == a.b.T - 1) ? mstd_mulmod(x, a.jump_mul) : x;
  }
}

// Every workgroup stages the parameters and builds the table behind them
// (rollout_split_kernel<S, false, true>'s prologue), then steps a contiguous
// block of wave groups dealt round-robin to its waves.
template <class S, int L>
__global__ __launch_bounds__(64 * kPackWaves, kPackOcc) void rollout_pack_kernel(RolloutArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ldsf[];
  char *lds = reinterpret_cast<char *>(ldsf);
  stage_split_rollout<S>(a.params, a.env, lds);
  __syncthreads();
  const float b3 = reinterpret_cast<const float *>(lds + RollSplitLds<S>::F)[RollSplitLds<S>::B3];
  const float *tab = reinterpret_cast<const float *>(lds + RollSplitLds<S>::bytes);
  build_logit_table<S>(lds, reinterpret_cast<float *>(lds + RollSplitLds<S>::bytes));
  __syncthreads();
  const int ngroups = rp::Pack<L>::groups(a.b.N);
  const int per = (ngroups + (int)gridDim.x - 1) / (int)gridDim.x;
  const int g_end = min(ngroups, ((int)blockIdx.x + 1) * per);
  pack_step_groups<S, L>(a, tab, b3, (int)blockIdx.x * per + (int)(threadIdx.x >> 6), g_end,
                         (int)(blockDim.x >> 6));
}

template <class S, int L>
hipError_t launch_pack(const RolloutArgs &a, int cus, hipStream_t s) {
  constexpr int lds = (int)roll_split_lds<S, true>();
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void *)rollout_pack_kernel<S, L>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = true;
  }
  const int ng = rp::Pack<L>::groups(a.b.N);
  const int wg = (ng + kPackWaves - 1) / kPackWaves;
  hipLaunchKernelGGL((rollout_pack_kernel<S, L>), dim3(cus < wg ? cus : wg),
                     dim3(64 * kPackWaves), lds, s, a);
  return hipGetLastError();
}

}  // namespace

int rollout_pack_lanes(int want) {
  return want == kRollPackLanesAlt ? kRollPackLanesAlt : kRollPackLanes;
}

hipError_t launch_rollout_pack(const RolloutArgs &a, int lanes, int cus, hipStream_t s) {
  using S = PShape<64, 2, 128, 128>;
  if (a.env.B != 64 || a.env.D != 2 || a.e0_mask || a.wide || a.wide_seen)
    return hipErrorInvalidValue;
  if (lanes == kRollPackLanes) return launch_pack<S, kRollPackLanes>(a, cus, s);
  if (lanes == kRollPackLanesAlt) return launch_pack<S, kRollPackLanesAlt>(a, cus, s);
  return hipErrorInvalidValue;
}

}  // namespace xh
