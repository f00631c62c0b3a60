// venv_learn_kernels.hip -- from a window xh_venv_act recorded to the
// learner's inputs, without leaving HBM (xh_venv_record_obs,
// xh_venv_advantages; include/xylo_hip.h):
//   venv_record_obs_kernel  observation::to_vector (bin_packing.h:31-40) of
//                           recorded rows: a run of rows or a shuffled
//                           minibatch, the state S_t or the successor row of
//                           replay_buffer::sample_td (S_t+1, or the terminal
//                           view E_t of a transition that ended);
//   venv_gae_kernel         calculate_advantage (policy_gradient.h:220-281) and
//                           the TD(0) targets (:205-215) with the reward read
//                           instead of implied: gae_kernel's and
//                           value_targets_kernel's arithmetic
//                           (value_kernels.hip), plus the lambda return.
// Both are HBM-bound.  Bytes per row of the observations: B D + 4 read (the
// int8 state), 8 B D written (+ 4 with an index list, + 9 for NEXT: done,
// action and the next slot's item).  Bytes per env of the scan: 4 (T + 1) + T
// + 4 T read (+ 4 T with v_term), 4 T written per output.
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_sums.h"

namespace xh {

// venv_kernels.hip's VStepShape: a lane owns 16 consecutive bins of one row
// (all of them at 8 bins) -- their int8 bytes as aligned 32-bit words in, their
// 16 * 2D floats as 16-byte stores out -- so B / 16 lanes share a row and a
// wave covers 64 / (B / 16) rows.
// The stores: a lane's 16 * 2D floats are one contiguous run, but stored from
// the lane that made them every instruction would touch 64 different lines
// with 16 bytes each.  The wave's output (its rows are consecutive) is one
// contiguous block, so the runs are exchanged through LDS, 8 16-byte pieces
// per lane and pass (all of them below 8), and lane l of instruction i stores
// piece 64 i + l of the pass: whole 128-byte lines per 8 lanes, as
// nontemporal stores (the block is written once and read by another kernel).
// Measured at 1M rows of 64 bins, 2-D: 0.366 ms from the
// owning lanes, 0.227 ms exchanged, 0.214 ms exchanged and nontemporal;
// nontemporal stores from the owning lanes 3.4 ms.
typedef float f4v __attribute__((ext_vector_type(4)));

template <int B, int D>
struct VObsShape {
  static constexpr int BPL = 16 < B ? 16 : B;  // bins per lane
  static constexpr int NW = BPL * D / 4;       // 32-bit words per lane
  static constexpr int LOWBIT = (4 * NW) & -(4 * NW);
  static constexpr int ALIGN = LOWBIT > 16 ? 16 : LOWBIT;
  static constexpr int LPE = B / BPL;          // lanes per row
  static constexpr int RPW = 64 / LPE;         // rows per wave
  static constexpr int BD = B * D;
  static constexpr int NF = BPL * 2 * D;       // floats per lane
};

// Per output row j (all in registers, the same instructions for every lane):
// its index q (the list's entry or first + j), slot t = q / N and env e; the
// source slot s -- t for STATE; for NEXT t + 1, or t itself where the row
// ended -- read from the record when s < P and from the present state when s
// = P; for an ended NEXT row the chosen bin is reduced by the item.  Lanes
// past the last row, and rows whose index is outside the view, load row 0's
// words (in range whenever count > 0 rows exist) and nothing is stored for
// them.
//
// CAP, the kernel's trailing arguments: nothing -- capacity kCapacity, the
// arguments and the code of before general item sets -- or one VObsCaps, a
// set's per-dim capacities: IEEE f32 divisions by float(cap[d]).
struct VObsCaps {
  int32_t cap[4];
};
__device__ __forceinline__ float vobs_capf(int) { return (float)kCapacity; }
__device__ __forceinline__ float vobs_capf(int d, const VObsCaps &c) {
  return (float)c.cap[d];
}

template <int B, int D, class... CAP>
__global__ __launch_bounds__(256) void venv_record_obs_kernel(VenvObsArgs a,
                                                              CAP... c) {
  using S = VObsShape<B, D>;
  static_assert(S::NF % 4 == 0, "the lane's floats as 16-byte stores");
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int el = lane / S::LPE, li = lane % S::LPE;
  const long j = wave * S::RPW + el;
  const bool in_range = j < a.count;
  const long jc = in_range ? j : 0;
  const long total = (long)(a.next ? a.P : a.P + 1) * a.N;
  const long qr = a.rows ? (long)a.rows[a.first + jc] : a.first + jc;
  const bool valid = qr >= 0 && qr < total;
  const long q = valid ? qr : 0;
  // NEXT: the row's done byte and action (slot 0's where the view is empty:
  // the record has at least one slot, the launcher sees to it)
  int done = 0, act = 0;
  if (a.next) {
    done = a.rec_done[q] != 0;
    act = a.rec_action[q];
  }
  const long sq = a.next && !done ? q + a.N : q;  // source row s N + e
  const bool present = sq >= (long)a.P * a.N;
  const long so = present ? sq - (long)a.P * a.N : sq;
  const int8_t *bp = (present ? a.cur_bins : a.rec_bins) + (size_t)so * S::BD;
  const int8_t *ip = (present ? a.cur_items : a.rec_items) + (size_t)so * 4;
  const uint32_t *wp = reinterpret_cast<const uint32_t *>(
      __builtin_assume_aligned(bp + li * S::BPL * D, S::ALIGN));
  uint32_t wv[S::NW];
#pragma unroll
  for (int w = 0; w < S::NW; ++w) wv[w] = wp[w];
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);

  if (in_range && !valid && li == 0) atomicOr(a.err, 4);
  const bool live = in_range && valid;
  int item[D];
#pragma unroll
  for (int d = 0; d < D; ++d) item[d] = (int)(signed char)((itw >> (8 * d)) & 0xff);
  const int sub = done ? act : -1;  // E_t: bins[action] -= item
  float f[S::NF];
#pragma unroll
  for (int k = 0; k < S::BPL; ++k) {
    const int bin = li * S::BPL + k;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int i = k * D + d;
      int v = (int)(signed char)((wv[i >> 2] >> (8 * (i & 3))) & 0xff);
      v = bin == sub ? v - item[d] : v;
      f[k * 2 * D + d] = (float)v / vobs_capf(d, c...);
      f[k * 2 * D + D + d] = (float)item[d] / vobs_capf(d, c...);
    }
  }
  constexpr int F4 = S::NF / 4;
  constexpr int G = F4 % 8 == 0 ? 8 : F4;  // 16-byte pieces per lane and pass
  __shared__ f4v stage[4][64 * G];
  const int wib = threadIdx.x >> 6;
  // bit l: lane l's row is stored (every lane reaches the barriers below)
  const unsigned long long rows_live = __ballot(live);
  f4v *ob = reinterpret_cast<f4v *>(__builtin_assume_aligned(a.obs, 16)) +
            (size_t)(wave * S::RPW) * (S::LPE * F4);
#pragma unroll
  for (int s = 0; s < F4 / G; ++s) {
    if (s) __syncthreads();  // the previous pass's pieces have been read
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int w = s * G + g;
      f4v x = {f[4 * w], f[4 * w + 1], f[4 * w + 2], f[4 * w + 3]};
      stage[wib][lane * G + (g + lane) % G] = x;  // rotated: LDS banks
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int p = i * 64 + lane, lp = p / G, gg = p % G;
      if ((rows_live >> lp) & 1) {
        const f4v x = stage[wib][lp * G + (gg + lp) % G];
        __builtin_nontemporal_store(x, ob + lp * F4 + s * G + gg);
      }
    }
  }
}

// One env per lane, a reverse scan over T in chunks of 8 steps, latest first:
// every load of a chunk (done, reward, v_term and the 9 values V(S_hi+1) ..
// V(S_hi-7)) is issued before the chunk's arithmetic and unconditionally, as
// gae_kernel does, so a chunk costs one HBM round trip.  adv, td_target and
// lambda_return are written in the same pass.  part != nullptr: the block's
// sum and sum of squares of its advantages in double (lane sums compensated
// by xh_sums.h's sum2, then the wave by shuffles and the block's four waves in
// LDS, fixed order), and the block's count of ended rows.
__global__ __launch_bounds__(256) void venv_gae_kernel(VenvGaeArgs a) {
#pragma clang fp contract(off)
  const int N = a.N, T = a.T;
  const float gamma = a.gamma;
  const float lg = a.lambda * a.gamma;
  double s1 = 0.0, c1 = 0.0, s2 = 0.0, c2 = 0.0;
  int ended = 0;
  constexpr int C = 8;
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < N;
       env += gridDim.x * blockDim.x) {
    float A = 0.0f;
    for (int hi = T - 1; hi >= 0; hi -= C) {
      int dn[C];
      float rw[C], vt[C], v[C + 1];
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const int t = hi - k;
        const size_t i = (size_t)(t >= 0 ? t : 0) * N + env;
        dn[k] = a.done[i];
        rw[k] = a.reward[i];
        vt[k] = a.v_term ? a.v_term[i] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k <= C; ++k) {
        const int t = hi + 1 - k;  // v[k] = V(S_t), t = hi + 1 .. hi - 7
        v[k] = a.values[(size_t)(t >= 0 ? t : 0) * N + env];
      }
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const int t = hi - k;
        if (t < 0) break;
        const int done = dn[k];
        const float reward = rw[k];
        const float vn = done ? 0.0f : v[k];
        const float delta = reward + gamma * vn - v[k + 1];
        A = done ? delta : delta + lg * A;
        const size_t i = (size_t)t * N + env;
        a.adv[i] = A;
        if (a.td_target) a.td_target[i] = reward + gamma * (done ? vt[k] : v[k]);
        if (a.lambda_return) a.lambda_return[i] = A + v[k + 1];
        sum2(s1, c1, (double)A);
        sum2(s2, c2, (double)A * (double)A);
        ended += done != 0;
      }
    }
  }
  if (!a.part) return;
  s1 += c1;
  s2 += c2;
  __shared__ double red[2][4];
  __shared__ int redn[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, kWave);
    s2 += __shfl_xor(s2, o, kWave);
    ended += __shfl_xor(ended, o, kWave);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = s1;
    red[1][w] = s2;
    redn[w] = ended;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    a.part[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    a.end_part[blockIdx.x] = (redn[0] + redn[1]) + (redn[2] + redn[3]);
  }
}

// stats[2] = rows, stats[3] = ended rows: an integer sum of the block counts
// in one wave (exact in any order)
__global__ __launch_bounds__(64) void venv_adv_counts_kernel(const int *end_part,
                                                             int nparts,
                                                             double rows,
                                                             double *stats) {
  long long n = 0;
  for (int i = threadIdx.x; i < nparts; i += 64) n += end_part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
  if (threadIdx.x == 0) {
    stats[2] = rows;
    stats[3] = (double)n;
  }
}

// ------------------------------------------------------------- launchers --
#define XH_VOBS_SHAPES(X) \
  X(8, 1) X(8, 2) X(8, 3) X(16, 1) X(16, 2) X(16, 3) X(32, 1) X(32, 2)      \
  X(32, 3) X(64, 1) X(64, 2) X(64, 3) X(128, 1) X(128, 2) X(128, 3)

hipError_t launch_venv_record_obs(const VenvObsArgs &a, hipStream_t s,
                                  const int32_t *cap) {
  VObsCaps c{{1, 1, 1, 1}};
  for (int d = 0; cap && d < a.D && d < 4; ++d) c.cap[d] = cap[d];
  if (a.count <= 0) return hipSuccess;
  // NEXT needs a recorded transition (an out-of-range lane reads row 0's)
  if (a.N <= 0 || a.P < (a.next ? 1 : 0)) return hipErrorInvalidValue;
#define X(XB, XD)                                                             \
  if (a.B == XB && a.D == XD) {                                               \
    const long waves = (a.count + VObsShape<XB, XD>::RPW - 1) /               \
                       VObsShape<XB, XD>::RPW;                                \
    const long blocks = (waves + 3) / 4;                                      \
    if (blocks > 0x7fffffffl) return hipErrorInvalidValue;                    \
    if (cap)                                                                  \
      hipLaunchKernelGGL((venv_record_obs_kernel<XB, XD, VObsCaps>),          \
                         dim3((unsigned)blocks), dim3(256), 0, s, a, c);      \
    else                                                                      \
      hipLaunchKernelGGL((venv_record_obs_kernel<XB, XD>),                    \
                         dim3((unsigned)blocks), dim3(256), 0, s, a);         \
    return hipGetLastError();                                                 \
  }
  XH_VOBS_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

// one env per thread up to 2^20 envs, as gae_grid
int venv_gae_grid(int N) {
  const long b = ((long)N + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

hipError_t launch_venv_gae(const VenvGaeArgs &a, hipStream_t s) {
  if (a.N <= 0 || a.T <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(venv_gae_kernel, dim3(venv_gae_grid(a.N)), dim3(256), 0, s,
                     a);
  return hipGetLastError();
}

hipError_t launch_venv_adv_counts(const int *end_part, int nparts, double rows,
                                  double *stats, hipStream_t s) {
  hipLaunchKernelGGL(venv_adv_counts_kernel, dim3(1), dim3(64), 0, s, end_part,
                     nparts, rows, stats);
  return hipGetLastError();
}

}  // namespace xh
