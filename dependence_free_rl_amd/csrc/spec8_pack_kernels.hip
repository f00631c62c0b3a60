// spec8_pack_kernels.hip -- the compaction pass of the 64-bin 2-D [128,128]
// train epoch ("duplicate rows"; layout spec8_pack_layout.h):
// once per learn(), from the batch's slots 0 .. T-1 (the same in all k
// epochs), the final advantages and p_old, the packed batch that
// policy_train_spec8_kernel's packed build reads.
//
// Three launches, integer work only, no float arithmetic at all and no atomic
// on global memory (classify and write by default find the duplicate states
// through a bitwise OR into LDS, further down; XH_SP8_PACK_DEDUP=loop: the
// kernels here, with no atomic at all):
//   classify  one wave per env-step (lane = bin): the number of distinct bin
//             states among the 64 bins -> the env-step's class (packable /
//             wide, by item); per chunk of 64 env-steps the classes' counts
//   scan      one workgroup: the exclusive prefix counts of the chunks per
//             class, in batch order, and the header
//   write     one wave per env-step: the distinct states in first-occurrence
//             order, their counts, the chosen bin's slot, into the segment the
//             prefix count names; the last env-step of a packed class also
//             writes the empty segments behind it
// Every output position is a prefix sum over the batch, so the layout -- and
// every float sum of the epochs that read it -- is a function of the batch
// alone.  No host synchronisation: the train kernel reads the group count
// from the header.
#include "spec8_pack_layout.h"
#include "xh_device.h"
#include "xh_kernels.h"

namespace xh {
namespace sp8 {

constexpr int kPkWaves = 4;         // waves per workgroup
constexpr int kPkChunk = 64;        // env-steps per workgroup
constexpr int kPkScanThreads = 1024;

// The distinct values of `key` over the wave's 64 lanes in first-occurrence
// order: returns their number, capped at kPkSegRows + 1 (a wide env-step);
// `slot` = the lane's value's index, `count` = its multiplicity, `first` =
// the lane is its value's first occurrence.  Lanes of values past the cap
// keep slot -1.
__device__ __forceinline__ int distinct64(int key, int &slot, int &count, bool &first) {
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  unsigned long long left = ~0ull;
  int d = 0;
  slot = -1;
  count = 0;
  first = false;
  while (left != 0ull && d <= kPkSegRows) {  // wave-uniform
    const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(left));
    const int kv = __builtin_amdgcn_readlane(key, lead);
    const unsigned long long m = __ballot(key == kv);
    if (key == kv) {
      slot = d;
      count = (int)__builtin_popcountll(m);
      first = lane == lead;
    }
    left &= ~m;
    ++d;
  }
  return d;
}

__device__ __forceinline__ int step_key(const Batch &b, size_t e, int lane) {
  return reinterpret_cast<const unsigned short *>(b.bins + e * (kPkSegs * kPkSegRows * 2))[lane];
}
__device__ __forceinline__ bool step_is_a(const EnvDesc &env, const Batch &b, size_t e) {
  const int8_t *it = b.items + e * 4;
  return it[0] == env.item_a[0] && it[1] == env.item_a[1];
}

// classify: workgroup b owns the env-steps [kPkChunk b, kPkChunk b + kPkChunk),
// a wave every kPkWaves-th of them; the chunk's counts per class -> blk
__global__ __launch_bounds__(64 * kPkWaves) void pack_classify_kernel(PackArgs a) {
  __shared__ int cnt[kPkWaves][kPkClasses];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long nt = (long)a.b.T * a.b.N;
  const long e0 = (long)blockIdx.x * kPkChunk;
  int n[kPkClasses] = {0, 0, 0, 0};  // wave-uniform
  for (int i = w; i < kPkChunk && e0 + i < nt; i += kPkWaves) {
    const long e = e0 + i;
    int slot, count;
    bool first;
    const int d = distinct64(step_key(a.b, (size_t)e, lane), slot, count, first);
    const bool ia = step_is_a(a.env, a.b, (size_t)e);
    const int k = (d > kPkSegRows ? kPkClsWideA : kPkClsA) + (ia ? 0 : 1);
    if (lane == 0) a.cls[e] = (uint8_t)k;
#pragma unroll
    for (int q = 0; q < kPkClasses; ++q) n[q] += k == q;
  }
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < kPkClasses; ++q) cnt[w][q] = n[q];
  __syncthreads();
  if (threadIdx.x < kPkClasses) {
    int v = 0;
#pragma unroll
    for (int u = 0; u < kPkWaves; ++u) v += cnt[u][threadIdx.x];
    a.blk[(size_t)blockIdx.x * kPkClasses + threadIdx.x] = v;
  }
}

// scan: thread i owns the chunks [i c, i c + c), c = ceil(chunks / threads):
// its counts per class, the exclusive scan of the threads' counts
// (Hillis-Steele in LDS, integers), then each chunk's offsets per class
// (behind the counts in blk) and the header
__global__ __launch_bounds__(kPkScanThreads) void pack_scan_kernel(PackArgs a) {
  __shared__ int sc[2][kPkClasses][kPkScanThreads];
  const int tid = threadIdx.x;
  const long nt = (long)a.b.T * a.b.N;
  const long nb = (nt + kPkChunk - 1) / kPkChunk;
  const long c = (nb + kPkScanThreads - 1) / kPkScanThreads;
  const long b0 = min((long)tid * c, nb), b1 = min(b0 + c, nb);
  const int *cnt = a.blk;
  int *off = a.blk + nb * kPkClasses;
  int n[kPkClasses] = {0, 0, 0, 0};
  for (long b = b0; b < b1; ++b)
#pragma unroll
    for (int q = 0; q < kPkClasses; ++q) n[q] += cnt[b * kPkClasses + q];
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) sc[0][q][tid] = n[q];
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < kPkScanThreads; o <<= 1) {
#pragma unroll
    for (int q = 0; q < kPkClasses; ++q)
      sc[cur ^ 1][q][tid] = sc[cur][q][tid] + (tid >= o ? sc[cur][q][tid - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  int p[kPkClasses];
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) p[q] = sc[cur][q][tid] - n[q];  // exclusive
  for (long b = b0; b < b1; ++b)
#pragma unroll
    for (int q = 0; q < kPkClasses; ++q) {
      off[b * kPkClasses + q] = p[q];
      p[q] += cnt[b * kPkClasses + q];
    }
  if (tid == kPkScanThreads - 1) {
    const int na = sc[cur][kPkClsA][tid], nbb = sc[cur][kPkClsB][tid],
              ua = sc[cur][kPkClsWideA][tid], ub = sc[cur][kPkClsWideB][tid];
    const int ga = (na + kPkSegs - 1) / kPkSegs, gb = (nbb + kPkSegs - 1) / kPkSegs;
    a.hdr[kPkNA] = na;
    a.hdr[kPkNB] = nbb;
    a.hdr[kPkUA] = ua;
    a.hdr[kPkUB] = ub;
    a.hdr[kPkGA] = ga;
    a.hdr[kPkGB] = gb;
    a.hdr[kPkGroups] = ga + gb + ua + ub;
    a.hdr[kPkHdrInts - 1] = 0;
  }
}

// write: the chunks as in classify; an env-step's position in its class = the
// chunk's offset + the chunk's earlier env-steps of the class (ballots over the
// chunk's classes, lane = env-step)
__global__ __launch_bounds__(64 * kPkWaves) void pack_write_kernel(PackArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long nt = (long)a.b.T * a.b.N;
  const long nbk = (nt + kPkChunk - 1) / kPkChunk;
  const int na = a.hdr[kPkNA], nb = a.hdr[kPkNB], ua = a.hdr[kPkUA];
  const int ga = a.hdr[kPkGA], gb = a.hdr[kPkGB];
  const long e0 = (long)blockIdx.x * kPkChunk;
  const int *off = a.blk + (nbk + blockIdx.x) * kPkClasses;
  const int kk = e0 + lane < nt ? (int)a.cls[e0 + lane] : -1;
  unsigned long long mk[kPkClasses];
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) mk[q] = __ballot(kk == q);
  for (int i = w; i < kPkChunk && e0 + i < nt; i += kPkWaves) {
    const long e = e0 + i;
    const int key = step_key(a.b, (size_t)e, lane);
    int slot, count;
    bool first;
    const int d = distinct64(key, slot, count, first);
    const int k = __builtin_amdgcn_readlane(kk, i);
    unsigned long long m = mk[0];
#pragma unroll
    for (int q = 1; q < kPkClasses; ++q) m = k == q ? mk[q] : m;
    const int p = off[k] + (int)__builtin_popcountll(m & ((1ull << i) - 1ull));
    const int act = a.b.action[e];
    const float po = a.b.pold[e], ad = a.adv[e];
    if (k >= kPkClsWideA) {
      uint8_t *rec = a.pk + (size_t)(ga + gb + (k == kPkClsWideA ? 0 : ua) + p) * kPkGroupBytes;
      reinterpret_cast<unsigned short *>(rec + kPkStates)[lane] = (unsigned short)key;
      rec[kPkCounts + lane] = 1;
      if (lane < kPkSegs)
        reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[lane] = PkSeg{act, po, ad, (int32_t)e};
      continue;
    }
    const int q = p % kPkSegs;
    uint8_t *rec = a.pk + (size_t)((k == kPkClsA ? 0 : ga) + p / kPkSegs) * kPkGroupBytes;
    unsigned short *st = reinterpret_cast<unsigned short *>(rec + kPkStates) + kPkSegRows * q;
    uint8_t *cn = rec + kPkCounts + kPkSegRows * q;
    // its states (slot < kPkSegRows: the env-step is packable) and the slots
    // it does not use
    if (first) {
      st[slot] = (unsigned short)key;
      cn[slot] = (uint8_t)count;
    }
    if (lane >= d && lane < kPkSegRows) {  // (slots d .. 15: no state's)
      st[lane] = 0;
      cn[lane] = 0;
    }
    const int cs = __shfl(slot, act & 63, 64);
    if (lane == 0)
      reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[q] =
          PkSeg{kPkSegRows * q + cs, po, ad, (int32_t)e};
    // the class's last env-step: the group's segments behind it are empty
    if (p == (k == kPkClsA ? na : nb) - 1) {
      for (int qq = q + 1; qq < kPkSegs; ++qq) {
        if (lane < kPkSegRows) {
          reinterpret_cast<unsigned short *>(rec + kPkStates)[kPkSegRows * qq + lane] = 0;
          rec[kPkCounts + kPkSegRows * qq + lane] = 0;
        }
        if (lane == 0)
          reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[qq] = PkSeg{-1, 1.0f, 0.0f, -1};
      }
    }
  }
}

// ---- classify and write on lane masks ("the duplicate
// search"; spec8_pack_layout.h: pk_dedup).  The same outputs, byte for byte;
// distinct64's loop, one dependent iteration per distinct state and run once
// per kernel, becomes: the states of the first lanes taken off by a ballot
// (at most kPkPeel of them, while more than kPkPeelStop lanes remain: the
// environment's batches have one state in most bins, and lanes that OR into
// one LDS word are served one after the other), the remaining lanes' sets
// from one LDS OR into the wave's own table of lane masks.  A bitwise OR ends
// at the same word in any order.  An env-step with a state outside the
// table's domain (a bin set by hand below -8) takes distinct64.  The wave's
// kPkSteps env-steps' loads are issued before the loop.
#ifndef XH_PK_PEEL
#define XH_PK_PEEL 2
#endif
constexpr int kPkSteps = kPkChunk / kPkWaves;  // env-steps per wave
constexpr int kPkPeel = XH_PK_PEEL, kPkPeelStop = 16;
static_assert(kPkSteps <= 64 && kPkCap == 8, "a lane per env-step of the wave; the domain");

// the lanes' LDS operations of one step are complete, and stay, before the
// next step's (spec8_table_kernels.hip)
__device__ __forceinline__ void wave_step() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// distinct64's outputs (d not capped) for the wave's 64 keys; `tab`: the
// wave's kPkMaskWords words, all zero on entry and on return
__device__ __forceinline__ int distinct_mask(int key, int lane, unsigned long long *tab, int &slot,
                                             int &count, bool &first) {
  const int b0 = (signed char)(key & 0xff), b1 = (signed char)((key >> 8) & 0xff);
  if (__ballot(pk_in_domain(b0, b1)) != ~0ull)  // wave-uniform
    return distinct64(key, slot, count, first);
  unsigned long long m = 0ull;  // the lanes of the lane's state
  unsigned long long left = ~0ull;  // wave-uniform: lanes whose m is not known yet
#pragma unroll
  for (int r = 0; r < kPkPeel; ++r) {
    if ((int)__builtin_popcountll(left) <= kPkPeelStop) break;
    const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(left));
    const int kv = __builtin_amdgcn_readlane(key, lead);
    const unsigned long long mm = __ballot(key == kv);
    if (key == kv) m = mm;
    left &= ~mm;
  }
  if (left != 0ull) {  // wave-uniform
    const bool mine = m == 0ull;
    unsigned long long *word = tab + pk_mask_index(b0, b1);
    if (mine) __hip_atomic_fetch_or(word, 1ull << lane, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_WORKGROUP);
    wave_step();
    if (mine) m = *word;
    wave_step();
    if (mine) *word = 0ull;
    wave_step();
  }
  const unsigned long long F = __ballot(pk_dedup_first(m, lane));
  const PkDedup r = pk_dedup(m, F, lane);
  slot = r.slot;
  count = r.count;
  first = r.first;
  return r.d;
}

// the wave's table, zeroed by the wave itself
__device__ __forceinline__ void mask_table_init(unsigned long long *tab, int lane) {
  for (int e = lane; e < kPkMaskWords; e += 64) tab[e] = 0ull;
  wave_step();
}

// step j of wave w of the chunk at e0: env-step e0 + w + kPkWaves j; the loads
// of a step past the batch's end read the last env-step (in bounds, not used)
__device__ __forceinline__ long wave_step_index(long e0, int w, int j, long nt) {
  return min(e0 + w + (long)kPkWaves * j, nt - 1);
}

__global__ __launch_bounds__(64 * kPkWaves) void pack_classify_mask_kernel(PackArgs a) {
  __shared__ unsigned long long mask[kPkWaves][kPkMaskWords];
  __shared__ int cnt[kPkWaves][kPkClasses];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long nt = (long)a.b.T * a.b.N;
  const long e0 = (long)blockIdx.x * kPkChunk;
  int key[kPkSteps];
#pragma unroll
  for (int j = 0; j < kPkSteps; ++j)
    key[j] = step_key(a.b, (size_t)wave_step_index(e0, w, j, nt), lane);
  // lane j: the item of step j
  const bool ia_l =
      step_is_a(a.env, a.b, (size_t)wave_step_index(e0, w, lane & (kPkSteps - 1), nt));
  mask_table_init(mask[w], lane);
  const unsigned long long ia_m = __ballot(ia_l);
  int kl = 0;  // lane j: the class of step j
#pragma unroll
  for (int j = 0; j < kPkSteps; ++j) {
    if (e0 + w + kPkWaves * j >= nt) break;
    int slot, count;
    bool first;
    const int d = distinct_mask(key[j], lane, mask[w], slot, count, first);
    const bool ia = (ia_m >> j) & 1ull;
    const int k = (d > kPkSegRows ? kPkClsWideA : kPkClsA) + (ia ? 0 : 1);
    kl = lane == j ? k : kl;
  }
  const bool mine = lane < kPkSteps && e0 + w + kPkWaves * lane < nt;
  if (mine) a.cls[e0 + w + kPkWaves * lane] = (uint8_t)kl;
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) {
    const int nq = (int)__builtin_popcountll(__ballot(mine && kl == q));
    if (lane == 0) cnt[w][q] = nq;
  }
  __syncthreads();
  if (threadIdx.x < kPkClasses) {
    int v = 0;
#pragma unroll
    for (int u = 0; u < kPkWaves; ++u) v += cnt[u][threadIdx.x];
    a.blk[(size_t)blockIdx.x * kPkClasses + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64 * kPkWaves) void pack_write_mask_kernel(PackArgs a) {
  __shared__ unsigned long long mask[kPkWaves][kPkMaskWords];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long nt = (long)a.b.T * a.b.N;
  const long nbk = (nt + kPkChunk - 1) / kPkChunk;
  const long e0 = (long)blockIdx.x * kPkChunk;
  int key[kPkSteps];
#pragma unroll
  for (int j = 0; j < kPkSteps; ++j)
    key[j] = step_key(a.b, (size_t)wave_step_index(e0, w, j, nt), lane);
  // lane j: the action, p_old and advantage of step j
  const long el = wave_step_index(e0, w, lane & (kPkSteps - 1), nt);
  const int act_l = a.b.action[el];
  const float po_l = a.b.pold[el], ad_l = a.adv[el];
  const int na = a.hdr[kPkNA], nb = a.hdr[kPkNB], ua = a.hdr[kPkUA];
  const int ga = a.hdr[kPkGA], gb = a.hdr[kPkGB];
  const int *off = a.blk + (nbk + blockIdx.x) * kPkClasses;
  int offq[kPkClasses];
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) offq[q] = off[q];
  const int kk = e0 + lane < nt ? (int)a.cls[e0 + lane] : -1;
  unsigned long long mk[kPkClasses];
#pragma unroll
  for (int q = 0; q < kPkClasses; ++q) mk[q] = __ballot(kk == q);
  mask_table_init(mask[w], lane);
#pragma unroll
  for (int j = 0; j < kPkSteps; ++j) {
    const int i = w + kPkWaves * j;
    if (e0 + i >= nt) break;
    const long e = e0 + i;
    int slot, count;
    bool first;
    const int d = distinct_mask(key[j], lane, mask[w], slot, count, first);
    const int k = __builtin_amdgcn_readlane(kk, i);
    unsigned long long m = mk[0];
    int p = offq[0];
#pragma unroll
    for (int q = 1; q < kPkClasses; ++q) {
      m = k == q ? mk[q] : m;
      p = k == q ? offq[q] : p;
    }
    p += (int)__builtin_popcountll(m & ((1ull << i) - 1ull));
    const int act = __builtin_amdgcn_readlane(act_l, j);
    const float po = __builtin_bit_cast(
        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, po_l), j));
    const float ad = __builtin_bit_cast(
        float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ad_l), j));
    if (k >= kPkClsWideA) {
      uint8_t *rec = a.pk + (size_t)(ga + gb + (k == kPkClsWideA ? 0 : ua) + p) * kPkGroupBytes;
      reinterpret_cast<unsigned short *>(rec + kPkStates)[lane] = (unsigned short)key[j];
      rec[kPkCounts + lane] = 1;
      if (lane < kPkSegs)
        reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[lane] = PkSeg{act, po, ad, (int32_t)e};
      continue;
    }
    const int q = p % kPkSegs;
    uint8_t *rec = a.pk + (size_t)((k == kPkClsA ? 0 : ga) + p / kPkSegs) * kPkGroupBytes;
    unsigned short *st = reinterpret_cast<unsigned short *>(rec + kPkStates) + kPkSegRows * q;
    uint8_t *cn = rec + kPkCounts + kPkSegRows * q;
    // its states (slot < kPkSegRows: the env-step is packable) and the slots
    // it does not use.  (Staging (state, count) by slot in LDS so that lanes
    // 0 .. 15 write the segment's 48 bytes contiguously measured the same,
    // DESIGN.md §8, and is not kept.)
    if (first) {
      st[slot] = (unsigned short)key[j];
      cn[slot] = (uint8_t)count;
    }
    if (lane >= d && lane < kPkSegRows) {  // (slots d .. 15: no state's)
      st[lane] = 0;
      cn[lane] = 0;
    }
    const int cs = __shfl(slot, act & 63, 64);
    if (lane == 0)
      reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[q] =
          PkSeg{kPkSegRows * q + cs, po, ad, (int32_t)e};
    // the class's last env-step: the group's segments behind it are empty
    if (p == (k == kPkClsA ? na : nb) - 1) {
      for (int qq = q + 1; qq < kPkSegs; ++qq) {
        if (lane < kPkSegRows) {
          reinterpret_cast<unsigned short *>(rec + kPkStates)[kPkSegRows * qq + lane] = 0;
          rec[kPkCounts + kPkSegRows * qq + lane] = 0;
        }
        if (lane == 0)
          reinterpret_cast<PkSeg *>(rec + kPkSegRecs)[qq] = PkSeg{-1, 1.0f, 0.0f, -1};
      }
    }
  }
}

}  // namespace sp8

hipError_t launch_spec8_pack(const PackArgs &a, bool loop, hipStream_t s) {
  if (!a.pk || !a.hdr || !a.cls || !a.blk || !a.adv || a.env.B != 64 || a.env.D != 2)
    return hipErrorInvalidValue;
  const long nt = (long)a.b.T * a.b.N;
  if (nt <= 0) return hipErrorInvalidValue;
  const int grid = (int)((nt + sp8::kPkChunk - 1) / sp8::kPkChunk);
  const dim3 block(64 * sp8::kPkWaves);
  if (loop)
    hipLaunchKernelGGL(sp8::pack_classify_kernel, dim3(grid), block, 0, s, a);
  else
    hipLaunchKernelGGL(sp8::pack_classify_mask_kernel, dim3(grid), block, 0, s, a);
  hipLaunchKernelGGL(sp8::pack_scan_kernel, dim3(1), dim3(sp8::kPkScanThreads), 0, s, a);
  if (loop)
    hipLaunchKernelGGL(sp8::pack_write_kernel, dim3(grid), block, 0, s, a);
  else
    hipLaunchKernelGGL(sp8::pack_write_mask_kernel, dim3(grid), block, 0, s, a);
  return hipGetLastError();
}

}  // namespace xh
