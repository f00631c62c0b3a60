// spec8_pack_kernels.hip -- the compaction pass of the 64-bin 2-D [128,128]
// train epoch ("duplicate rows"; layout spec8_pack_layout.h):
// once per learn(), from the batch's slots 0 .. T-1 (the same in all k
// epochs), the final advantages and p_old, the packed batch that
// policy_train_spec8_kernel's packed build reads.
//
// Three launches, integer work only, no float arithmetic at all and no atomic:
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

}  // namespace sp8

hipError_t launch_spec8_pack(const PackArgs &a, hipStream_t s) {
  if (!a.pk || !a.hdr || !a.cls || !a.blk || !a.adv || a.env.B != 64 || a.env.D != 2)
    return hipErrorInvalidValue;
  const long nt = (long)a.b.T * a.b.N;
  const int grid = (int)((nt + sp8::kPkChunk - 1) / sp8::kPkChunk);
  hipLaunchKernelGGL(sp8::pack_classify_kernel, dim3(grid), dim3(64 * sp8::kPkWaves), 0, s, a);
  hipLaunchKernelGGL(sp8::pack_scan_kernel, dim3(1), dim3(sp8::kPkScanThreads), 0, s, a);
  hipLaunchKernelGGL(sp8::pack_write_kernel, dim3(grid), dim3(64 * sp8::kPkWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace xh
