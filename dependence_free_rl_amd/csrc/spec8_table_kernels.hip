// spec8_table_kernels.hip -- the streaming pass of the 64-bin 2-D [128,128]
// train epoch on the table ("the epoch on the table"; layouts
// spec8_pack_layout.h, xh_logit_table.h, spec8_table_layout.h).
//
// The per-bin net's logit is a function of the table entry (bin state, item)
// alone, and every parameter gradient is linear in the rows' loss gradient g at
// fixed activations, so the backward pass needs of the batch only
//   G_s = sum over the rows with entry s of g_row.
// Between the table's forward and backward: the stream, and -- only with the
// former table launches (policy_spec8_kernels.hip, XH_SP8_TAB_TU;
// XH_TRAIN_TABLE=spec8), since table_bwd_kernel (table_mm_kernels.hip) sums
// `part` itself in the same order -- the reduce:
//   stream  one wave per group of the packed batch, lane = row: the logit of
//           the row's entry from the table (LDS), the count-weighted softmax
//           of the row's segment (an env-step; a wide group: all 64 rows), the
//           PPO clipped-ratio / actor-critic gradient per distinct state -- the
//           packed build's expressions (pack_stage) -- added into the wave's
//           own f32 table in LDS; then the workgroup's waves' tables summed in
//           wave order, in double -> part
//   reduce  the workgroups' sums in workgroup order, in double, rounded to
//           f32 once -> G; max_s |G_s| -> gmax (an integer max over the bits)
// No float atomic: a segment's states are distinct, so its lanes add without
// conflict; a group's segments add one after the other; a wide group's rows
// (one env-step, states may repeat) add one row at a time, in row order.  A
// wave's groups, a workgroup's waves and the workgroups are summed in a fixed
// order: G is a function of the packed batch, the logits and the grid.
#include "spec8_pack_layout.h"
#include "spec8_table_layout.h"
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_logit_table.h"

namespace xh {
namespace sp8 {

constexpr int kTsWaves = 8;      // waves per workgroup of the stream
constexpr int kTrSlices = 16;    // waves per workgroup of the reduce
constexpr int kTrEntries = 64;   // entries per workgroup of the reduce

// the lanes' adds of one step are complete, and stay, before the next step's
__device__ __forceinline__ void wave_step() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct TsRow {
  int bins, cnt;  // the lane's row: its two bins (int8 pair), its count
  PkSeg seg;      // the record of the row's segment
};

__global__ __launch_bounds__(64 * kTsWaves) void table_stream_kernel(TableStreamArgs a) {
  __shared__ float zt[lt::kEntries];
  __shared__ float gt[kTsWaves][lt::kEntries];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int e = tid; e < lt::kEntries; e += 64 * kTsWaves) {
    zt[e] = a.logits[e];
#pragma unroll
    for (int u = 0; u < kTsWaves; ++u) gt[u][e] = 0.0f;
  }
  if (blockIdx.x == 0 && tid == 0) *a.gmax = 0.0f;  // (the reduce's max starts here)
  __syncthreads();
  const int ngroups = __builtin_amdgcn_readfirstlane(a.pk_hdr[kPkGroups]);
  const int ga = __builtin_amdgcn_readfirstlane(a.pk_hdr[kPkGA]);
  const int np = ga + __builtin_amdgcn_readfirstlane(a.pk_hdr[kPkGB]);
  const int ua = __builtin_amdgcn_readfirstlane(a.pk_hdr[kPkUA]);
  float *tab = gt[w];
  int ood = 0;  // wave-uniform
  auto load = [&](int g) {
    const uint8_t *rec = a.pk + (size_t)g * kPkGroupBytes;
    TsRow r;
    r.bins = reinterpret_cast<const unsigned short *>(rec + kPkStates)[lane];
    r.cnt = rec[kPkCounts + lane];
    r.seg = reinterpret_cast<const PkSeg *>(rec + kPkSegRecs)[lane / kPkSegRows];
    return r;
  };
  // wave w of workgroup b: groups b + gridDim.x (w + kTsWaves i), the next
  // one's record loaded a group ahead
  const int step = (int)gridDim.x * kTsWaves;
  int g = (int)blockIdx.x + (int)gridDim.x * w;
  TsRow cur{};
  if (g < ngroups) cur = load(g);
  for (; g < ngroups; g += step) {
    TsRow nxt = cur;
    if (g + step < ngroups) nxt = load(g + step);
    const bool ia = g < ga || (g >= np && g < np + ua);
    const bool wide = g >= np;
    int b0 = (signed char)(cur.bins & 0xff), b1 = (signed char)((cur.bins >> 8) & 0xff);
    const bool live = cur.cnt != 0;
    // a state outside the table (the host gate keeps such batches away): the
    // nearest entry, and counted
    const bool out = b0 < -lt::kCap || b0 > lt::kCap || b1 < -lt::kCap || b1 > lt::kCap;
    ood += (int)__builtin_popcountll(__ballot(out && live));
    b0 = min(max(b0, -lt::kCap), lt::kCap);
    b1 = min(max(b1, -lt::kCap), lt::kCap);
    const int e = lt::entry(ia ? 0 : 1, b0, b1);
    const float c = (float)cur.cnt;
    const float ex = __expf(zt[e]);
    float ssum = seg_sum<kPkSegRows>(c * ex);
    if (wide) {  // wave-uniform: one env-step over all four segments
      ssum += __shfl_xor(ssum, 16, kWave);
      ssum += __shfl_xor(ssum, 32, kWave);
    }
    const float se = ssum > 0.0f ? ssum : 1.0f;  // (an empty segment: p stays finite)
    const float p = ex * __builtin_amdgcn_rcpf(se);
    const int cu = cur.seg.cu;  // the chosen bin's row = its lane; -1: empty
    const float pc = __shfl(p, cu & 63, kWave);
    const float cp = c * p, A = cur.seg.adv;
    float gv;
    if (a.algo == kPPO) {
      // clipped_gradient through softmax_layer::backward, closed under the
      // counts (policy_spec8_kernels.hip, pack_stage)
      const float ce = a.clip_eps;
      const float r = pc * __builtin_amdgcn_rcpf(cur.seg.pold);
      const float k = fminf(fmaxf(r, 1.0f - ce), 1.0f + ce);
      const float ig = fminf(k * A, r * A) * -1.0f;
      const float gc = ig * __builtin_amdgcn_rcpf(pc);
      gv = ((lane == cu ? p : 0.0f) - cp * pc) * gc;
    } else {
      gv = cp * A;
      if (lane == cu) gv -= A;
    }
    if (!live || cu < 0) gv = 0.0f;
    if (!wide) {
      for (int q = 0; q < kPkSegs; ++q) {  // the segments in order
        if (lane / kPkSegRows == q && live) tab[e] += gv;
        wave_step();
      }
    } else {
      for (int r = 0; r < kPkSegs * kPkSegRows; ++r) {  // the rows in order
        if (lane == r) tab[e] += gv;
        wave_step();
      }
    }
    cur = nxt;
  }
  __syncthreads();
  double *part = a.part + (size_t)blockIdx.x * lt::kEntries;
  for (int e = tid; e < lt::kEntries; e += 64 * kTsWaves) {
    double v = 0.0;
#pragma unroll
    for (int u = 0; u < kTsWaves; ++u) v += (double)gt[u][e];
    part[e] = v;
  }
  if (a.ood && lane == 0 && ood) atomicAdd(a.ood, ood);
}

// reduce: workgroup b owns the entries [64 b, 64 b + 64); wave k sums the
// parts k, k + 16, ..., then the 16 waves' sums in wave order
__global__ __launch_bounds__(64 * kTrSlices) void table_reduce_kernel(TableStreamArgs a,
                                                                      int nparts) {
  __shared__ double sc[kTrSlices][kTrEntries];
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  const int e = (int)blockIdx.x * kTrEntries + lane;
  double v = 0.0;
  if (e < lt::kEntries)
    for (int p = k; p < nparts; p += kTrSlices) v += a.part[(size_t)p * lt::kEntries + e];
  sc[k][lane] = v;
  __syncthreads();
  if (k == 0) {
    double t = 0.0;
#pragma unroll
    for (int u = 0; u < kTrSlices; ++u) t += sc[u][lane];
    const float gs = (float)t;
    if (e < lt::kEntries) a.G[e] = gs;
    float m = e < lt::kEntries ? fabsf(gs) : 0.0f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
    // (non-negative floats order as their bits)
    if (lane == 0) atomicMax(reinterpret_cast<unsigned *>(a.gmax), __float_as_uint(m));
  }
}

}  // namespace sp8

hipError_t launch_table_stream(const TableStreamArgs &a, int grid, hipStream_t s, bool reduce) {
  if (!a.pk || !a.pk_hdr || !a.logits || !a.part || !a.G || !a.gmax || grid < 1 ||
      (a.algo != kPPO && a.algo != kAC))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sp8::table_stream_kernel, dim3(grid), dim3(64 * sp8::kTsWaves), 0, s, a);
  if (!reduce) return hipGetLastError();  // (table_bwd_kernel sums `part` itself)
  const int blocks = (lt::kEntries + sp8::kTrEntries - 1) / sp8::kTrEntries;
  hipLaunchKernelGGL(sp8::table_reduce_kernel, dim3(blocks), dim3(64 * sp8::kTrSlices), 0, s, a,
                     grid);
  return hipGetLastError();
}

}  // namespace xh
