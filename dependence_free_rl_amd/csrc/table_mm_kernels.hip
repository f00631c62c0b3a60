// table_mm_kernels.hip -- the forward and the backward of the 64-bin 2-D
// [128,128] train epoch on the table ("the epoch on the
// table"; tiles: table_tile_layout.h), on the exact f32 MFMA.
//
// The table has lt::kEntries = 578 (bin state, item) points: three
// 578 x 128 x 128 products per epoch, about 57 MFLOP.  At that size the f16-pair
// machinery of policy_spec8_kernels.hip (scale reductions over W2, split
// fragments, the bound on |G|) costs more than the products, so these kernels
// take v_mfma_f32_16x16x4_f32 with W2 straight from L2: no scale, no split, no
// bound.  One workgroup of four waves per tile of tt::kR entries:
//   table_fwd_kernel  layer 1 from the exact f32 chain (the expression of the
//                     spec8 kernel's hk, the item folded into the bias the same
//                     way) -> LDS; layer 2 on the MFMA; relu; the w3 dot + b3
//                     -> logits[e]; H2 (f32; the mask is H2 > 0) -> h2[row]
//   table_bwd_kernel  G of the tile's entries from the stream's per-workgroup
//                     sums (tt::part_slice_sum / tt::part_total: the order of
//                     table_reduce_kernel, no atomics, no waiting on another
//                     workgroup); dz2 = G (x) w3 o [H2 > 0], dW3 / db2 / db3;
//                     dH1 = dz2 W2 o [H1 > 0] and dW2 = dz2^T H1 on the MFMA
//                     (H1 recomputed from the same chain: the same bits); dW1 /
//                     db1 / the item sums; one slab in the slab layout
//                     (PolicyLayout) per tile.
// MFMA operand maps (16x16x4, lane l): A[m = l & 15][k = l >> 4], B[k = l >> 4]
// [n = l & 15], D register j: [m = 4 (l >> 4) + j][n = l & 15].  Along K the
// kernels put element 16 kg + 4 (l >> 4) + s in slot l >> 4 of step s of K
// group kg (A and B alike), so that a lane's four steps read one float4.
// Tail rows (tt::is_tail) are computed on the last entry's state with G = 0:
// every product they enter is an exact zero, and they write no logit.
#include "table_tile_layout.h"
#include "xh_device.h"
#include "xh_kernels.h"

namespace xh {
namespace tm {

constexpr int kH = 128, kF0 = 4, kD = 2;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRT = tt::kR / 16;  // 16-row MFMA tiles of a table tile
// LDS row stride of the [row][128] images: the 16 floats four consecutive rows
// contribute to one B fragment fall into disjoint banks (144 mod 64 = 16)
constexpr int kLS = 144;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }

// the rows' inputs: bins / capacity of the row's entry, and its item
struct TileRows {
  float x0[tt::kR], x1[tt::kR];
  int item_a[tt::kR];  // 1: item_a
  int entry[tt::kR];   // -1: a tail row
};
__device__ __forceinline__ void stage_rows(TileRows &tr, int tile) {
  const int r = threadIdx.x;
  if (r < tt::kR) {
    const int e = tt::row_entry(tile, r);
    const int es = e < 0 ? lt::kEntries - 1 : e;
    int b0, b1;
    tt::entry_bins(es, b0, b1);
    tr.x0[r] = (float)b0 / (float)kCapacity;
    tr.x1[r] = (float)b1 / (float)kCapacity;
    tr.item_a[r] = tt::entry_item(es) == 0;
    tr.entry[r] = e;
  }
}

// H1 of the tile -> h1s[row][i]: feature i = tid & 127, rows tid >> 7, + 2, ...
// (the exact f32 chain: policy_spec8_kernels.hip, h1_4, at scale 1)
__device__ __forceinline__ void layer1(const float *__restrict__ P, const EnvDesc &env,
                                       const TileRows &tr, float *h1s) {
  const PolicyLayout PL{kF0, kH, kH};
  const int fi = threadIdx.x & (kH - 1), half = threadIdx.x >> 7;
  const float w1a = P[PL.oW1() + fi * kF0], w1b = P[PL.oW1() + fi * kF0 + 1];
  float b1a = P[PL.ob1() + fi], b1b = b1a;
#pragma unroll
  for (int d = 0; d < kD; ++d) {
    const float wv = P[PL.oW1() + fi * kF0 + kD + d];
    b1a += wv * ((float)env.item_a[d] / (float)kCapacity);
    b1b += wv * ((float)env.item_b[d] / (float)kCapacity);
  }
#pragma unroll
  for (int r = half; r < tt::kR; r += 2) {
    const float b1 = tr.item_a[r] ? b1a : b1b;
    h1s[r * kLS + fi] = relu(fmaf(tr.x1[r], w1b, fmaf(tr.x0[r], w1a, b1)));
  }
}

__global__ __launch_bounds__(kThreads) void table_fwd_kernel(TableFwdArgs a) {
  __shared__ TileRows tr;
  __shared__ __attribute__((aligned(16))) float h1s[tt::kR * kLS];
  __shared__ float zp[kWaves][tt::kR];
  const PolicyLayout PL{kF0, kH, kH};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  if (a.zero_ood && tile == 0 && tid == 0) *a.zero_ood = 0;
  // this wave's W2 fragments: outputs o = 16 (2 w + ot) + n, K group kg
  v4f bw[2][8];
#pragma unroll
  for (int ot = 0; ot < 2; ++ot)
#pragma unroll
    for (int kg = 0; kg < 8; ++kg)
      bw[ot][kg] = *reinterpret_cast<const v4f *>(P + PL.oW2() + (16 * (2 * w + ot) + n) * kH +
                                                  16 * kg + 4 * kk);
  stage_rows(tr, tile);
  __syncthreads();
  layer1(P, a.env, tr, h1s);
  __syncthreads();
  v4f acc[2][kRT];
#pragma unroll
  for (int ot = 0; ot < 2; ++ot)
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) acc[ot][rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int kg = 0; kg < 8; ++kg) {
    v4f ah[kRT];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
      ah[rt] = *reinterpret_cast<const v4f *>(h1s + (16 * rt + n) * kLS + 16 * kg + 4 * kk);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
          acc[ot][rt] = mfma16(ah[rt][s], bw[ot][kg][s], acc[ot][rt]);
  }
  // H2 = relu(. + b2) -> h2; the w3 dot over this wave's 32 outputs
  float b2v[2], w3v[2];
#pragma unroll
  for (int ot = 0; ot < 2; ++ot) {
    b2v[ot] = P[PL.ob2() + 16 * (2 * w + ot) + n];
    w3v[ot] = P[PL.ow3() + 16 * (2 * w + ot) + n];
  }
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 16 * rt + 4 * kk + j;
      float z = 0.0f;
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        const float h = relu(acc[ot][rt][j] + b2v[ot]);
        a.h2[((size_t)tile * tt::kR + r) * kH + 16 * (2 * w + ot) + n] = h;
        z = fmaf(h, w3v[ot], z);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) z += __shfl_xor(z, o, kWave);
      if (n == 0) zp[w][r] = z;
    }
  __syncthreads();
  if (tid < tt::kR && tr.entry[tid] >= 0)
    a.logits[tr.entry[tid]] =
        ((zp[0][tid] + zp[1][tid]) + (zp[2][tid] + zp[3][tid])) + P[PL.ob3()];
}

__global__ __launch_bounds__(kThreads) void table_bwd_kernel(TableBwdArgs a) {
  __shared__ TileRows tr;
  __shared__ double sc[tt::kSlices][tt::kR];
  __shared__ float gs[tt::kR];
  __shared__ __attribute__((aligned(16))) float h1s[tt::kR * kLS];
  __shared__ __attribute__((aligned(16))) float dz2[tt::kR * kLS];
  __shared__ float dz1[tt::kR * kLS];
  __shared__ float red[4][kH];  // the upper row half's partial sums
  const PolicyLayout PL{kF0, kH, kH};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x;
  const int fi = tid & (kH - 1), half = tid >> 7;
  float *__restrict__ slab = a.slab + (size_t)tile * a.slab_stride;

  // the loads nothing of this launch feeds, issued first so that their latency
  // runs beside the part sums': dH1's W2 fragments (features i = 16 (2 w + it)
  // + n, K = o) and this thread's H2 column (output fi, its rows)
  float bw[2][8][4];
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int kg = 0; kg < 8; ++kg)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        bw[it][kg][s] = P[PL.oW2() + (16 * kg + 4 * kk + s) * kH + 16 * (2 * w + it) + n];
  float h2v[tt::kR / 2];
#pragma unroll
  for (int j = 0; j < tt::kR / 2; ++j)
    h2v[j] = a.h2[((size_t)tile * tt::kR + 2 * j + half) * kH + fi];

  // ---- G of the tile's entries
  stage_rows(tr, tile);
  for (int idx = tid; idx < tt::kSlices * tt::kR; idx += kThreads) {
    const int r = idx % tt::kR, k = idx / tt::kR;
    const int e = tt::row_entry(tile, r);
    sc[k][r] = e >= 0 ? tt::part_slice_sum(a.part, a.nparts, e, k) : 0.0;
  }
  __syncthreads();
  if (tid < tt::kR) {
    const int e = tr.entry[tid];
    const float g = e >= 0 ? tt::part_total(&sc[0][tid], tt::kR) : 0.0f;
    gs[tid] = g;
    if (e >= 0) a.G[e] = g;
  }
  layer1(P, a.env, tr, h1s);
  __syncthreads();

  // ---- dz2 = G (x) w3 o [H2 > 0]; dW3, db2 (output o = fi, the lane halves'
  // rows summed half 0 first), db3
  {
    const float w3 = P[PL.ow3() + fi];
    float dw3 = 0.0f, db2 = 0.0f;
#pragma unroll
    for (int r = half; r < tt::kR; r += 2) {
      const float h = h2v[r >> 1];
      const float g = gs[r];
      const float d = h > 0.0f ? g * w3 : 0.0f;
      dz2[r * kLS + fi] = d;
      dw3 = fmaf(g, h, dw3);
      db2 += d;
    }
    if (half) {
      red[0][fi] = dw3;
      red[1][fi] = db2;
    }
    __syncthreads();
    if (!half) {
      slab[PL.ow3() + fi] = dw3 + red[0][fi];
      slab[PL.ob2() + fi] = db2 + red[1][fi];
    }
    if (tid == 0) {
      float s = 0.0f;
      for (int r = 0; r < tt::kR; ++r) s += gs[r];
      slab[PL.ob3()] = s;
    }
  }

  // ---- dH1 = dz2 W2 o [H1 > 0] -> dz1: features i = 16 (2 w + it) + n, K = o
  {
    v4f acc[2][kRT];
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) acc[it][rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
      v4f ad[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
        ad[rt] = *reinterpret_cast<const v4f *>(dz2 + (16 * rt + n) * kLS + 16 * kg + 4 * kk);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt)
            acc[it][rt] = mfma16(ad[rt][s], bw[it][kg][s], acc[it][rt]);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int o = (16 * rt + 4 * kk + j) * kLS + 16 * (2 * w + it) + n;
          dz1[o] = h1s[o] > 0.0f ? acc[it][rt][j] : 0.0f;
        }
  }

  // ---- dW2 = dz2^T H1: outputs o = 16 (2 w + ot) + m, K = the tile's rows
  // (row 4 s + l >> 4 in step s)
#pragma unroll
  for (int ot = 0; ot < 2; ++ot) {
    float ad[tt::kR / 4];
#pragma unroll
    for (int s = 0; s < tt::kR / 4; ++s) ad[s] = dz2[(4 * s + kk) * kLS + 16 * (2 * w + ot) + n];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      v4f acc = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < tt::kR / 4; ++s)
        acc = mfma16(ad[s], h1s[(4 * s + kk) * kLS + 16 * it + n], acc);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        slab[PL.oW2() + (16 * (2 * w + ot) + 4 * kk + j) * kH + 16 * it + n] = acc[j];
    }
  }
  __syncthreads();

  // ---- dW1 / db1 / the item sums of feature fi
  {
    float w0 = 0.0f, w1 = 0.0f, sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int r = half; r < tt::kR; r += 2) {
      const float d = dz1[r * kLS + fi];
      w0 = fmaf(d, tr.x0[r], w0);
      w1 = fmaf(d, tr.x1[r], w1);
      if (tr.item_a[r])
        sa += d;
      else
        sb += d;
    }
    if (half) {
      red[0][fi] = w0;
      red[1][fi] = w1;
      red[2][fi] = sa;
      red[3][fi] = sb;
    }
    __syncthreads();
    if (!half) {
      w0 += red[0][fi];
      w1 += red[1][fi];
      const float va = sa + red[2][fi], vb = sb + red[3][fi];
      slab[PL.oW1() + fi * kF0 + 0] = w0;
      slab[PL.oW1() + fi * kF0 + 1] = w1;
#pragma unroll
      for (int d = 0; d < kD; ++d)
        slab[PL.oW1() + fi * kF0 + kD + d] =
            va * ((float)a.env.item_a[d] / (float)kCapacity) +
            vb * ((float)a.env.item_b[d] / (float)kCapacity);
      slab[PL.ob1() + fi] = va + vb;
    }
  }
}

}  // namespace tm

hipError_t launch_table_fwd(const TableFwdArgs &a, hipStream_t s) {
  if (!a.params || !a.logits || !a.h2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tm::table_fwd_kernel, dim3(tt::kTiles), dim3(tm::kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_table_bwd(const TableBwdArgs &a, hipStream_t s) {
  const PolicyLayout PL{tm::kF0, tm::kH, tm::kH};
  if (!a.params || !a.h2 || !a.part || !a.G || !a.slab || a.nparts < 1 ||
      a.slab_stride < PL.size())
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tm::table_bwd_kernel, dim3(tt::kTiles), dim3(tm::kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace xh
