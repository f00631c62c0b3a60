// net_value_kernels.hip -- the value net of a venv learner read straight from
// the venv's recorded window (xh_net_forward_record / xh_net_backward_record,
// net_api.cpp; DESIGN.md §3.2, "the value net on the record"): the full-layer
// MLP Fin = 2BD -> 64 -> relu -> 32 -> relu -> 1, forward and parameter
// gradient, fused so that neither the f32 observation nor any activation
// leaves the workgroup.
//
//   net_value_fwd_kernel<B, D>  tiles of 64 rows per workgroup of four waves,
//       persistent grid.  A row is addressed as venv_record_obs_kernel
//       addresses it (index list, slot P = the present state, NEXT's done and
//       action bytes, the terminal view's subtraction).  Layer 0 is a 64 x Fin
//       by Fin x 64 product on v_mfma_f32_16x16x4_f32: K runs in chunks of KC
//       features; a chunk of the tile's observations is made in LDS from the
//       int8 words of the record ((float)v / (float)cap[d], the division
//       record_obs does), the W0 fragments of the chunk come from L2 (wave w
//       owns outputs 16 w .. 16 w + 15, so every W0 entry is read once per
//       tile).  The item half of a row's observation is the same D numbers in
//       every bin: its columns are written once per tile, the chunks rewrite
//       the bin columns only.  Layers 1 and 2 as net_kernels.hip's layer 2 and
//       epilogue.  Writes the values and nothing else.
//   net_value_bwd_kernel<B, D>  recomputes the forward with the same functions
//       (the relu masks are the forward's bits); dz2 = g w2 o [z2 > 0]; dW1 =
//       dz2^T H1 and dz1 = dz2 W1 o [H1 > 0] on the MFMA; then a second pass
//       over the chunks for dW0 = dz1^T X, wave w holding rows 16 w .. 16 w +
//       15 of dW0 in Fin / 4 accumulator registers per lane over all of the
//       workgroup's tiles.  One slab in ValueLayout per workgroup, summed in
//       fixed order by launch_slab_reduce.  No floating-point atomics.  Layer
//       0 gets no data gradient.
// MFMA operand maps and the float4-per-four-K-steps layout are those of
// net_kernels.hip / table_mm_kernels.hip (16x16x4, lane l: A[m = l & 15][k = l
// >> 4], B[k = l >> 4][n = l & 15], D register j: [m = 4 (l >> 4) + j][n = l &
// 15]); LDS row strides are the width + 16 floats.
// Tail rows (past count in the last tile) are computed on row count - 1, rows
// whose index is outside the view on row 0 of the view, both with g = 0: every
// product they enter is an exact zero, and they store no value.
#include "xh_device.h"
#include "xh_kernels.h"

namespace xh {
namespace vn {

constexpr int kThreads = 256;
constexpr int kTile = 64, kRT = kTile / 16;
constexpr int kV1 = kNetValueV1, kV2 = kNetValueV2;
constexpr int kLS1 = kV1 + 16, kLS2 = kV2 + 16;  // LDS row strides of H1, dz2
constexpr int kXS = 64 + 16;                     // ... of a chunk of X

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }

// Layer 0's K dimension: Fin features in NCH chunks of KC = CB bins.  A row's
// bytes of a chunk are UPC units of U 32-bit words; a unit holds whole bins
// (4 at 1-D and 3-D, 2 at 2-D), so byte i of a unit is dim i % D of bin i / D
// at compile time.
template <int B_, int D_>
struct Shape {
  static constexpr int B = B_, D = D_, BD = B * D, Fin = 2 * BD;
  static constexpr int KC = D == 3 ? 48 : (Fin < 64 ? Fin : 64);
  static constexpr int NCH = Fin / KC, KG = KC / 16;
  static constexpr int CB = KC / (2 * D);
  static constexpr int U = D == 3 ? 3 : 1, UB = 4 * U / D;  // words, bins per unit
  static constexpr int UPC = CB / UB;
  static_assert(Fin % KC == 0 && KC % 16 == 0 && CB % UB == 0 && KC <= 64, "chunks");
};

// What the tile's rows are, per row in LDS (thread r < 64 fills row r).
struct Meta {
  const int8_t *rowp[kTile];  // the source state's B D bytes
  unsigned itw[kTile];        // its item word
  int sub[kTile];             // E_t: the bin reduced by the item, or -1
  float itq[kTile][4];        // item[d] / cap[d]
  float g[kTile];             // backward: dout, 0 for rows that do not count
  int live[kTile];            // the row is in range and its index in the view
};

// venv_record_obs_kernel's row addressing.  Rows past count: row count - 1;
// an index outside the view: row 0 and the venv's error bit 4.
template <int BD>
__device__ __forceinline__ void stage_meta(const NetValueArgs &a, long tile, Meta &m) {
  const int t = threadIdx.x;
  if (t >= kTile) return;
  const VenvObsArgs &r = a.rec;
  const long j = tile * kTile + t;
  const bool in_range = j < r.count;
  const long jc = in_range ? j : r.count - 1;
  const long total = (long)(r.next ? r.P : r.P + 1) * r.N;
  const long qr = r.rows ? (long)r.rows[r.first + jc] : r.first + jc;
  const bool valid = qr >= 0 && qr < total;
  const long q = valid ? qr : 0;
  int done = 0, act = 0;
  if (r.next) {
    done = r.rec_done[q] != 0;
    act = r.rec_action[q];
  }
  const long sq = r.next && !done ? q + r.N : q;  // source row s N + e
  const bool present = sq >= (long)r.P * r.N;
  const long so = present ? sq - (long)r.P * r.N : sq;
  m.rowp[t] = (present ? r.cur_bins : r.rec_bins) + (size_t)so * BD;
  const int8_t *ip = (present ? r.cur_items : r.rec_items) + (size_t)so * 4;
  const unsigned itw = *reinterpret_cast<const unsigned *>(ip);
  if (in_range && !valid) atomicOr(r.err, 4);
  const bool live = in_range && valid;
  m.itw[t] = itw;
  m.sub[t] = done ? act : -1;
#pragma unroll
  for (int d = 0; d < 4; ++d)
    m.itq[t][d] = (float)(int)(signed char)((itw >> (8 * d)) & 0xff) / (float)a.cap[d];
  m.live[t] = live;
  m.g[t] = a.dout && live ? a.dout[j] : 0.0f;
}

// the item columns of every bin of a chunk: the same for all of a tile's chunks
template <class S>
__device__ __forceinline__ void fill_items(const Meta &m, float *xs) {
  constexpr int D = S::D, PER = S::CB * D;
  for (int idx = threadIdx.x; idx < kTile * PER; idx += kThreads) {
    const int r = idx / PER, rem = idx - r * PER;
    const int bl = rem / D, d = rem - bl * D;
    xs[r * kXS + bl * 2 * D + D + d] = m.itq[r][d];
  }
}

// the bin columns of chunk c -> xs[row][(bin - c CB) 2D + d]
template <class S>
__device__ __forceinline__ void stage_chunk(const NetValueArgs &a, const Meta &m, int c,
                                            float *xs) {
  constexpr int D = S::D;
  const float capf[3] = {(float)a.cap[0], (float)a.cap[1], (float)a.cap[2]};
  for (int idx = threadIdx.x; idx < kTile * S::UPC; idx += kThreads) {
    const int r = idx / S::UPC, u = idx - r * S::UPC;
    const uint32_t *wp = reinterpret_cast<const uint32_t *>(m.rowp[r]) +
                         (c * S::UPC + u) * S::U;
    uint32_t wv[S::U];
#pragma unroll
    for (int i = 0; i < S::U; ++i) wv[i] = wp[i];
    const unsigned itw = m.itw[r];
    const int subl = m.sub[r] - (c * S::CB + u * S::UB);  // within the unit
    float *xr = xs + r * kXS + u * S::UB * 2 * D;
#pragma unroll
    for (int i = 0; i < 4 * S::U; ++i) {
      const int bl = i / D, d = i % D;
      int v = (int)(signed char)((wv[i >> 2] >> (8 * (i & 3))) & 0xff);
      const int item = (int)(signed char)((itw >> (8 * d)) & 0xff);
      v = bl == subl ? v - item : v;
      xr[bl * 2 * D + d] = (float)v / capf[d];
    }
  }
}

// Layer 0 without its bias: acc[rt] register j = row 16 rt + 4 kk + j, output
// 16 w + n; K ascending by chunks from a zero accumulator.  Ends behind a
// barrier: xs may be rewritten.
template <class S>
__device__ __forceinline__ void layer0(const NetValueArgs &a, const float *__restrict__ W0,
                                       const Meta &m, float *xs, int w, int n, int kk,
                                       v4f (&acc)[kRT]) {
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt) acc[rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  const float *wrow = W0 + (size_t)(16 * w + n) * S::Fin + 4 * kk;
  for (int c = 0; c < S::NCH; ++c) {
    v4f bw[S::KG];  // in flight while the chunk is made
#pragma unroll
    for (int kg = 0; kg < S::KG; ++kg)
      bw[kg] = *reinterpret_cast<const v4f *>(wrow + c * S::KC + 16 * kg);
    stage_chunk<S>(a, m, c, xs);
    __syncthreads();
#pragma unroll
    for (int kg = 0; kg < S::KG; ++kg) {
      v4f ah[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
        ah[rt] = *reinterpret_cast<const v4f *>(xs + (16 * rt + n) * kXS + 16 * kg + 4 * kk);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[rt] = mfma16(ah[rt][s], bw[kg][s], acc[rt]);
    }
    __syncthreads();
  }
}

// H1 = relu(layer 0 + b0) -> h1s[row][feature]
__device__ __forceinline__ void store_h1(const v4f (&acc)[kRT], float b0, int w, int n, int kk,
                                         float *h1s) {
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      h1s[(16 * rt + 4 * kk + j) * kLS1 + 16 * w + n] = relu(acc[rt][j] + b0);
}

// Layer 1 (64 -> 32): wave w owns output tile w & 1 of row tiles 2 (w >> 1),
// 2 (w >> 1) + 1; its W1 fragments stay in registers for all tiles
__device__ __forceinline__ void load_w1(const float *__restrict__ W1, int ot, int n, int kk,
                                        v4f (&bw)[kV1 / 16]) {
#pragma unroll
  for (int kg = 0; kg < kV1 / 16; ++kg)
    bw[kg] = *reinterpret_cast<const v4f *>(W1 + (16 * ot + n) * kV1 + 16 * kg + 4 * kk);
}
// without its bias: acc[rt] register j = row 16 (rt0 + rt) + 4 kk + j
__device__ __forceinline__ void layer1(const float *h1s, const v4f (&bw)[kV1 / 16], int rt0,
                                       int n, int kk, v4f (&acc)[2]) {
  acc[0] = acc[1] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int kg = 0; kg < kV1 / 16; ++kg) {
    v4f ah[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      ah[rt] = *reinterpret_cast<const v4f *>(h1s + (16 * (rt0 + rt) + n) * kLS1 + 16 * kg +
                                              4 * kk);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) acc[rt] = mfma16(ah[rt][s], bw[kg][s], acc[rt]);
  }
}

template <int B, int D>
__global__ __launch_bounds__(kThreads) void net_value_fwd_kernel(NetValueArgs a) {
  using S = Shape<B, D>;
  __shared__ __attribute__((aligned(16))) float xs[kTile * kXS];
  __shared__ __attribute__((aligned(16))) float h1s[kTile * kLS1];
  __shared__ float zp[2][kTile];
  __shared__ Meta m;
  const ValueLayout VL{S::Fin, kV1, kV2};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ot = w & 1, rt0 = 2 * (w >> 1);
  const long tiles = (a.rec.count + kTile - 1) / kTile;

  v4f bw1[kV1 / 16];
  load_w1(P + VL.oW2(), ot, n, kk, bw1);
  const float b0 = P[VL.ob1() + 16 * w + n];
  const float b1 = P[VL.ob2() + 16 * ot + n], w2 = P[VL.ow3() + 16 * ot + n];
  const float b2 = P[VL.ob3()];

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_meta<S::BD>(a, tile, m);
    __syncthreads();
    fill_items<S>(m, xs);
    v4f acc[kRT];
    layer0<S>(a, P + VL.oW1(), m, xs, w, n, kk, acc);
    store_h1(acc, b0, w, n, kk, h1s);
    __syncthreads();
    v4f z2[2];
    layer1(h1s, bw1, rt0, n, kk, z2);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = relu(z2[rt][j] + b1) * w2;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) z += __shfl_xor(z, o, kWave);
        if (n == 0) zp[ot][16 * (rt0 + rt) + 4 * kk + j] = z;
      }
    __syncthreads();
    if (tid < kTile && m.live[tid]) a.out[tile * kTile + tid] = (zp[0][tid] + zp[1][tid]) + b2;
  }
}

template <int B, int D>
__global__ __launch_bounds__(kThreads) void net_value_bwd_kernel(NetValueArgs a) {
  using S = Shape<B, D>;
  __shared__ __attribute__((aligned(16))) float xs[kTile * kXS];
  // h1s: H1, then dz1 in place; after the last tile the dw2 / db1 partials
  __shared__ __attribute__((aligned(16))) float h1s[kTile * kLS1];
  // dz2; after the last tile the db0 partials
  __shared__ __attribute__((aligned(16))) float dz2s[kTile * kLS2];
  __shared__ Meta m;
  static_assert(2 * 8 * kV2 <= kTile * kLS1, "dw2 / db1 partials fit h1s");
  static_assert(4 * kV1 <= kTile * kLS2, "db0 partials fit dz2s");
  const ValueLayout VL{S::Fin, kV1, kV2};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ot = w & 1, rt0 = 2 * (w >> 1);
  // dW1: this wave's two 16 x 16 tiles: output tile w >> 1, feature tiles
  // 2 (w & 1), 2 (w & 1) + 1
  const int ot1 = w >> 1, it1 = 2 * (w & 1);
  const long tiles = (a.rec.count + kTile - 1) / kTile;
  float *__restrict__ slab = a.slab + (size_t)blockIdx.x * a.slab_stride;

  v4f bw1[kV1 / 16];
  load_w1(P + VL.oW2(), ot, n, kk, bw1);
  const float b0 = P[VL.ob1() + 16 * w + n];
  const float b1 = P[VL.ob2() + 16 * ot + n], w2 = P[VL.ow3() + 16 * ot + n];

  // the sums over this workgroup's tiles
  v4f dw0[S::NCH * S::KG];  // rows 16 w + 4 kk + j of dW0, features 16 t + n
#pragma unroll
  for (int t = 0; t < S::NCH * S::KG; ++t) dw0[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  v4f dw1[2] = {v4f{0.0f, 0.0f, 0.0f, 0.0f}, v4f{0.0f, 0.0f, 0.0f, 0.0f}};
  float dw2 = 0.0f, db1 = 0.0f, db0 = 0.0f, db2 = 0.0f;

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_meta<S::BD>(a, tile, m);
    __syncthreads();
    fill_items<S>(m, xs);
    {
      v4f acc[kRT];
      layer0<S>(a, P + VL.oW1(), m, xs, w, n, kk, acc);
      store_h1(acc, b0, w, n, kk, h1s);
    }
    __syncthreads();

    // ---- layer 1 again; dz2 = g w2 o [z2 > 0] -> dz2s; dw2, db1, db2
    {
      v4f z2[2];
      layer1(h1s, bw1, rt0, n, kk, z2);
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 16 * (rt0 + rt) + 4 * kk + j;
          const float g = m.g[r];
          const float z = z2[rt][j] + b1;
          const float d = z > 0.0f ? g * w2 : 0.0f;
          dz2s[r * kLS2 + 16 * ot + n] = d;
          dw2 = fmaf(g, relu(z), dw2);
          db1 += d;
        }
      if (w == 0) {
        float v = m.g[lane];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
        db2 += v;
      }
    }
    __syncthreads();

    // ---- dW1 += dz2^T H1: K = the tile's rows (row 4 s + kk in step s)
    {
      float ad[kTile / 4];
#pragma unroll
      for (int s = 0; s < kTile / 4; ++s) ad[s] = dz2s[(4 * s + kk) * kLS2 + 16 * ot1 + n];
#pragma unroll
      for (int qi = 0; qi < 2; ++qi)
#pragma unroll
        for (int s = 0; s < kTile / 4; ++s)
          dw1[qi] = mfma16(ad[s], h1s[(4 * s + kk) * kLS1 + 16 * (it1 + qi) + n], dw1[qi]);
    }

    // ---- dz1 = dz2 W1 o [H1 > 0] -> h1s in place: wave w owns features
    // 16 w + n of all row tiles; its W1 fragments (K = the 32 outputs) come
    // from L2 per tile
    {
      float bt[kV2 / 16][4];
#pragma unroll
      for (int kg = 0; kg < kV2 / 16; ++kg)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          bt[kg][s] = P[VL.oW2() + (16 * kg + 4 * kk + s) * kV1 + 16 * w + n];
      v4f acc[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) acc[rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kg = 0; kg < kV2 / 16; ++kg) {
        v4f ad[kRT];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
          ad[rt] = *reinterpret_cast<const v4f *>(dz2s + (16 * rt + n) * kLS2 + 16 * kg + 4 * kk);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt) acc[rt] = mfma16(ad[rt][s], bt[kg][s], acc[rt]);
      }
      __syncthreads();  // dW1 has read H1
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int o = (16 * rt + 4 * kk + j) * kLS1 + 16 * w + n;
          h1s[o] = h1s[o] > 0.0f ? acc[rt][j] : 0.0f;
        }
    }
    __syncthreads();

    // ---- db0 of feature lane over rows w, w + 4, ...; dW0 += dz1^T X over
    // the chunks again (K = the tile's rows)
    for (int r = w; r < kTile; r += 4) db0 += h1s[r * kLS1 + lane];
    {
      float ad[kTile / 4];
#pragma unroll
      for (int s = 0; s < kTile / 4; ++s) ad[s] = h1s[(4 * s + kk) * kLS1 + 16 * w + n];
#pragma unroll
      for (int c = 0; c < S::NCH; ++c) {
        stage_chunk<S>(a, m, c, xs);
        __syncthreads();
#pragma unroll
        for (int ft = 0; ft < S::KG; ++ft)
#pragma unroll
          for (int s = 0; s < kTile / 4; ++s)
            dw0[c * S::KG + ft] =
                mfma16(ad[s], xs[(4 * s + kk) * kXS + 16 * ft + n], dw0[c * S::KG + ft]);
        __syncthreads();
      }
    }
  }

  // ---- the slab: dW0 and dW1 from the accumulators, the rest through LDS
  // partials summed in a fixed order
#pragma unroll
  for (int t = 0; t < S::NCH * S::KG; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      slab[VL.oW1() + (size_t)(16 * w + 4 * kk + j) * S::Fin + 16 * t + n] = dw0[t][j];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      slab[VL.oW2() + (16 * ot1 + 4 * kk + j) * kV1 + 16 * (it1 + qi) + n] = dw1[qi][j];
  constexpr int kP = 8;  // partials per layer-1 output: kk x the two row waves
  float *red2 = h1s, *red0 = dz2s;
  {
    const int col = 16 * ot + n, p = 4 * (w >> 1) + kk;
    red2[p * kV2 + col] = dw2;
    red2[(kP + p) * kV2 + col] = db1;
  }
  red0[w * kV1 + lane] = db0;
  __syncthreads();
  if (tid < kV2) {
    float s2 = red2[tid], s1 = red2[kP * kV2 + tid];
#pragma unroll
    for (int p = 1; p < kP; ++p) {
      s2 += red2[p * kV2 + tid];
      s1 += red2[(kP + p) * kV2 + tid];
    }
    slab[VL.ow3() + tid] = s2;
    slab[VL.ob2() + tid] = s1;
  }
  if (tid < kV1)
    slab[VL.ob1() + tid] =
        (red0[tid] + red0[kV1 + tid]) + (red0[2 * kV1 + tid] + red0[3 * kV1 + tid]);
  if (tid == 0) slab[VL.ob3()] = db2;
}

template <int B, int D>
hipError_t launch(const NetValueArgs &a, int grid, bool backward, hipStream_t s) {
  if (backward)
    hipLaunchKernelGGL((net_value_bwd_kernel<B, D>), dim3(grid), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((net_value_fwd_kernel<B, D>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

template <int B>
hipError_t launch_b(const NetValueArgs &a, int grid, bool backward, hipStream_t s) {
  switch (a.rec.D) {
    case 1: return launch<B, 1>(a, grid, backward, s);
    case 2: return launch<B, 2>(a, grid, backward, s);
    case 3: return launch<B, 3>(a, grid, backward, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_any(const NetValueArgs &a, int grid, bool backward, hipStream_t s) {
  const VenvObsArgs &r = a.rec;
  const long tiles = (r.count + kTile - 1) / kTile;
  const long total = (long)(r.next ? r.P : r.P + 1) * r.N;
  if (!a.params || !r.cur_bins || !r.cur_items || !r.err || r.count < 1 || r.first < 0 ||
      total < 1 || grid < 1 || grid > tiles)
    return hipErrorInvalidValue;
  if (r.P > 0 && (!r.rec_bins || !r.rec_items)) return hipErrorInvalidValue;
  if (r.next && (!r.rec_action || !r.rec_done)) return hipErrorInvalidValue;
  if (!r.rows && r.first + r.count > total) return hipErrorInvalidValue;
  for (int d = 0; d < r.D; ++d)
    if (a.cap[d] < 1) return hipErrorInvalidValue;
  switch (r.B) {
    case 8: return launch_b<8>(a, grid, backward, s);
    case 16: return launch_b<16>(a, grid, backward, s);
    case 32: return launch_b<32>(a, grid, backward, s);
    case 64: return launch_b<64>(a, grid, backward, s);
    case 128: return launch_b<128>(a, grid, backward, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace vn

long net_value_tiles(long count) { return (count + vn::kTile - 1) / vn::kTile; }

int net_value_lds_bytes(int backward) {
  const int common = 4 * (vn::kTile * vn::kXS + vn::kTile * vn::kLS1) + (int)sizeof(vn::Meta);
  return common + 4 * (backward ? vn::kTile * vn::kLS2 : 2 * vn::kTile);
}

hipError_t launch_net_value_fwd(const NetValueArgs &a, int grid, hipStream_t s) {
  if (!a.out) return hipErrorInvalidValue;
  return vn::launch_any(a, grid, false, s);
}

hipError_t launch_net_value_bwd(const NetValueArgs &a, int grid, hipStream_t s) {
  const ValueLayout VL{a.rec.B * 2 * a.rec.D, vn::kV1, vn::kV2};
  if (!a.dout || !a.slab || a.slab_stride < VL.size()) return hipErrorInvalidValue;
  return vn::launch_any(a, grid, true, s);
}

}  // namespace xh
