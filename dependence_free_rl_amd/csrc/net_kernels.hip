// net_kernels.hip -- the per-bin policy net of a venv learner (xh_net,
// net_api.cpp; DESIGN.md §3.2, "the device-resident nets"): the conv1d_1 chain
// F0 = 2D -> H1 -> relu -> H2 -> relu -> 1 over the flat per-bin rows
// R = rows * B of an observation block [rows][B][2D], forward and parameter
// gradient, fused so that no activation leaves the workgroup.
//
//   net_policy_fwd_kernel<F0, H1, H2>  tiles of 64 flat rows per workgroup of
//       four waves, persistent grid.  Layer 1 is an f32 fmaf chain into LDS,
//       layer 2 runs on v_mfma_f32_16x16x4_f32 with the W2 fragments held in
//       registers for all of the workgroup's tiles, then relu, the w3 dot and
//       + b3.  Writes the logits and nothing else.
//   net_policy_bwd_kernel<F0, H1, H2>  from obs and dout it recomputes H1 and
//       the layer-2 pre-activation with the forward's code (the same bits);
//       dz2 = g w3 o [z2 > 0]; dW2 = dz2^T H1 and dH1 = dz2 W2 o [H1 > 0] on the
//       MFMA; dW1, db1, db2, dW3, db3 on the VALU.  Every sum runs over all of
//       the workgroup's tiles in registers; one slab in PolicyLayout per
//       workgroup, summed in fixed order by launch_slab_reduce.  No
//       floating-point atomics.
// MFMA operand maps and the float4-per-four-K-steps layout are those of
// table_mm_kernels.hip (16x16x4, lane l: A[m = l & 15][k = l >> 4], B[k = l >>
// 4][n = l & 15], D register j: [m = 4 (l >> 4) + j][n = l & 15]); the LDS row
// stride is the width + 16 floats (144 at 128).
// Tail rows (past R in the last tile) are computed on row R - 1 with g = 0:
// every product they enter is an exact zero, and they store no logit.
#include "xh_device.h"
#include "xh_kernels.h"

namespace xh {
namespace pn {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 64, kRT = kTile / 16;

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }

// How the four waves share a tile's products.
template <int H1_, int H2_>
struct Shape {
  static constexpr int H1 = H1_, H2 = H2_;
  static constexpr int LS1 = H1 + 16, LS2 = H2 + 16;  // LDS row strides
  static constexpr int KG1 = H1 / 16, KG2 = H2 / 16;  // K groups of 16
  // layer 2: the H2 / 16 output tiles over WO waves, the 4 row tiles over WR
  static constexpr int WO = KG2 < kWaves ? KG2 : kWaves, WR = kWaves / WO;
  static constexpr int OT = KG2 / WO, RTW = kRT / WR;
  // layer 1 / dW1: feature tid % H1, rows tid / H1, + G1, ...
  static constexpr int G1 = kThreads / H1;
  // dW2: the KG2 x KG1 tiles of 16 x 16, NP consecutive ones per wave
  static constexpr int NP = KG2 * KG1 / kWaves;
  static constexpr int NPI = NP < KG1 ? NP : KG1, NPO = NP / NPI;
  // dH1: the KG1 feature tiles over the waves, all row tiles each
  static constexpr int IT = KG1 / kWaves;
  static_assert(H1 % 64 == 0 && H2 % 32 == 0 && H1 <= 128 && H2 <= H1, "widths");
};

// the tile's inputs -> xs[row][F0] (rows past R: row R - 1) and, with dout,
// its loss gradients -> gs[row] (rows past R: 0)
template <int F0>
__device__ __forceinline__ void stage_rows(const float *__restrict__ obs, long R, long tile,
                                           const float *__restrict__ dout, float *xs, float *gs) {
  for (int idx = threadIdx.x; idx < kTile * F0; idx += kThreads) {
    const int r = idx / F0, k = idx - r * F0;
    long row = tile * kTile + r;
    if (row >= R) row = R - 1;
    xs[idx] = obs[row * F0 + k];
  }
  if (dout && threadIdx.x < kTile) {
    const long row = tile * kTile + threadIdx.x;
    gs[threadIdx.x] = row < R ? dout[row] : 0.0f;
  }
}

// H1 of the tile -> h1s[row][i]: x0 w0 + x1 w1 + ... as one fmaf chain from
// zero, then + b1: the order of the Dense GEMM's K loop and bias epilogue
// (dense_kernels.hip), so that H1 is the layer launches' bit for bit
template <int F0, class S>
__device__ __forceinline__ void layer1(const float (&w1)[F0], float b1, const float *xs,
                                       float *h1s) {
  const int fi = threadIdx.x & (S::H1 - 1), g = threadIdx.x / S::H1;
#pragma unroll 4
  for (int r = g; r < kTile; r += S::G1) {
    float h = 0.0f;
#pragma unroll
    for (int k = 0; k < F0; ++k) h = fmaf(xs[r * F0 + k], w1[k], h);
    h1s[r * S::LS1 + fi] = relu(h + b1);
  }
}

// this wave's W2 fragments: outputs o = 16 (ot0 + ot) + n, K group kg
template <class S>
__device__ __forceinline__ void load_w2(const float *__restrict__ W2, int ot0, int n, int kk,
                                        v4f (&bw)[S::OT][S::KG1]) {
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot)
#pragma unroll
    for (int kg = 0; kg < S::KG1; ++kg)
      bw[ot][kg] = *reinterpret_cast<const v4f *>(W2 + (16 * (ot0 + ot) + n) * S::H1 + 16 * kg +
                                                  4 * kk);
}

// layer 2 without its bias: acc[ot][rt] register j = row 16 (rt0 + rt) + 4 kk +
// j, output 16 (ot0 + ot) + n; K ascending from a zero accumulator
template <class S>
__device__ __forceinline__ void layer2(const float *h1s, const v4f (&bw)[S::OT][S::KG1], int rt0,
                                       int n, int kk, v4f (&acc)[S::OT][S::RTW]) {
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot)
#pragma unroll
    for (int rt = 0; rt < S::RTW; ++rt) acc[ot][rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int kg = 0; kg < S::KG1; ++kg) {
    v4f ah[S::RTW];
#pragma unroll
    for (int rt = 0; rt < S::RTW; ++rt)
      ah[rt] = *reinterpret_cast<const v4f *>(h1s + (16 * (rt0 + rt) + n) * S::LS1 + 16 * kg +
                                              4 * kk);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int ot = 0; ot < S::OT; ++ot)
#pragma unroll
        for (int rt = 0; rt < S::RTW; ++rt)
          acc[ot][rt] = mfma16(ah[rt][s], bw[ot][kg][s], acc[ot][rt]);
  }
}

template <int F0, int H1, int H2>
__global__ __launch_bounds__(kThreads) void net_policy_fwd_kernel(NetPolicyArgs a) {
  using S = Shape<H1, H2>;
  __shared__ float xs[kTile * F0];
  __shared__ __attribute__((aligned(16))) float h1s[kTile * S::LS1];
  __shared__ float zp[S::WO][kTile];
  const PolicyLayout PL{F0, H1, H2};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ot0 = (w % S::WO) * S::OT, rt0 = (w / S::WO) * S::RTW;
  const long tiles = (a.R + kTile - 1) / kTile;

  // what every tile of this workgroup uses, held in registers
  v4f bw[S::OT][S::KG1];
  load_w2<S>(P + PL.oW2(), ot0, n, kk, bw);
  float w1[F0];
  const int fi = tid & (H1 - 1);
#pragma unroll
  for (int k = 0; k < F0; ++k) w1[k] = P[PL.oW1() + fi * F0 + k];
  const float b1 = P[PL.ob1() + fi];
  float b2v[S::OT], w3v[S::OT];
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot) {
    b2v[ot] = P[PL.ob2() + 16 * (ot0 + ot) + n];
    w3v[ot] = P[PL.ow3() + 16 * (ot0 + ot) + n];
  }
  const float b3 = P[PL.ob3()];

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_rows<F0>(a.obs, a.R, tile, nullptr, xs, nullptr);
    __syncthreads();
    layer1<F0, S>(w1, b1, xs, h1s);
    __syncthreads();
    v4f acc[S::OT][S::RTW];
    layer2<S>(h1s, bw, rt0, n, kk, acc);
#pragma unroll
    for (int rt = 0; rt < S::RTW; ++rt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = 0.0f;
#pragma unroll
        for (int ot = 0; ot < S::OT; ++ot) z = fmaf(relu(acc[ot][rt][j] + b2v[ot]), w3v[ot], z);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) z += __shfl_xor(z, o, kWave);
        if (n == 0) zp[w % S::WO][16 * (rt0 + rt) + 4 * kk + j] = z;
      }
    __syncthreads();
    if (tid < kTile && tile * kTile + tid < a.R) {
      float z;
      if constexpr (S::WO == 4)
        z = (zp[0][tid] + zp[1][tid]) + (zp[2][tid] + zp[3][tid]);
      else
        z = zp[0][tid] + zp[1][tid];
      a.logits[tile * kTile + tid] = z + b3;
    }
  }
}

template <int F0, int H1, int H2>
__global__ __launch_bounds__(kThreads) void net_policy_bwd_kernel(NetPolicyArgs a) {
  using S = Shape<H1, H2>;
  __shared__ float xs[kTile * F0];
  __shared__ float gs[kTile];
  // h1s: H1, then dz1 in place; after the last tile the dW3 / db2 partials
  __shared__ __attribute__((aligned(16))) float h1s[kTile * S::LS1];
  // dz2; after the last tile the dW1 / db1 partials
  __shared__ __attribute__((aligned(16))) float dz2s[kTile * S::LS2];
  static_assert(2 * 4 * S::WR * H2 <= kTile * S::LS1, "dW3 / db2 partials fit h1s");
  static_assert(S::G1 * H1 * (F0 + 1) <= kTile * S::LS2, "dW1 / db1 partials fit dz2s");
  const PolicyLayout PL{F0, H1, H2};
  const float *__restrict__ P = a.params;
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kk = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ot0 = (w % S::WO) * S::OT, rt0 = (w / S::WO) * S::RTW;
  const int fi = tid & (H1 - 1), grp = tid / H1;
  // dW2: this wave's tiles p = NP w + NPI qo + qi -> output tile p / KG1,
  // feature tile p % KG1
  const int p0 = S::NP * w;
  const long tiles = (a.R + kTile - 1) / kTile;
  float *__restrict__ slab = a.slab + (size_t)blockIdx.x * a.slab_stride;

  v4f bw[S::OT][S::KG1];
  load_w2<S>(P + PL.oW2(), ot0, n, kk, bw);
  float w1[F0];
#pragma unroll
  for (int k = 0; k < F0; ++k) w1[k] = P[PL.oW1() + fi * F0 + k];
  const float b1 = P[PL.ob1() + fi];
  float b2v[S::OT], w3v[S::OT];
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot) {
    b2v[ot] = P[PL.ob2() + 16 * (ot0 + ot) + n];
    w3v[ot] = P[PL.ow3() + 16 * (ot0 + ot) + n];
  }

  // the sums over this workgroup's tiles
  v4f dw2[S::NPO][S::NPI];
#pragma unroll
  for (int qo = 0; qo < S::NPO; ++qo)
#pragma unroll
    for (int qi = 0; qi < S::NPI; ++qi) dw2[qo][qi] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  float dw3[S::OT], db2[S::OT], dw1[F0], db1 = 0.0f, db3 = 0.0f;
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot) dw3[ot] = db2[ot] = 0.0f;
#pragma unroll
  for (int k = 0; k < F0; ++k) dw1[k] = 0.0f;

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_rows<F0>(a.obs, a.R, tile, a.dout, xs, gs);
    __syncthreads();
    layer1<F0, S>(w1, b1, xs, h1s);
    __syncthreads();

    // ---- layer 2 again; dz2 = g w3 o [z2 > 0] -> dz2s; dW3, db2, db3
    {
      v4f acc[S::OT][S::RTW];
      layer2<S>(h1s, bw, rt0, n, kk, acc);
#pragma unroll
      for (int rt = 0; rt < S::RTW; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 16 * (rt0 + rt) + 4 * kk + j;
          const float g = gs[r];
#pragma unroll
          for (int ot = 0; ot < S::OT; ++ot) {
            const float z = acc[ot][rt][j] + b2v[ot];
            const float d = z > 0.0f ? g * w3v[ot] : 0.0f;
            dz2s[r * S::LS2 + 16 * (ot0 + ot) + n] = d;
            dw3[ot] = fmaf(g, relu(z), dw3[ot]);
            db2[ot] += d;
          }
        }
      if (w == 0) {
        float v = gs[lane];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
        db3 += v;
      }
    }
    __syncthreads();

    // ---- dW2 += dz2^T H1: K = the tile's rows (row 4 s + kk in step s)
#pragma unroll
    for (int qo = 0; qo < S::NPO; ++qo) {
      const int ot = (p0 + S::NPI * qo) / S::KG1, itb = (p0 + S::NPI * qo) % S::KG1;
      float ad[kTile / 4];
#pragma unroll
      for (int s = 0; s < kTile / 4; ++s) ad[s] = dz2s[(4 * s + kk) * S::LS2 + 16 * ot + n];
#pragma unroll
      for (int qi = 0; qi < S::NPI; ++qi)
#pragma unroll
        for (int s = 0; s < kTile / 4; ++s)
          dw2[qo][qi] =
              mfma16(ad[s], h1s[(4 * s + kk) * S::LS1 + 16 * (itb + qi) + n], dw2[qo][qi]);
    }

    // ---- dH1 = dz2 W2 o [H1 > 0] -> h1s in place.  Its W2 fragments
    // (features i = 16 (IT w + it) + n, K = o) come from L2 per tile: held
    // beside the forward's and dW2's accumulators they would spill
    {
      float bt[S::IT][S::KG2][4];
#pragma unroll
      for (int it = 0; it < S::IT; ++it)
#pragma unroll
        for (int kg = 0; kg < S::KG2; ++kg)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            bt[it][kg][s] = P[PL.oW2() + (16 * kg + 4 * kk + s) * H1 + 16 * (S::IT * w + it) + n];
      v4f acc[S::IT][kRT];
#pragma unroll
      for (int it = 0; it < S::IT; ++it)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[it][rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kg = 0; kg < S::KG2; ++kg) {
        v4f ad[kRT];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
          ad[rt] =
              *reinterpret_cast<const v4f *>(dz2s + (16 * rt + n) * S::LS2 + 16 * kg + 4 * kk);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int it = 0; it < S::IT; ++it)
#pragma unroll
            for (int rt = 0; rt < kRT; ++rt)
              acc[it][rt] = mfma16(ad[rt][s], bt[it][kg][s], acc[it][rt]);
      }
      __syncthreads();  // dW2 has read H1
#pragma unroll
      for (int it = 0; it < S::IT; ++it)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int o = (16 * rt + 4 * kk + j) * S::LS1 + 16 * (S::IT * w + it) + n;
            h1s[o] = h1s[o] > 0.0f ? acc[it][rt][j] : 0.0f;
          }
    }
    __syncthreads();

    // ---- dW1, db1 of feature fi over rows grp, grp + G1, ...
#pragma unroll 4
    for (int r = grp; r < kTile; r += S::G1) {
      const float d = h1s[r * S::LS1 + fi];
#pragma unroll
      for (int k = 0; k < F0; ++k) dw1[k] = fmaf(d, xs[r * F0 + k], dw1[k]);
      db1 += d;
    }
    __syncthreads();
  }

  // ---- the slab: dW2 from the accumulators, the rest through LDS partials
  // summed in a fixed order
#pragma unroll
  for (int qo = 0; qo < S::NPO; ++qo) {
    const int ot = (p0 + S::NPI * qo) / S::KG1, itb = (p0 + S::NPI * qo) % S::KG1;
#pragma unroll
    for (int qi = 0; qi < S::NPI; ++qi)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        slab[PL.oW2() + (16 * ot + 4 * kk + j) * H1 + 16 * (itb + qi) + n] = dw2[qo][qi][j];
  }
  constexpr int kP3 = 4 * S::WR;  // partials per output: kk x the row waves
  float *red3 = h1s, *red1 = dz2s;
#pragma unroll
  for (int ot = 0; ot < S::OT; ++ot) {
    const int col = 16 * (ot0 + ot) + n, p = 4 * (w / S::WO) + kk;
    red3[p * H2 + col] = dw3[ot];
    red3[(kP3 + p) * H2 + col] = db2[ot];
  }
#pragma unroll
  for (int k = 0; k < F0; ++k) red1[(grp * (F0 + 1) + k) * H1 + fi] = dw1[k];
  red1[(grp * (F0 + 1) + F0) * H1 + fi] = db1;
  __syncthreads();
  if (tid < H2) {
    float s3 = red3[tid], s2 = red3[kP3 * H2 + tid];
#pragma unroll
    for (int p = 1; p < kP3; ++p) {
      s3 += red3[p * H2 + tid];
      s2 += red3[(kP3 + p) * H2 + tid];
    }
    slab[PL.ow3() + tid] = s3;
    slab[PL.ob2() + tid] = s2;
  }
  if (tid < H1) {
#pragma unroll
    for (int k = 0; k <= F0; ++k) {
      float s = red1[k * H1 + tid];
#pragma unroll
      for (int g = 1; g < S::G1; ++g) s += red1[(g * (F0 + 1) + k) * H1 + tid];
      if (k < F0)
        slab[PL.oW1() + tid * F0 + k] = s;
      else
        slab[PL.ob1() + tid] = s;
    }
  }
  if (tid == 0) slab[PL.ob3()] = db3;
}

template <int F0, int H1, int H2>
hipError_t launch(const NetPolicyArgs &a, int grid, bool backward, hipStream_t s) {
  if (backward)
    hipLaunchKernelGGL((net_policy_bwd_kernel<F0, H1, H2>), dim3(grid), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((net_policy_fwd_kernel<F0, H1, H2>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

template <int F0>
hipError_t launch_f0(const NetPolicyArgs &a, int grid, bool backward, hipStream_t s) {
  if (a.H1 == 128 && a.H2 == 128) return launch<F0, 128, 128>(a, grid, backward, s);
  if (a.H1 == 128 && a.H2 == 64) return launch<F0, 128, 64>(a, grid, backward, s);
  if (a.H1 == 64 && a.H2 == 64) return launch<F0, 64, 64>(a, grid, backward, s);
  if (a.H1 == 64 && a.H2 == 32) return launch<F0, 64, 32>(a, grid, backward, s);
  return hipErrorInvalidValue;
}

hipError_t launch_any(const NetPolicyArgs &a, int grid, bool backward, hipStream_t s) {
  const long tiles = (a.R + kTile - 1) / kTile;
  if (!a.params || !a.obs || a.R < 1 || grid < 1 || grid > tiles) return hipErrorInvalidValue;
  switch (a.F0) {
    case 2: return launch_f0<2>(a, grid, backward, s);
    case 4: return launch_f0<4>(a, grid, backward, s);
    case 6: return launch_f0<6>(a, grid, backward, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace pn

bool net_policy_shape_supported(int F0, int H1, int H2) {
  return (F0 == 2 || F0 == 4 || F0 == 6) &&
         ((H1 == 128 && (H2 == 128 || H2 == 64)) || (H1 == 64 && (H2 == 64 || H2 == 32)));
}

long net_policy_tiles(long R) { return (R + pn::kTile - 1) / pn::kTile; }

int net_policy_lds_bytes(int F0, int H1, int H2, int backward) {
  const int h1 = pn::kTile * (H1 + 16), x = pn::kTile * F0;
  if (backward) return 4 * (x + pn::kTile + h1 + pn::kTile * (H2 + 16));
  return 4 * (x + h1 + (H2 / 16 < 4 ? H2 / 16 : 4) * pn::kTile);
}

hipError_t launch_net_policy_fwd(const NetPolicyArgs &a, int grid, hipStream_t s) {
  if (!a.logits) return hipErrorInvalidValue;
  return pn::launch_any(a, grid, false, s);
}

hipError_t launch_net_policy_bwd(const NetPolicyArgs &a, int grid, hipStream_t s) {
  const PolicyLayout PL{a.F0, a.H1, a.H2};
  if (!a.dout || !a.slab || a.slab_stride < PL.size()) return hipErrorInvalidValue;
  return pn::launch_any(a, grid, true, s);
}

}  // namespace xh
