// xh_roll_split.h -- what the split rollouts share across translation units
// (policy_kernels.hip: rollout_split_kernel; rollout_pack_kernels.hip: the
// packed table stepper): the policy shape, the raw row registers, the f16-pair
// staging and forward of the [128,128] / [64,64] shapes and the logit-table
// build of the 64-bin 2-D one.  Device code only.
#pragma once
#include "spec8_e0_layout.h"
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_logit_table.h"
#include "xh_split.h"

namespace xh {

template <int B_, int D_, int H1_, int H2_>
struct PShape {
  static constexpr int B = B_, D = D_, H1 = H1_, H2 = H2_;
  static constexpr int F0 = 2 * D;
  static constexpr int S1 = (F0 + 1) / 2;  // layer-1 MFMA k-steps
  static constexpr int NIT = H1 / 32, NOT = H2 / 32;
  static constexpr int G = B <= 64 ? 64 / B : 1;   // envs per group
  static constexpr int HG = B <= 64 ? 1 : B / 64;  // 64-row half-groups
  static constexpr int R = 64 * HG;                // rows per group
  static constexpr int BD = B * D;
  static constexpr int W2S = H1 + 4;           // LDS W2 image row stride
  static constexpr int HS = H1 + 1;            // LDS H1 image row stride
  static constexpr int AS = H2 + 1;            // LDS dA2 image row stride
  static constexpr int FJ = NOT >= 4 ? 2 : 1;  // fwd r-tiles per wave
  static constexpr int JW = (NOT * NIT + 3) / 4;  // dW2 tiles per wave
  static constexpr int JH = (2 * NIT + 3) / 4;    // dH1 r-tiles per wave
  // 4-wave train kernel: workgroups per CU it is compiled for.  The 1-D
  // [64,64] shape (config 2) fits 256 VGPRs without scratch, so two
  // workgroups share a CU and one's barrier / softmax phases overlap the
  // other's MFMAs; the wider shapes need the full register file (spills
  // measured at 2).
  static constexpr int TOCC = (H1 <= 64 && H2 <= 64 && D == 1) ? 2 : 1;
  static_assert(B == 8 || B == 16 || B == 32 || B == 64 || B == 128, "B");
  static_assert(NIT == 1 || NIT == 2 || NIT == 4, "H1 in {32,64,128}");
  static_assert(NOT == 1 || NOT == 2 || NOT == 4, "H2 in {32,64,128}");
  static_assert(D >= 1 && D <= 3, "D");
  // LDS carve (floats), every region 16-byte aligned.
  static constexpr int r4(int x) { return (x + 3) & ~3; }
  static constexpr int L_W2 = 0;
  static constexpr int L_W1 = L_W2 + H2 * W2S;
  static constexpr int L_B1 = L_W1 + r4(H1 * F0);
  static constexpr int L_B2 = L_B1 + H1;
  static constexpr int L_W3 = L_B2 + H2;
  static constexpr int L_B3 = L_W3 + H2;
  static constexpr int L_Z = L_B3 + 4;
  static constexpr int L_ROLLOUT_END = L_Z + NOT * R;
  static constexpr int L_H1 = L_ROLLOUT_END;
  static constexpr int L_DA2 = L_H1 + r4(64 * HS);
  static constexpr int L_TRAIN_END = L_DA2 + r4(64 * AS);
  // 8-wave kernel: transposed images [feature][row] (row stride 64+4 floats:
  // conflict-free ds_read_b128 along rows)
  static constexpr int TS = 68;
  static constexpr int L_H1T = L_ROLLOUT_END;
  static constexpr int L_DAT = L_H1T + H1 * TS;
  // the layer-1 biases with the item's contribution folded in, for the two
  // item-table entries (8-wave kernel, one env per group)
  static constexpr int L_B1F = L_DAT + H2 * TS;
  static constexpr int L_TRAIN8_END = L_B1F + 2 * H1;
  // end-of-kernel reduction scratch (aliases the H1 / dA2 images)
  static constexpr int RED = H1 * F0 + H1 + 2 * H2 + 1;
  static_assert(4 * RED <= 64 * HS + 64 * AS, "scratch fits");
};

// Stage the small per-bin parameters (all of layer 1/3, biases) and the W2
// image into LDS.
template <class S>
__device__ __forceinline__ void stage_params(const float *__restrict__ P,
                                             float *lds) {
  const PolicyLayout L{S::F0, S::H1, S::H2};
  const int tid = threadIdx.x;
  for (int i = tid; i < S::H2 * S::H1; i += blockDim.x) {
    const int o = i / S::H1, k = i - o * S::H1;
    lds[S::L_W2 + o * S::W2S + k] = P[L.oW2() + i];
  }
  for (int i = tid; i < S::H1 * S::F0; i += blockDim.x)
    lds[S::L_W1 + i] = P[L.oW1() + i];
  for (int i = tid; i < S::H1; i += blockDim.x) lds[S::L_B1 + i] = P[L.ob1() + i];
  for (int i = tid; i < S::H2; i += blockDim.x) {
    lds[S::L_B2 + i] = P[L.ob2() + i];
    lds[S::L_W3 + i] = P[L.ow3() + i];
  }
  if (tid == 0) lds[S::L_B3] = P[L.ob3()];
}

// The raw int8 state of the two rows a lane carries (rows rt*32 + lane&31 of
// a group), fetched one group ahead so the global-load latency overlaps the
// previous group's MFMA work (1 wave per SIMD in the train kernel).
template <class S>
struct RowRaw {
  int bv[2][S::D];
  int iv[2][S::D];
};

template <class S>
__device__ __forceinline__ void fetch_rows(const Batch &b, int slot, int e0,
                                           RowRaw<S> &rr) {
  const int lr = threadIdx.x & 31;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int r = rt * 32 + lr;
    const size_t env = (size_t)slot * b.N + e0 + r / S::B;
    const int8_t *bp = b.bins + env * S::BD + (r % S::B) * S::D;
    const int8_t *ip = b.items + env * 4;
#pragma unroll
    for (int d = 0; d < S::D; ++d) {
      rr.bv[rt][d] = bp[d];
      rr.iv[rt][d] = ip[d];
    }
  }
}

// Observation feature f of a row (observation::to_vector, bin_packing.h:31-40):
// [bin dims / 8, item dims / 8].  f may be runtime (lane-half dependent).
template <class S>
__device__ __forceinline__ float row_feature(const RowRaw<S> &rr, int rt,
                                             int f) {
  int v = 0;
#pragma unroll
  for (int d = 0; d < S::D; ++d) {
    if (f == d) v = rr.bv[rt][d];
    if (f == S::D + d) v = rr.iv[rt][d];
  }
  return f < S::F0 ? (float)v / (float)kCapacity : 0.0f;
}

// ============================== rollout step, wave per env, f16 pairs ==
// The wave-per-group rollout of the [128,128] and [64,64] shapes with layer 2 on the f16
// matrix cores at f32-class accuracy (xh_split.h, f16 pairs: W2 and H1 each
// scaled by a power of two chosen per launch -- max|W2|, and the bound
// |H1[r][i]| <= sum_k |W1[i][k]| + |b1[i]| since every observation feature
// is in [-1, 1] -- and split exactly into two f16 parts; three f16 products
// per K slice).  Layer 1 (f32 MFMA, the same chain, bias and relu as
// rollout_wave_kernel) leaves H1 tile `it` of an r-tile in accumulator
// registers (lane = row, register j = feature acc_row(j, h)); its registers
// 8s .. 8s+7, scaled and split, are directly the B operand of K-slice s of
// the 32x32x16 MFMA, whose k order is then feature it*32 + 16s + 8(e>>2) +
// 4h + (e&3) for element e of lane half h.  W2 is staged with the columns
// of every 16-block permuted to that order (bits 2 and 3 of the column
// swapped), so each A fragment is one ds_read_b128 of the swizzled image.
// Layer 1 is staged times S_H (weights and bias: its output is S_H H1
// exactly), b2 times S_W S_H as layer 2's C input and w3 divided by it, so
// the partial logits take the same roundings as unscaled values; both
// biases enter as the MFMA chains' C inputs.  The logits differ from rollout_wave_kernel's in the
// last places (f32-class: tests/test_gpu_scale.py); the sampler, the env
// step and everything after are the same code.
// Layer 1 runs its k-steps over the D bin features only: the item (an
// item-table entry in every slot these kernels see, RolloutArgs::wide
// otherwise) is folded into a per-entry bias, (b1 + W1_item . item / 8) S_H,
// as in the train kernels -- D = 2: one f32 MFMA per tile instead of two,
// D = 3: two instead of three.
// LDS (bytes): two W2 part images [o][permuted i] (H2 rows of 256 bytes: 64
// KB at [128,128]), then f32 W1 [H1][F0], b1, b2 S_W S_H, w3 / (S_W S_H), b3,
// S_H, the scale reduction, the two folded biases [2][H1].
template <class S>
struct RollSplitLds {
  static constexpr int W2 = 0;
  static constexpr int F = 2 * S::H2 * kImgRow;
  static constexpr int W1 = 0, B1 = S::H1 * S::F0, B2 = B1 + S::H1, W3 = B2 + S::H2,
                       B3 = W3 + S::H2, SH = B3 + 1, SC = B3 + 4, B1F = SC + 2 * 16;
  static constexpr int S1F = (S::D + 1) / 2;  // layer-1 k-steps over the bins
  static constexpr size_t bytes = F + sizeof(float) * (B1F + 2 * S::H1);
};

// Stage the f16-pair W2 images (columns permuted, see above) and the small
// parameters of the split rollouts; every thread of the block calls it (it
// synchronises the block).
template <class S>
__device__ __forceinline__ void stage_split_rollout(const float *__restrict__ P,
                                                    const EnvDesc &env, char *lds) {
  using L = RollSplitLds<S>;
  float *lf = reinterpret_cast<float *>(lds + L::F);
  const PolicyLayout PL{S::F0, S::H1, S::H2};
  // the scales: max|W2| and the H1 bound, reduced over the block
  float mw = 0.0f, mh = 0.0f;
  for (int e = threadIdx.x; e < S::H2 * S::H1; e += blockDim.x)
    mw = fmaxf(mw, fabsf(P[PL.oW2() + e]));
  for (int i = threadIdx.x; i < S::H1; i += blockDim.x) {
    float v = fabsf(P[PL.ob1() + i]);
    for (int k = 0; k < S::F0; ++k) v += fabsf(P[PL.oW1() + i * S::F0 + k]);
    mh = fmaxf(mh, v);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    mw = fmaxf(mw, __shfl_xor(mw, o, kWave));
    mh = fmaxf(mh, __shfl_xor(mh, o, kWave));
  }
  const int nw = blockDim.x >> 6, wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lf[L::SC + wv] = mw;
    lf[L::SC + 16 + wv] = mh;
  }
  __syncthreads();
  float MW = 0.0f, MH = 0.0f;
  for (int v = 0; v < nw; ++v) {
    MW = fmaxf(MW, lf[L::SC + v]);
    MH = fmaxf(MH, lf[L::SC + 16 + v]);
  }
  const float SW = f16_scale_for(MW), SH = f16_scale_for(MH), S2 = SW * SH;
  for (int e = threadIdx.x; e < S::H2 * S::H1; e += blockDim.x) {
    const int o = e / S::H1, i = e % S::H1;
    // logical column i -> its slot: bits 2 and 3 swapped within the 16-block
    const int c = (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1);
    _Float16 x0, x1;
    split2h(P[PL.oW2() + e] * SW, x0, x1);
    const int off = img_off(o, c >> 3) + 2 * (c & 7);
    *reinterpret_cast<_Float16 *>(lds + L::W2 + off) = x0;
    *reinterpret_cast<_Float16 *>(lds + L::W2 + S::H2 * kImgRow + off) = x1;
  }
  // layer 1 staged times S_H (its output is H1 S_H exactly: a power of two),
  // b2 times S_W S_H (layer 2's C input), w3 divided by it
  for (int i = threadIdx.x; i < S::H1 * S::F0; i += blockDim.x)
    lf[L::W1 + i] = P[PL.oW1() + i] * SH;
  for (int i = threadIdx.x; i < S::H1; i += blockDim.x) {
    lf[L::B1 + i] = P[PL.ob1() + i] * SH;
    lf[L::B2 + i] = P[PL.ob2() + i] * S2;
    lf[L::W3 + i] = P[PL.ow3() + i] * (1.0f / S2);
    float ba = P[PL.ob1() + i], bb = ba;
#pragma unroll
    for (int d = 0; d < S::D; ++d) {
      const float wv = P[PL.oW1() + i * S::F0 + S::D + d];
      ba += wv * ((float)env.item_a[d] / (float)kCapacity);
      bb += wv * ((float)env.item_b[d] / (float)kCapacity);
    }
    lf[L::B1F + i] = ba * SH;
    lf[L::B1F + S::H1 + i] = bb * SH;
  }
  if (threadIdx.x == 0) {
    lf[L::B3] = P[PL.ob3()];
    lf[L::SH] = SH;
  }
}

// Partial logits (without b3) of the two r-tiles of `cur` (64 rows) by the
// f16-pair layer 2: zl[rt] = the logit sum of row rt*32 + (lane & 31).
// b1r[rt]: the folded layer-1 bias (LDS, x S_H) of r-tile rt's item.
// E0: also the relu masks of the 64 x 128 pre-activations for PPO's first
// epoch, mbits[ot] = this lane's word 64 ot + lane of the record
// (spec8_e0_layout.h: bit 16 rt + e = [pre[ot][e] > 0] of r-tile rt; 0.0 and
// -0.0 give 0 as relu' does) -- two VALU per value (v_med3_i32 on the bits,
// v_lshl_or_b32), no compare writing VCC.
template <class S, bool E0 = false>
__device__ __forceinline__ void wave_logits_split(const char *lds,
                                                  const RowRaw<S> &cur,
                                                  const float *const (&b1r)[2],
                                                  float (&zl)[2],
                                                  unsigned *mbits = nullptr) {
  using L = RollSplitLds<S>;
  const float *lf = reinterpret_cast<const float *>(lds + L::F);
  const int lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
  const char *w2i[2] = {lds + L::W2, lds + L::W2 + S::H2 * kImgRow};
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    // the bin features only (feature 2 s1 + h < D; the item is in the bias)
    float xb[L::S1F];
#pragma unroll
    for (int s1 = 0; s1 < L::S1F; ++s1) {
      const int f = 2 * s1 + h;
      xb[s1] = f < S::D ? row_feature<S>(cur, rt, f) : 0.0f;
    }
    // layer 2's accumulators start at b2 S_W S_H (C layout: register 4q + u
    // = feature ot*32 + 8q + 4h + u)
    f32x16s pre[S::NOT];
#pragma unroll
    for (int ot = 0; ot < S::NOT; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bb = *reinterpret_cast<const float4 *>(lf + L::B2 + ot * 32 + 8 * q + 4 * h);
        pre[ot][4 * q + 0] = bb.x;
        pre[ot][4 * q + 1] = bb.y;
        pre[ot][4 * q + 2] = bb.z;
        pre[ot][4 * q + 3] = bb.w;
      }
    // (fully unrolled: the next tile's layer 1 and split schedule beside this
    // tile's layer-2 MFMAs; 0.75 -> 0.72 ms per config-3 iteration)
#pragma unroll
    for (int it = 0; it < S::NIT; ++it) {
      // layer-1 tile it, times S_H: the bias as the chain's C input, relu
      f32x16 t1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bb = *reinterpret_cast<const float4 *>(b1r[rt] + it * 32 + 8 * q + 4 * h);
        t1[4 * q + 0] = bb.x;
        t1[4 * q + 1] = bb.y;
        t1[4 * q + 2] = bb.z;
        t1[4 * q + 3] = bb.w;
      }
#pragma unroll
      for (int s1 = 0; s1 < L::S1F; ++s1) {
        const int k = 2 * s1 + h;
        const float wa = k < S::D ? lf[L::W1 + (it * 32 + lr) * S::F0 + k] : 0.0f;
        t1 = mfma32(wa, xb[s1], t1);
      }
      f16x8 bfr[2][2];
      {
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        u32x4_t hb[2], lb[2];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          unsigned h2, l2;
          split2h_x2(relu(t1[2 * jj]), relu(t1[2 * jj + 1]), h2, l2);
          hb[jj >> 2][jj & 3] = h2;
          lb[jj >> 2][jj & 3] = l2;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bfr[s][0] = __builtin_bit_cast(f16x8, hb[s]);
          bfr[s][1] = __builtin_bit_cast(f16x8, lb[s]);
        }
      }
#pragma unroll
      for (int ot = 0; ot < S::NOT; ++ot) {
        const int rb = row_base(ot * 32 + lr, h);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          f16x8 af[2];
#pragma unroll
          for (int p = 0; p < 2; ++p)
            af[p] = __builtin_bit_cast(f16x8, ld_row(w2i[p], rb, 2 * it + s));
          // the three f16 products, small terms first
          pre[ot] = mfma_f16(af[1], bfr[s][0], pre[ot]);
          pre[ot] = mfma_f16(af[0], bfr[s][1], pre[ot]);
          pre[ot] = mfma_f16(af[0], bfr[s][0], pre[ot]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float z = 0.0f;
#pragma unroll
    for (int ot = 0; ot < S::NOT; ++ot) {
      float zp = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 ww = *reinterpret_cast<const float4 *>(lf + L::W3 + ot * 32 + 8 * q + 4 * h);
        const float wq[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) zp = fmaf(relu(pre[ot][4 * q + u]), wq[u], zp);
      }
      z += zp + __shfl_xor(zp, 32, kWave);
    }
    zl[rt] = z;
    if constexpr (E0) {
#pragma unroll
      for (int ot = 0; ot < S::NOT; ++ot) {
        unsigned wd = rt == 0 ? 0u : mbits[ot];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          int m;
          asm("v_med3_i32 %0, %1, 0, 1" : "=v"(m) : "v"(__float_as_int(pre[ot][e])));
          wd |= (unsigned)m << sp8::e0_bit(rt, e);
        }
        mbits[ot] = wd;
      }
    }
  }
}

// The logit table of the 64-bin 2-D shape (xh_logit_table.h, DESIGN.md
// §3.0g): the partial logits (without b3) of every bin state in [-capacity,
// capacity]^2 under each of the two items, by wave_logits_split itself on
// synthetic rows -- call c carries states 32 c .. 32 c + 31 in both r-tiles,
// r-tile 0 with item_a's folded bias and r-tile 1 with item_b's.  A row's
// logit depends on its own MFMA column only and the half swap's sum is
// commutative, so an entry holds the bits the forward gives that (state, item)
// in any lane of any group.  Every wave of the block calls it after
// stage_split_rollout and its barrier (the calls are dealt to the waves);
// `out` holds lt::kEntries floats.
template <class S>
__device__ __forceinline__ void build_logit_table(const char *lds, float *out) {
  static_assert(S::B == 64 && S::D == 2 && S::G == 1 && lt::kCap == kCapacity,
                "the logit table: 64 bins, 2-D");
  const float *lfr = reinterpret_cast<const float *>(lds + RollSplitLds<S>::F);
  const float *const b1r[2] = {lfr + RollSplitLds<S>::B1F,
                               lfr + RollSplitLds<S>::B1F + S::H1};
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lr = lane & 31;
  const int nw = blockDim.x >> 6;
#pragma unroll 1
  for (int c = w; c < lt::kCalls; c += nw) {
    const int sn = lt::enum_state(c, lr);
    const int s = sn < lt::kStates ? sn : lt::kStates - 1;
    int b0, b1;
    lt::state_bins(s, b0, b1);
    RowRaw<S> cur;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      cur.bv[rt][0] = b0;
      cur.bv[rt][1] = b1;
      cur.iv[rt][0] = cur.iv[rt][1] = 0;  // folded into b1r: not read
    }
    float zl[2];
    wave_logits_split<S>(lds, cur, b1r, zl);
    if (lane < 32 && sn < lt::kStates) {
      out[lt::entry(0, b0, b1)] = zl[0];
      out[lt::entry(1, b0, b1)] = zl[1];
    }
  }
}

// Dynamic LDS of rollout_split_kernel: the staged parameters, then the table.
template <class S, bool TAB>
constexpr size_t roll_split_lds() {
  return RollSplitLds<S>::bytes + (TAB ? sizeof(float) * lt::kEntries : 0);
}

}  // namespace xh
