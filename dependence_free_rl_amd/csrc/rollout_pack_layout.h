// rollout_pack_layout.h -- the lane layout of the packed 64-bin table rollout
// (rollout_pack_kernels.hip) and the order of its softmax
// sum, compiled by the kernel and by the host check
// (tests/rollout_pack_layout_check.cc): plain C++, no HIP header needed on
// the host.
//
// A wave steps G = 64 / L envs at once.  Lane l holds env e0 + l / L and the
// kBpl = 64 / L consecutive bins (l % L) * kBpl .. of it; an env's L lanes are
// an aligned segment of the wave, inside one row of 16 lanes when L <= 16.
//
// The softmax sum keeps the bits of seg_sum<64> over lane = bin (xh_device.h):
// that is the xor butterfly over the bin index, levels 1, 2, .., 32, and float
// addition commutes, so a level only has to add the two partial sums the
// butterfly adds.  Levels 1 .. kBpl / 2 pair bins of one lane (lane_tree), the
// levels from kBpl on pair lane l with lane l ^ (level / kBpl) of its segment
// (seg_sum<L>: DPP patterns for L <= 16).
#ifndef XH_ROLLOUT_PACK_LAYOUT_H_
#define XH_ROLLOUT_PACK_LAYOUT_H_

#if defined(__HIPCC__)
#define XH_RP_HD __host__ __device__
#else
#define XH_RP_HD
#endif

namespace xh {
namespace rp {

constexpr int kWaveLanes = 64;
constexpr int kBins = 64;  // the shape's bins per env

template <int L>
struct Pack {
  static_assert(L == 4 || L == 8 || L == 16, "lanes per env: 4, 8 or 16");
  static constexpr int kL = L;
  static constexpr int kG = kWaveLanes / L;  // envs per wave
  static constexpr int kBpl = kBins / L;     // bins per lane
  // the env (offset from the wave's first) and the first bin of a lane
  XH_RP_HD static int env_of(int lane) { return lane / L; }
  XH_RP_HD static int pos_of(int lane) { return lane % L; }
  XH_RP_HD static int bin0_of(int lane) { return (lane % L) * kBpl; }
  // the lane and the register of bin `bin` of the wave's env number `e`
  XH_RP_HD static int lane_of(int e, int bin) { return e * L + bin / kBpl; }
  XH_RP_HD static int reg_of(int bin) { return bin % kBpl; }
  // waves that N envs take, and whether a lane of wave g carries an env
  XH_RP_HD static int groups(int N) { return (N + kG - 1) / kG; }
  XH_RP_HD static bool active(int g, int lane, int N) { return g * kG + lane / L < N; }
};

// The in-lane levels of the sum: the butterfly's levels 1 .. N / 2 over N
// consecutive bins (v[i] += v[i ^ o] for the i with bit o clear).
template <int N>
XH_RP_HD inline float lane_tree(const float (&v)[N]) {
  float t[N];
  for (int i = 0; i < N; ++i) t[i] = v[i];
  for (int o = 1; o < N; o <<= 1)
    for (int i = 0; i < N; i += 2 * o) t[i] = t[i] + t[i + o];
  return t[0];
}

}  // namespace rp
}  // namespace xh

#endif  // XH_ROLLOUT_PACK_LAYOUT_H_
