// xh_sums.h -- the fixed-order double sums of the on-device statistics
// (stats_kernels.hip) and the update diagnostics (diag_kernels.hip): reduced
// across the wave by shuffles, across the workgroup's 4 waves in LDS in a
// fixed order, one partial per workgroup, and the partials summed in a fixed
// order by one wave.  No floating-point atomics.
#pragma once
#include "xh_device.h"

namespace xh {
namespace {

// s += x in double with the rounding error kept (Knuth's two-sum): c collects
// what the additions lose, so a lane's sum over any number of steps carries
// one rounding, not one per step (venv_gae_kernel, venv_policy_loss_kernel)
__device__ __forceinline__ void sum2(double &s, double &c, double x) {
#pragma clang fp contract(off)
  const double t = s + x;
  const double bb = t - s;
  c += (s - (t - bb)) + (x - bb);
  s = t;
}

// Sums of S values over a 256-thread workgroup -> part[0..S) (thread 0).
template <int S>
__device__ __forceinline__ void block_sums(double (&v)[S], double *part) {
  __shared__ double red[S][4];
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, kWave);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < S; ++k) red[k][w] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < S; ++k)
      part[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}

// Column sums of part[nparts][S] in one wave: lane l adds rows l, l + 64, ...
// in order, then the shuffle tree.  Every lane returns the sums.
template <int S>
__device__ __forceinline__ void wave_column_sums(const double *part, int nparts,
                                                 double (&v)[S]) {
#pragma unroll
  for (int k = 0; k < S; ++k) v[k] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 64)
#pragma unroll
    for (int k = 0; k < S; ++k) v[k] += part[(size_t)i * S + k];
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, kWave);
}

}  // namespace
}  // namespace xh
