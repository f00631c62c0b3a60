// venv_episode_kernels.hip -- episode statistics of a venv (xh_venv_set_
// episode_stats, opt-in): the per-env blocks that venv_step_kernel and
// venv_act_kernel count into (venv_kernels.hip, venv_ep_count) reduced to one
// row of XH_VEP_COUNT doubles in a device ring.
//
// Per env: running int32 (the episode in flight), first int32 (the env's first
// finished length, -1 until then) and VenvEpAcc (the episodes that ended since
// the last row: count, length sum, square sum, min, max).  venv_ep_sum_kernel
// takes one env per lane (coalesced), sums in double -- every term is an
// integer and every sum stays below 2^53, so the sums are exact -- across the
// wave by shuffles, across the workgroup's 4 waves in LDS in a fixed order,
// one partial per workgroup (xh_sums.h); the min / max entries go the same
// way.  It clears the accumulators it read.  venv_ep_row_kernel, one wave,
// adds the partials in a fixed order and writes the row.  No floating-point
// atomics: a row is bit-identical from run to run.
#include <climits>

#include "../../include/xylo_hip.h"
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_sums.h"

namespace xh {

namespace {

// min of v[0], max of v[1] and v[2] over a 256-thread workgroup -> part[0..3)
__device__ __forceinline__ void block_exts(double (&v)[kVepExts], double *part) {
  __shared__ double red[kVepExts][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v[0] = fmin(v[0], __shfl_xor(v[0], o, kWave));
    v[1] = fmax(v[1], __shfl_xor(v[1], o, kWave));
    v[2] = fmax(v[2], __shfl_xor(v[2], o, kWave));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < kVepExts; ++k) red[k][w] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    part[0] = fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3]));
    part[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    part[2] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
  }
}

__device__ __forceinline__ VenvEpAcc ep_acc_cleared() {
  VenvEpAcc z;
  z.count = 0;
  z.len_min = INT_MAX;
  z.len_max = 0;
  z.pad = 0;
  z.len_sum = 0;
  z.len_sqsum = 0;
  return z;
}

}  // namespace

__global__ __launch_bounds__(256) void venv_ep_init_kernel(
    int N, int32_t *running, int32_t *first, VenvEpAcc *acc) {
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < N;
       env += gridDim.x * blockDim.x) {
    running[env] = 0;
    first[env] = -1;
    acc[env] = ep_acc_cleared();
  }
}

// psum[block] = (episodes, sum len, sum len^2, envs finished, sum first, sum
// first^2, sum running); pext[block] = (min len, max len, max running), +inf /
// -inf / -inf where the block has none.
__global__ __launch_bounds__(256) void venv_ep_sum_kernel(
    int N, const int32_t *running, const int32_t *first, VenvEpAcc *acc,
    double *psum, double *pext) {
#pragma clang fp contract(off)
  double v[kVepSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double x[kVepExts] = {(double)INFINITY, -(double)INFINITY,
                        -(double)INFINITY};
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < N;
       env += gridDim.x * blockDim.x) {
    const int run = running[env];
    const int fl = first[env];
    const VenvEpAcc ac = acc[env];
    if (ac.count != 0) {
      v[0] += (double)ac.count;
      v[1] += (double)ac.len_sum;
      v[2] += (double)ac.len_sqsum;
      x[0] = fmin(x[0], (double)ac.len_min);
      x[1] = fmax(x[1], (double)ac.len_max);
      acc[env] = ep_acc_cleared();
    }
    if (fl >= 0) {
      const double f = (double)fl;
      v[3] += 1.0;
      v[4] += f;
      v[5] += f * f;
    }
    v[6] += (double)run;
    x[2] = fmax(x[2], (double)run);
  }
  block_sums<kVepSums>(v, psum + (size_t)blockIdx.x * kVepSums);
  block_exts(x, pext + (size_t)blockIdx.x * kVepExts);
}

__global__ __launch_bounds__(64) void venv_ep_row_kernel(
    const double *psum, const double *pext, int nparts, double row_index,
    double calls, double *row) {
#pragma clang fp contract(off)
  double v[kVepSums];
  wave_column_sums<kVepSums>(psum, nparts, v);
  double x[kVepExts] = {(double)INFINITY, -(double)INFINITY,
                        -(double)INFINITY};
  for (int i = threadIdx.x; i < nparts; i += 64) {
    x[0] = fmin(x[0], pext[(size_t)i * kVepExts]);
    x[1] = fmax(x[1], pext[(size_t)i * kVepExts + 1]);
    x[2] = fmax(x[2], pext[(size_t)i * kVepExts + 2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x[0] = fmin(x[0], __shfl_xor(x[0], o, kWave));
    x[1] = fmax(x[1], __shfl_xor(x[1], o, kWave));
    x[2] = fmax(x[2], __shfl_xor(x[2], o, kWave));
  }
  if (threadIdx.x != 0) return;
  const double nan = __builtin_nan("");
  row[XH_VEP_ROW] = row_index;
  row[XH_VEP_CALLS] = calls;
  row[XH_VEP_EPISODES] = v[0];
  row[XH_VEP_LEN_SUM] = v[1];
  row[XH_VEP_LEN_SQSUM] = v[2];
  row[XH_VEP_LEN_MIN] = v[0] > 0.0 ? x[0] : nan;
  row[XH_VEP_LEN_MAX] = v[0] > 0.0 ? x[1] : nan;
  row[XH_VEP_ENVS_FINISHED] = v[3];
  row[XH_VEP_FIRST_LEN_SUM] = v[4];
  row[XH_VEP_FIRST_LEN_SQSUM] = v[5];
  row[XH_VEP_RUNNING_SUM] = v[6];
  row[XH_VEP_RUNNING_MAX] = x[2];
}

// ----------------------------------------------------------- launchers ----
// workgroups of the reduction: 256 envs each up to 1024 of them, then a
// grid-stride loop (the one-wave row kernel walks the partials 64 at a time)
int venv_ep_grid(int N) {
  const long b = ((long)N + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

hipError_t launch_venv_ep_init(int N, int32_t *running, int32_t *first,
                               VenvEpAcc *acc, hipStream_t s) {
  hipLaunchKernelGGL(venv_ep_init_kernel, dim3(venv_ep_grid(N)), dim3(256), 0,
                     s, N, running, first, acc);
  return hipGetLastError();
}

hipError_t launch_venv_ep_row(int N, const int32_t *running,
                              const int32_t *first, VenvEpAcc *acc,
                              double *psum, double *pext, double row_index,
                              double calls, double *row, hipStream_t s) {
  const int grid = venv_ep_grid(N);
  hipLaunchKernelGGL(venv_ep_sum_kernel, dim3(grid), dim3(256), 0, s, N,
                     running, first, acc, psum, pext);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(venv_ep_row_kernel, dim3(1), dim3(64), 0, s, psum, pext,
                     grid, row_index, calls, row);
  return hipGetLastError();
}

}  // namespace xh
