// diag_kernels.hip -- the sums of the PPO update diagnostics
// (xh_trainer_set_update_diag, opt-in): from the per-row records the policy
// forward left (policy_kernels.hip: policy_diag_kernel /
// policy_diag_split_kernel) and the batch's p_old and advantages to one row of
// XH_UPD_COUNT doubles in the diagnostics' device ring.
//
// The per-row terms are xh_diag.h's (the host check compiles the same
// function).  Sums as the training statistics form them (xh_sums.h): double,
// contraction off, shuffles within the wave, a fixed order across the
// workgroup's waves and across the workgroup partials; no floating-point
// atomics, so a row is bit-identical from run to run.
#include "../../include/xylo_hip.h"
#include "xh_device.h"
#include "xh_diag.h"
#include "xh_kernels.h"
#include "xh_sums.h"

namespace xh {

static_assert(XH_UPD_KL_SUM - XH_UPD_LOGR_SUM + 1 == kUpdSums &&
              XH_UPD_K3_SUM == XH_UPD_LOGR_SUM + 2 &&
              XH_UPD_ENTROPY_SUM == XH_UPD_LOGR_SUM + 5 &&
              XH_UPD_COUNT == XH_UPD_KL_SUM + 1,
              "row layout: the entries summed over ranks are contiguous");

// The seven sums over the T * N transition rows: log ratio, its square, k3,
// clipped rows, the surrogate, the entropy and the KL records (NaN records --
// no sampling distributions -- sum to NaN).  part[block][7].
__global__ __launch_bounds__(256) void update_diag_sum_kernel(
    const float *p_new, const float *pold, const float *adv, const double *ent,
    const double *kl, long n, float clip_eps, double *part) {
#pragma clang fp contract(off)
  double v[kUpdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n;
       q += (long)gridDim.x * blockDim.x) {
    const DiagTerms d = diag_terms(p_new[q], pold[q], adv[q], clip_eps);
    v[0] += d.logr;
    v[1] += d.logr2;
    v[2] += d.k3;
    v[3] += d.clipped;
    v[4] += d.surr;
    v[5] += ent[q];
    v[6] += kl[q];
  }
  block_sums<kUpdSums>(v, part + (size_t)blockIdx.x * kUpdSums);
}

// The row: the fixed-order sum of the workgroup partials (this rank's share;
// all-reduced on row[XH_UPD_LOGR_SUM ..] next) behind the learn index and the
// job's row count.
__global__ __launch_bounds__(64) void update_diag_row_kernel(
    const double *part, int nparts, double learn, double rows_global,
    double *row) {
#pragma clang fp contract(off)
  double v[kUpdSums];
  wave_column_sums<kUpdSums>(part, nparts, v);
  if (threadIdx.x != 0) return;
  row[XH_UPD_LEARN] = learn;
  row[XH_UPD_ROWS] = rows_global;
#pragma unroll
  for (int k = 0; k < kUpdSums; ++k) row[XH_UPD_LOGR_SUM + k] = v[k];
}

hipError_t launch_update_diag_sum(const float *p_new, const float *pold,
                                  const float *adv, const double *ent,
                                  const double *kl, int N, int T, float clip_eps,
                                  double *part, hipStream_t s) {
  hipLaunchKernelGGL(update_diag_sum_kernel, dim3(gae_grid(N)), dim3(256), 0, s,
                     p_new, pold, adv, ent, kl, (long)N * T, clip_eps, part);
  return hipGetLastError();
}

hipError_t launch_update_diag_row(const double *part, int nparts, double learn,
                                  double rows_global, double *row,
                                  hipStream_t s) {
  hipLaunchKernelGGL(update_diag_row_kernel, dim3(1), dim3(64), 0, s, part,
                     nparts, learn, rows_global, row);
  return hipGetLastError();
}

}  // namespace xh
