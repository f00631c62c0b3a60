// stats_kernels.hip -- on-device training statistics (xh_trainer_set_stats,
// opt-in): one row of XH_STAT_COUNT doubles per iteration in a device ring.
// The rollout opens the row with the episode part (episode_stats_kernel +
// episode_row_kernel), learn() fills the learner part (learner_stats_kernel +
// grad_norm_kernel + learner_row_kernel).
//
// Every sum is accumulated in double with contraction off (each term is the
// plain IEEE product / sum a host check reproduces), reduced across the wave
// by shuffles, across the workgroup's 4 waves in LDS in a fixed order, written
// as one partial per workgroup, and the partials are summed in a fixed order
// by one wave (the adv_stats_kernel pattern, value_kernels.hip).  No
// floating-point atomics: a row is bit-identical from run to run.
#include "../../include/xylo_hip.h"
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_sums.h"

namespace xh {

static_assert(XH_STAT_NEGLOGP_SUM - XH_STAT_EPISODES + 1 == kStatEpisodeSummed &&
              XH_STAT_ADV_SQSUM - XH_STAT_VERR_SUM + 1 == kStatLearnerSums &&
              XH_STAT_VERR_SUM == XH_STAT_NEGLOGP_SUM + 1,
              "row layout: the entries summed over ranks are contiguous");

// One env per lane: walks done[0..T)[e] in slot order (coalesced across envs
// in the [T][N] layout) with the env's running episode length, which persists
// in ep_len across launches (an episode spans several rollout windows).  At
// each done the finished length (the overflowing step included) and its
// square are added and the count restarts.  The same pass adds
// -log((double)p_old).  part[block] = (episodes, sum len, sum len^2,
// sum -log p_old).
__global__ __launch_bounds__(256) void episode_stats_kernel(
    const uint8_t *done, const float *pold, int N, int T, int *ep_len,
    double *part) {
#pragma clang fp contract(off)
  double v[kStatEpisodeSums] = {0.0, 0.0, 0.0, 0.0};
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < N;
       env += gridDim.x * blockDim.x) {
    int len = ep_len[env];
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const size_t q = (size_t)t * N + env;
      const int d = done[q];
      const double p = (double)pold[q];
      ++len;
      if (d) {
        const double l = (double)len;
        v[0] += 1.0;
        v[1] += l;
        v[2] += l * l;
        len = 0;
      }
      v[3] += -log(p);
    }
    ep_len[env] = len;
  }
  block_sums<kStatEpisodeSums>(v, part + (size_t)blockIdx.x * kStatEpisodeSums);
}

// Opens the row: the fixed-order sum of the workgroup partials, the episode
// part (this rank's share of the summed entries; the all-reduce over ranks
// runs on row[XH_STAT_EPISODES ..] next) and NaN in the learner part.
__global__ __launch_bounds__(64) void episode_row_kernel(
    const double *part, int nparts, double iter, double transitions_global,
    double transitions_local, double *row) {
#pragma clang fp contract(off)
  double v[kStatEpisodeSums];
  wave_column_sums<kStatEpisodeSums>(part, nparts, v);
  if (threadIdx.x != 0) return;
  row[XH_STAT_ITER] = iter;
  row[XH_STAT_TRANSITIONS] = transitions_global;
  row[XH_STAT_EPISODES] = v[0];
  row[XH_STAT_EPLEN_SUM] = v[1];
  row[XH_STAT_EPLEN_SQSUM] = v[2];
  // reward 1 per step, 0 on the overflowing step (bin_packing.h:102-106)
  row[XH_STAT_REWARD_SUM] = transitions_local - v[0];
  row[XH_STAT_NEGLOGP_SUM] = v[3];
  const double nan = __builtin_nan("");
  for (int k = XH_STAT_VERR_SUM; k < XH_STAT_COUNT; ++k) row[k] = nan;
}

// The six sums over the T * N transition rows: e = target - V0, e^2, target,
// target^2, A, A^2.  part[block][6].
__global__ __launch_bounds__(256) void learner_stats_kernel(
    const float *v0, const float *targets, const float *adv, long n,
    double *part) {
#pragma clang fp contract(off)
  double v[kStatLearnerSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n;
       q += (long)gridDim.x * blockDim.x) {
    const double tg = (double)targets[q];
    const double e = tg - (double)v0[q];
    const double a = (double)adv[q];
    v[0] += e;
    v[1] += e * e;
    v[2] += tg;
    v[3] += tg * tg;
    v[4] += a;
    v[5] += a * a;
  }
  block_sums<kStatLearnerSums>(v, part + (size_t)blockIdx.x * kStatLearnerSums);
}

// Squared L2 norms of three flat f32 vectors, one workgroup each: the first
// and the last epoch's policy gradient and the value gradient -> out[0..3).
__global__ __launch_bounds__(256) void grad_norm_kernel(
    const float *g0, const float *g1, int np, const float *gv, int nv,
    double *out) {
#pragma clang fp contract(off)
  const float *g = blockIdx.x == 0 ? g0 : blockIdx.x == 1 ? g1 : gv;
  const int n = blockIdx.x == 2 ? nv : np;
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double x = (double)g[i];
    v[0] += x * x;
  }
  block_sums<1>(v, out + blockIdx.x);
}

// Fills the learner part of the open row: the fixed-order sum of the
// workgroup partials (this rank's share; all-reduced on row[XH_STAT_VERR_SUM
// ..] next), then the entries that are job-wide already: the gradient norms
// and, for KL-PPO (kl_last != nullptr: the last epoch's [beta used, mean KL,
// new beta]), the beta and the mean KL; and from the clip logs of this learn()
// (clip_kernels.hip; nullptr while clipping is off for the net) the clipped
// policy steps, the smallest policy scale and the value scale.
__global__ __launch_bounds__(64) void learner_row_kernel(
    const double *part, int nparts, const double *norms, const float *kl_last,
    const double *pclip, int psteps, const double *vclip, double *row) {
#pragma clang fp contract(off)
  double v[kStatLearnerSums];
  wave_column_sums<kStatLearnerSums>(part, nparts, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kStatLearnerSums; ++k) row[XH_STAT_VERR_SUM + k] = v[k];
  row[XH_STAT_PGRAD_SQ_FIRST] = norms[0];
  row[XH_STAT_PGRAD_SQ_LAST] = norms[1];
  row[XH_STAT_VGRAD_SQ] = norms[2];
  const double nan = __builtin_nan("");
  row[XH_STAT_KL_BETA] = kl_last ? (double)kl_last[2] : nan;
  row[XH_STAT_KL_MEAN] = kl_last ? (double)kl_last[1] : nan;
  // the clip logs of this learn() ({norm, scale} per optimizer step)
  double steps = nan, smin = nan;
  if (pclip) {
    steps = 0.0;
    smin = 1.0;
    for (int e = 0; e < psteps; ++e) {
      const double sc = pclip[2 * e + 1];
      if (sc < 1.0) steps += 1.0;
      if (sc < smin) smin = sc;
    }
  }
  row[XH_STAT_PCLIP_STEPS] = steps;
  row[XH_STAT_PCLIP_SCALE_MIN] = smin;
  row[XH_STAT_VCLIP_SCALE] = vclip ? vclip[1] : nan;
}

// ----------------------------------------------------------- launchers ----
hipError_t launch_episode_stats(const uint8_t *done, const float *pold, int N,
                                int T, int *ep_len, double *part,
                                hipStream_t s) {
  hipLaunchKernelGGL(episode_stats_kernel, dim3(gae_grid(N)), dim3(256), 0, s,
                     done, pold, N, T, ep_len, part);
  return hipGetLastError();
}

hipError_t launch_episode_row(const double *part, int nparts, double iter,
                              double transitions_global,
                              double transitions_local, double *row,
                              hipStream_t s) {
  hipLaunchKernelGGL(episode_row_kernel, dim3(1), dim3(64), 0, s, part, nparts,
                     iter, transitions_global, transitions_local, row);
  return hipGetLastError();
}

hipError_t launch_learner_stats(const float *v0, const float *targets,
                                const float *adv, int N, int T, double *part,
                                hipStream_t s) {
  hipLaunchKernelGGL(learner_stats_kernel, dim3(gae_grid(N)), dim3(256), 0, s,
                     v0, targets, adv, (long)N * T, part);
  return hipGetLastError();
}

hipError_t launch_grad_norms(const float *g_first, const float *g_last, int np,
                             const float *gv, int nv, double *out,
                             hipStream_t s) {
  hipLaunchKernelGGL(grad_norm_kernel, dim3(3), dim3(256), 0, s, g_first,
                     g_last, np, gv, nv, out);
  return hipGetLastError();
}

hipError_t launch_learner_row(const double *part, int nparts,
                              const double *norms, const float *kl_last,
                              const double *pclip, int psteps,
                              const double *vclip, double *row, hipStream_t s) {
  hipLaunchKernelGGL(learner_row_kernel, dim3(1), dim3(64), 0, s, part, nparts,
                     norms, kl_last, pclip, psteps, vclip, row);
  return hipGetLastError();
}

}  // namespace xh
