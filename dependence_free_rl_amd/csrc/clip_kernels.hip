// clip_kernels.hip -- global-norm gradient clipping on the device
// (xh_trainer_set_grad_clip, xh_clip_grad_norm; opt-in).  Two launches after
// the slab reduce (and the all-reduce, with a communicator):
//   clip_sumsq_kernel  one double partial of sum g[i]^2 per workgroup
//   clip_step_kernel   every workgroup sums the partials in the same fixed
//                      order, derives the scale (xh_clip.h) and runs the
//                      optimizer update (xh_opt.h) on g[i] * scale
// The gradient buffer itself is left as reduced.  No floating-point atomics:
// which lane and which workgroup adds element i is a function of i and n
// alone (not of the buffer's alignment), the lanes of a wave combine in a
// shuffle tree, the 4 waves in LDS in a fixed order and the partials in one
// wave in a fixed order, so the norm has the same bits from run to run and on
// every rank of a job (all ranks hold the same all-reduced gradient).
#include "xh_clip.h"
#include "xh_device.h"
#include "xh_kernels.h"
#include "xh_opt.h"

namespace xh {

namespace {

// four consecutive floats at any 4-byte aligned address (epoch e's policy
// gradient starts e * np floats into its buffer, np odd for the real nets):
// one 16-byte global load, which needs dword alignment only
typedef float float4_a4 __attribute__((ext_vector_type(4), aligned(4)));

}  // namespace

// part[block] = the sum over the block's share of (double)g[i] * (double)g[i].
// Thread k of the grid takes the float quads k, k + threads, ... in that
// order (x, y, z, w within a quad), then the tail element 4 * (n / 4) + k if
// there is one.
__global__ __launch_bounds__(256) void clip_sumsq_kernel(const float *g, int n,
                                                         double *part) {
#pragma clang fp contract(off)
  const int nq = n >> 2;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int nth = gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int q = tid; q < nq; q += nth) {
    const float4_a4 x = *reinterpret_cast<const float4_a4 *>(g + 4 * (size_t)q);
    const double a = (double)x.x, b = (double)x.y, c = (double)x.z,
                 d = (double)x.w;
    acc += a * a;
    acc += b * b;
    acc += c * c;
    acc += d * d;
  }
  const int tail = 4 * nq + tid;
  if (tid < 4 && tail < n) {
    const double a = (double)g[tail];
    acc += a * a;
  }
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Every wave of every workgroup sums part[0..nparts) the same way (lane l
// adds partials l, l + 64, ... in order, then the shuffle tree: the one-wave
// column sum of stats_kernels.hip), so all of them hold the same ss and the
// same scale without a second pass over memory or a grid-wide barrier.  Then
// the grid strides over the parameters: g' = g[i] * scale, one f32 multiply,
// and the unchanged opt_update on g'.  scaled != nullptr (xh_clip_grad_norm):
// g' is written there and no parameter is touched.  Workgroup 0 logs
// {norm, (double)scale}.
__global__ __launch_bounds__(256) void clip_step_kernel(
    const double *part, int nparts, double r, float max_norm, const float *g,
    float *p, float *m, float *v, int n, OptStep o, float *scaled,
    double *log) {
#pragma clang fp contract(off)
  double ss = 0.0;
  for (int i = threadIdx.x & 63; i < nparts; i += 64) ss += part[i];
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) ss += __shfl_xor(ss, k, kWave);
  const ClipScale c = clip_scale(ss, r, max_norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    log[0] = c.norm;
    log[1] = (double)c.scale;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const float gi = g[i] * c.scale;
    if (scaled)
      scaled[i] = gi;
    else
      opt_update(p, m, v, i, gi, o);
  }
}

// ----------------------------------------------------------- launchers ----
// one quad per thread up to kClipMaxParts workgroups: a function of n only
int clip_parts(int n) {
  const long b = ((long)n + 1023) / 1024;
  return (int)(b < 1 ? 1 : (b > kClipMaxParts ? kClipMaxParts : b));
}

hipError_t launch_clip_sumsq(const float *g, int n, double *part,
                             hipStream_t s) {
  hipLaunchKernelGGL(clip_sumsq_kernel, dim3(clip_parts(n)), dim3(256), 0, s, g,
                     n, part);
  return hipGetLastError();
}

hipError_t launch_clip_step(const double *part, double r, float max_norm,
                            const float *g, float *params, float *m, float *v,
                            int n, OptStep o, float *scaled, double *log,
                            hipStream_t s) {
  const long b = ((long)n + 255) / 256;
  const int grid = (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
  hipLaunchKernelGGL(clip_step_kernel, dim3(grid), dim3(256), 0, s, part,
                     clip_parts(n), r, max_norm, g, params, m, v, n, o, scaled,
                     log);
  return hipGetLastError();
}

}  // namespace xh
