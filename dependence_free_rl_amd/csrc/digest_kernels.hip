// digest_kernels.hip -- the state digest on the device (xh_trainer_state_digest
// and the verification pass of xh_trainer_load_state; opt-in, nothing in
// rollout() or learn() launches it).  Two launches for all arrays of a trainer:
//   digest_partial_kernel  grid (kDigestBlocks, entries): one uint64 partial
//                          per workgroup of the terms of its share of words
//   digest_final_kernel    one workgroup: wave w sums the partials of entries
//                          w, w + 4, ... and writes their digests
// The terms (xh_digest.h: splitmix64 of word index and word) are added mod
// 2^64, which is associative and commutative, so which thread takes which word
// and the shape of the reduction tree do not change the result: no atomics, no
// fixed order, no floating point, and the value xh_digest_host gets in a loop.
#include "xh_device.h"
#include "xh_digest.h"
#include "xh_kernels.h"

namespace xh {

namespace {

typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

}  // namespace

// Words are taken grid-strided: as 16-byte loads where the array starts on a
// 16-byte boundary (every array but an env slot of an odd-sized batch), as
// dwords where it starts on a 4-byte boundary, else byte by byte; the up to
// three tail bytes, zero-padded to a word, by the entry's first thread.  Every
// branch is uniform over the workgroup.
__global__ __launch_bounds__(256) void digest_partial_kernel(DigestTable tab,
                                                             u64 *part) {
  const int k = blockIdx.y;
  const unsigned char *p = static_cast<const unsigned char *>(tab.e[k].ptr);
  const u64 bytes = tab.e[k].bytes;
  const u64 full = bytes >> 2;  // whole words
  const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 nth = (u64)gridDim.x * blockDim.x;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
  u64 acc = 0, start = 0;
  if ((addr & 15) == 0) {
    const u64 nq = full >> 2;
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    for (u64 i = tid; i < nq; i += nth) {
      const u32x4 v = q[i];
      acc += digest_term(4 * i, v.x) + digest_term(4 * i + 1, v.y) +
             digest_term(4 * i + 2, v.z) + digest_term(4 * i + 3, v.w);
    }
    start = nq << 2;
  }
  if ((addr & 3) == 0) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    for (u64 i = start + tid; i < full; i += nth) acc += digest_term(i, w[i]);
  } else {
    for (u64 i = tid; i < full; i += nth) {
      const unsigned char *b = p + 4 * i;
      acc += digest_term(i, (uint32_t)b[0] | (uint32_t)b[1] << 8 |
                                (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24);
    }
  }
  if (tid == 0 && (bytes & 3)) {
    uint32_t w = 0;
    for (u64 b = 0; b < (bytes & 3); ++b)
      w |= (uint32_t)p[4 * full + b] << (8 * b);
    acc += digest_term(full, w);
  }
  __shared__ u64 red[4];
  acc = wave_sum_u64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    part[(size_t)k * kDigestBlocks + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// out[k] = the sum of entry k's kDigestBlocks partials for k < n, else 0.
__global__ __launch_bounds__(256) void digest_final_kernel(const u64 *part, int n,
                                                           u64 *out) {
  const int lane = threadIdx.x & 63;
  for (int k = threadIdx.x >> 6; k < kDigestMaxEntries; k += 4) {
    u64 acc = 0;
    if (k < n)
      for (int i = lane; i < kDigestBlocks; i += kWave)
        acc += part[(size_t)k * kDigestBlocks + i];
    acc = wave_sum_u64(acc);
    if (lane == 0) out[k] = acc;
  }
}

hipError_t launch_digest(const DigestTable &tab, unsigned long long *ws,
                         hipStream_t s) {
  if (tab.n < 0 || tab.n > kDigestMaxEntries) return hipErrorInvalidValue;
  if (tab.n > 0) {
    hipLaunchKernelGGL(digest_partial_kernel, dim3(kDigestBlocks, tab.n),
                       dim3(256), 0, s, tab, ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(digest_final_kernel, dim3(1), dim3(256), 0, s, ws, tab.n,
                     digest_results(ws));
  return hipGetLastError();
}

}  // namespace xh
