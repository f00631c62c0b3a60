// xh_digest.h -- the state digest (include/xylo_hip.h, "THE DIGEST"): the one
// definition the device kernel (digest_kernels.hip), xh_digest_host and the
// blob parser (xh_state_blob.h) compile.  No HIP dependency: a plain C++
// compiler sees host functions only.
#ifndef XH_DIGEST_H_
#define XH_DIGEST_H_

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XH_DIGEST_HD __host__ __device__
#else
#define XH_DIGEST_HD
#endif

namespace xh {

// splitmix64's finaliser (Steele, Lea, Flood 2014) after its increment
XH_DIGEST_HD inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the term of word w at word index i
XH_DIGEST_HD inline uint64_t digest_term(uint64_t i, uint32_t w) {
  return splitmix64((i << 32) | (uint64_t)w);
}

// sum of the terms of `bytes` bytes whose first word has index `first`
// (digest_host(p, n) = digest_host(p, k) + digest_host(p + k, n - k, k / 4)
// for k a multiple of 4: the additions commute).  Little-endian host.
inline uint64_t digest_host(const void *data, size_t bytes, uint64_t first = 0) {
  const unsigned char *p = static_cast<const unsigned char *>(data);
  const size_t full = bytes / 4;
  uint64_t acc = 0;
  for (size_t i = 0; i < full; ++i) {
    uint32_t w;
    std::memcpy(&w, p + 4 * i, 4);
    acc += digest_term(first + i, w);
  }
  if (bytes & 3) {
    uint32_t w = 0;
    std::memcpy(&w, p + 4 * full, bytes & 3);
    acc += digest_term(first + full, w);
  }
  return acc;
}

}  // namespace xh

#endif  // XH_DIGEST_H_
