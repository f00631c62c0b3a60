// xh_host.h -- internal helpers of the C ABI's host runtime (every .cpp unit
// here): the error slot behind xh_last_error, status macros, the exception
// guard, stream-ordered copies, zero-filled device allocations, pooled timing
// events, the device row ring of the opt-in statistics (index arithmetic:
// xh_ring.h), the context struct with its release rule, and the env
// description both the trainer and the venv start from.
#ifndef XH_HOST_H_
#define XH_HOST_H_

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <exception>
#include <string>
#include <vector>

#include "../../include/xylo_hip.h"
#include "xh_kernels.h"
#include "xh_ring.h"

struct xh_ctx {
  int device = 0, rank = 0, world = 1;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;
  int trainers = 0;      // live trainers on this context
  bool closing = false;  // xh_ctx_destroy called while trainers were alive
  int fault = 0;         // xh_ctx_inject_fault (test hook): pending fault
};

namespace xh {
namespace host {

// the message of the last failing call on this thread (xh_last_error)
inline thread_local std::string g_err;

inline int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(x)                                                         \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess)                                                 \
      return fail(XH_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x,     \
                  hipGetErrorString(e_));                                 \
  } while (0)

#define RCCLCHK(x)                                                        \
  do {                                                                    \
    ncclResult_t r_ = (x);                                                \
    if (r_ != ncclSuccess)                                                \
      return fail(XH_ERR_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #x,    \
                  ncclGetErrorString(r_));                                \
  } while (0)

#define CHK(x)                   \
  do {                           \
    int s_ = (x);                \
    if (s_ != XH_OK) return s_;  \
  } while (0)

// Runs a cleanup after a failing call and keeps that call's message: the
// cleanup's own ABI calls may overwrite the error slot.
template <class F>
int fail_after(int status, F &&cleanup) {
  std::string keep = g_err;
  cleanup();
  g_err = std::move(keep);
  return status;
}

// No exception may cross the ABI.
template <class F>
int guard(F &&f) {
  try {
    return f();
  } catch (const std::exception &e) {
    return fail(XH_ERR_INVALID, "exception: %s", e.what());
  } catch (...) {
    return fail(XH_ERR_INVALID, "unknown exception");
  }
}

// Copies between the device and caller (pageable) host memory, ordered on
// the context's stream and waited for before returning (the caller may free
// or read its buffer right after).  Not hipMemcpy: the stream is
// non-blocking, so a null-stream H2D copy of pageable memory, which returns
// once the bytes are staged, is not ordered before the next kernel on it --
// measured: parameters read stale by the first rollout kernel, intermittently.
inline hipError_t copy_to_host(void *host, const void *dev, size_t n,
                               hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}
inline hipError_t copy_to_device(void *dev, const void *host, size_t n,
                                 hipStream_t s) {
  const hipError_t e = hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

inline int copy_ok(hipError_t e) {
  return e == hipSuccess ? XH_OK
                         : fail(XH_ERR_HIP, "copy: %s", hipGetErrorString(e));
}

// A device allocation of `bytes`, zeroed on the context's stream `s`: a
// null-stream hipMemset is not ordered before the non-blocking stream's next
// copy / kernel (measured: the zero fill landing after the parameter upload,
// intermittently).  *out is written on success only; `what` names the owner
// in the message.
inline int dev_zalloc(hipStream_t s, void **out, size_t bytes,
                      const char *what) {
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess)
    return fail(XH_ERR_HIP, "%s: allocating %zu bytes", what, bytes);
  if (hipMemsetAsync(p, 0, bytes, s) != hipSuccess) {
    (void)hipFree(p);
    return fail(XH_ERR_HIP, "%s: zero fill", what);
  }
  *out = p;
  return XH_OK;
}

// Timing events come from their owner's pool (which gets them back when the
// timing is reset), without the system-scope fence: they only time launches,
// every host read of device memory synchronises the stream itself.
inline hipError_t pooled_event(std::vector<hipEvent_t> &pool, hipEvent_t *e) {
  if (!pool.empty()) {
    *e = pool.back();
    pool.pop_back();
    return hipSuccess;
  }
  return hipEventCreateWithFlags(e, hipEventDisableSystemFence);
}

// A device ring of rows of `width` doubles (the trainer's statistics and
// update diagnostics, the venv's episode statistics): row r lives in slot
// r % history, `rows` counts the rows written so far, unwritten rows are NaN.
// Its owner allocates and fills `dev`; history == 0 while it is off.
struct row_ring {
  double *dev = nullptr;
  int width = 0;
  int history = 0;
  long rows = 0;
};

inline double *ring_row(const row_ring &r, long row) {
  return r.dev + (size_t)(row % r.history) * r.width;
}

// Rows [first, first + count) of the ring -> out, in at most two runs, after
// one synchronisation of the context's stream; `who` prefixes the messages.
inline int ring_read(const row_ring &r, const xh_ctx *c, long first, int count,
                     double *out, const char *who) {
  switch (ring_check(first, count, r.history, r.rows)) {
    case kRingRange:
      return fail(XH_ERR_INVALID, "%s: %d rows from row %ld, %ld written", who,
                  count, first, r.rows);
    case kRingOverwritten:
      return fail(XH_ERR_INVALID, "%s: row %ld is overwritten (the ring holds "
                  "rows %ld .. %ld)", who, first, r.rows - r.history,
                  r.rows - 1);
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const ring_runs run = ring_span(first, count, r.history);
  const size_t rowb = (size_t)r.width * 8;
  if (run.n1 > 0)
    HIPCHK(copy_to_host(out, r.dev + (size_t)run.at * r.width,
                        (size_t)run.n1 * rowb, c->stream));
  if (run.n2 > 0)
    HIPCHK(copy_to_host(out + (size_t)run.n1 * r.width, r.dev,
                        (size_t)run.n2 * rowb, c->stream));
  return XH_OK;
}

inline void ctx_free(xh_ctx *c) {
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->comm) ncclCommDestroy(c->comm);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

// A destroyed trainer or venv gives up its reference (counted: it held one):
// the last one frees a context that xh_ctx_destroy was already called on.
inline void ctx_release(xh_ctx *c, bool counted) {
  if (counted && --c->trainers == 0 && c->closing) ctx_free(c);
}

inline uint32_t mstd_pow(uint64_t k) {  // 16807^k mod (2^31-1)
  uint64_t acc = 1, base = 16807;
  while (k) {
    if (k & 1) acc = acc * base % 2147483647ull;
    base = base * base % 2147483647ull;
    k >>= 1;
  }
  return (uint32_t)acc;
}

constexpr int kBinCapacity = 8;  // bin_packing.h:48, every dim

// the bin-packing env of `bins` x `dims` (item sizes and their probability)
inline xh::EnvDesc make_env(int bins, int dims) {
  static const int ia[3][3] = {{4, 0, 0}, {4, 2, 0}, {4, 2, 2}};
  static const int ib[3][3] = {{1, 0, 0}, {1, 2, 0}, {1, 2, 1}};
  xh::EnvDesc env{};
  env.B = bins;
  env.D = dims;
  for (int d = 0; d < 3; ++d) {
    env.item_a[d] = ia[dims - 1][d];
    env.item_b[d] = ib[dims - 1][d];
  }
  env.p_a = 0.4;
  return env;
}

// venv_api.cpp: xh_venv_record_obs's checks and row addressing, for a launch
// that reads `count` rows of v's recorded window (a->obs is left null;
// a->count == 0: nothing to launch).  *cap: the venv's per-dim capacities
// (1 past its dims), *ctx: its context; either may be null.  `who` prefixes
// the messages.
int venv_record_rows(xh_venv *v, const char *who, int view,
                     const int32_t *rows_dev, long first, long count,
                     xh::VenvObsArgs *a, const int32_t **cap, xh_ctx **ctx);

}  // namespace host
}  // namespace xh

#endif  // XH_HOST_H_
