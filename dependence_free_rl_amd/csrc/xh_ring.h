// xh_ring.h -- index arithmetic of the device row rings (xh_host.h: row_ring).
// Pure host code without a HIP header, so tests/ring_span_check.cc checks it
// with the host compiler alone.
#ifndef XH_RING_H_
#define XH_RING_H_

namespace xh {
namespace host {

// Why a read of rows [first, first + count) is refused, `rows` written so far.
enum { kRingOk = 0, kRingRange = 1, kRingOverwritten = 2 };
inline int ring_check(long first, long count, long history, long rows) {
  if (first < 0 || count < 0 || first > rows - count) return kRingRange;
  if (first < rows - history) return kRingOverwritten;
  return kRingOk;
}

// Row i of the request lives in slot (first + i) % history: at most two runs,
// n1 rows from slot `at`, then n2 rows from slot 0.
struct ring_runs {
  long at, n1, n2;
};
inline ring_runs ring_span(long first, long count, long history) {
  const long at = first % history;
  const long n1 = count < history - at ? count : history - at;
  return {at, n1, count - n1};
}

}  // namespace host
}  // namespace xh

#endif  // XH_RING_H_
