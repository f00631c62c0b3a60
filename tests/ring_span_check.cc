// CPU check of the device row rings' index arithmetic
// (dependence_free_rl_amd/csrc/xh_ring.h, used by xh_host.h's ring_read):
// ring_span against a brute-force walk, row i of a request in slot
// (first + i) % history, over every history in 1..5, every rows in 0..12 and
// every (first, count) inside the readable window; ring_check accepts exactly
// that window and names the reason for the rest.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "xh_ring.h"

using namespace xh::host;

static int fails = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond) && fails++ < 20)                                           \
      std::printf("FAIL %s (history %ld rows %ld first %ld count %ld)\n",  \
                  #cond, history, rows, first, count);                     \
  } while (0)

int main() {
  long cases = 0;
  for (long history = 1; history <= 5; ++history)
    for (long rows = 0; rows <= 12; ++rows) {
      const long lo = std::max(0L, rows - history);
      for (long first = lo; first <= rows; ++first)
        for (long count = 0; first + count <= rows; ++count, ++cases) {
          EXPECT(ring_check(first, count, history, rows) == kRingOk);
          const ring_runs r = ring_span(first, count, history);
          EXPECT(r.at >= 0 && r.at < history);
          EXPECT(r.n1 >= 0 && r.n2 >= 0 && r.n1 + r.n2 == count);
          EXPECT(r.at + r.n1 <= history && r.n2 <= r.at);
          // the two runs cover exactly the request's slots, in order
          std::vector<long> got;
          for (long i = 0; i < r.n1; ++i) got.push_back(r.at + i);
          for (long i = 0; i < r.n2; ++i) got.push_back(i);
          std::vector<long> want;
          for (long i = 0; i < count; ++i) want.push_back((first + i) % history);
          EXPECT(got == want);
        }
      // what the ABI refuses, with its reason
      for (long first = -2; first <= rows + 2; ++first)
        for (long count = -2; count <= rows + 3; ++count) {
          const int got = ring_check(first, count, history, rows);
          const int want = first < 0 || count < 0 || first + count > rows
                               ? kRingRange
                           : first < lo ? kRingOverwritten
                                        : kRingOk;
          EXPECT(got == want);
        }
    }
  std::printf("%ld requests checked\n", cases);
  if (fails) return 1;
  std::printf("ring span: ok\n");
  return 0;
}
