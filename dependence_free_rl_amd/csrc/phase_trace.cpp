// phase_trace.cpp -- the diagnostic build's side of learn() (`make diag`):
// XH_ABLATE, which drops whole phases of the train kernel, and XH_PHASE_TRACE,
// the phase stamps of the first epoch's train launch summarised on stderr.
// The product library refuses the first and never arms the second: there this
// unit costs learn() two getenv calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../include/xylo_hip.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_trainer.h"

namespace xh {
namespace host {
namespace {

constexpr size_t kTraceN =
    (size_t)xh::kTraceBlocks * xh::kTraceGroups * 8 * xh::kTraceSlots;
// + the kernel span words: earliest start (init all ones), latest end
// and per-workgroup start / end words for 1024 workgroups
constexpr size_t kTraceBytes = kTraceN * 8 + 16 + 4096 * 8;

long long *g_trace_buf = nullptr;  // lives as long as the process

// per phase: summed cycles over groups 1.. (group 0 warms up) of wave `wave`,
// every wave for -1; "group" = stamp 0 of the next group minus stamp 0 of
// this one.  Returns the number of wave-groups summed.
long phase_sums(const std::vector<long long> &tr, int wave,
                double (&sum)[xh::kTraceSlots + 1]) {
  long n = 0;
  for (int b = 0; b < xh::kTraceBlocks; ++b)
    for (int gi = 1; gi + 1 < xh::kTraceGroups; ++gi)
      for (int w = 0; w < 8; ++w) {
        if (wave >= 0 && w != wave) continue;
        const long long *p =
            &tr[((b * xh::kTraceGroups + gi) * 8 + w) * xh::kTraceSlots];
        const long long *pn = p + 8 * xh::kTraceSlots;
        if (!p[0] || !pn[0]) continue;
        for (int k = 1; k < xh::kTraceSlots; ++k) sum[k] += p[k] - p[k - 1];
        sum[xh::kTraceSlots] += pn[0] - p[xh::kTraceSlots - 1];
        sum[0] += pn[0] - p[0];
        ++n;
      }
  return n;
}

// kernel-level stamps (4-wave kernel: the last trace group)
void report_kernel_stamps(const std::vector<long long> &tr) {
  double k1 = 0, k2 = 0, k3 = 0;
  long kn = 0;
  for (int b = 0; b < xh::kTraceBlocks; ++b)
    for (int w = 0; w < 8; ++w) {
      const long long *p =
          &tr[((b * xh::kTraceGroups + xh::kTraceGroups - 1) * 8 + w) *
              xh::kTraceSlots];
      if (!p[0] || !p[3]) continue;
      k1 += p[1] - p[0];
      k2 += p[2] - p[1];
      k3 += p[3] - p[2];
      ++kn;
    }
  if (kn)
    std::fprintf(stderr, "kernel stamps (%ld waves, cycles): stage %.0f "
                 "| groups %.0f | epilogue %.0f\n", kn, k1 / kn,
                 k2 / kn, k3 / kn);
}

double quantile(std::vector<double> v, double f) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[(size_t)(f * (v.size() - 1))];
}

// per-workgroup phase spread and placement, on the wall clock of `wc` kHz
void report_workgroups(const std::vector<long long> &tr, int wc) {
  // [b][start, staged, loop done, end] on the wall clock
  std::vector<double> ph[4];
  for (int b = 0; b < 512; ++b) {
    const long long *w4 = &tr[kTraceN + 2 + 4 * b];
    if (!w4[0] || !w4[3]) continue;
    ph[0].push_back((w4[1] - w4[0]) * 1e3 / wc);
    ph[1].push_back((w4[2] - w4[1]) * 1e3 / wc);
    ph[2].push_back((w4[3] - w4[2]) * 1e3 / wc);
    ph[3].push_back((w4[3] - w4[0]) * 1e3 / wc);
  }
  auto q = quantile;
  const char *nm[4] = {"stage", "groups", "epilogue", "total"};
  std::fprintf(stderr, "workgroups %zu (us, min/p10/med/p90/max):",
               ph[3].size());
  for (int k = 0; k < 4; ++k)
    std::fprintf(stderr, " %s %.1f/%.1f/%.1f/%.1f/%.1f", nm[k],
                 q(ph[k], 0), q(ph[k], .1), q(ph[k], .5), q(ph[k], .9),
                 q(ph[k], 1));
  std::fprintf(stderr, "\n");
  // placement: workgroups per CU (xcc, se, sh, cu from HW_ID /
  // XCC_ID) and the duration of each CU's pair
  std::map<long, std::vector<double>> cu;
  std::map<long, std::vector<int>> cub;
  for (int b = 0; b < 512; ++b) {
    const long long *w4 = &tr[kTraceN + 2 + 4 * b];
    if (!w4[0] || !w4[3]) continue;
    const unsigned hw = (unsigned)tr[kTraceN + 2 + 2048 + 2 * b];
    const unsigned xc = (unsigned)tr[kTraceN + 2 + 2048 + 2 * b + 1];
    const long key = ((long)(xc & 15) << 12) | (((hw >> 13) & 7) << 8) |
                     (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
    cu[key].push_back((w4[3] - w4[0]) * 1e3 / wc);
    cub[key].push_back(b);
  }
  std::map<size_t, int> per;
  std::vector<double> pmax, pdiff;
  for (auto &kv : cu) {
    per[kv.second.size()]++;
    if (kv.second.size() == 2) {
      pmax.push_back(std::max(kv.second[0], kv.second[1]));
      pdiff.push_back(std::fabs(kv.second[0] - kv.second[1]));
    }
  }
  std::fprintf(stderr, "placement: %zu CUs;", cu.size());
  for (auto &kv : per) std::fprintf(stderr, " %d CUs with %zu wg;", kv.second, kv.first);
  std::fprintf(stderr, " pair max dur p10/med/p90 %.1f/%.1f/%.1f, pair |diff| med/p90 %.1f/%.1f\n",
               q(pmax, .1), q(pmax, .5), q(pmax, .9), q(pdiff, .5), q(pdiff, .9));
  int shown = 0;
  for (auto &kv : cub) {
    if (shown++ >= 6) break;
    std::fprintf(stderr, "  cu %05lx: blocks", kv.first);
    for (size_t i = 0; i < kv.second.size(); ++i)
      std::fprintf(stderr, " %d(%.1fus)", kv.second[i], cu[kv.first][i]);
    std::fprintf(stderr, "\n");
  }
}

}  // namespace

int phase_trace_begin(xh_trainer *t, xh::PolicyTrainArgs *pa) {
  // XH_ABLATE drops whole phases (wrong results by design): honoured by the
  // diagnostic build only, refused by the product library
  const char *ab = std::getenv("XH_ABLATE");
  pa->ablate = ab ? std::atoi(ab) : 0;
  if (pa->ablate && !xh::diag_build())
    return fail(XH_ERR_INVALID, "XH_ABLATE=%s is set but this is the "
                "product library (phase ablation exists only in `make "
                "diag`)", ab);
  if (xh::diag_build() && std::getenv("XH_PHASE_TRACE")) {
    hipStream_t s = t->ctx->stream;
    if (!g_trace_buf && hipMalloc(&g_trace_buf, kTraceBytes) != hipSuccess)
      return fail(XH_ERR_HIP, "trace buffer");
    if (hipMemsetAsync(g_trace_buf, 0, kTraceBytes, s) != hipSuccess ||
        hipMemsetAsync(g_trace_buf + kTraceN, 0xFF, 8, s) != hipSuccess)
      return fail(XH_ERR_HIP, "trace buffer");
    pa->trace = g_trace_buf;
  }
  return XH_OK;
}

int phase_trace_report(xh_trainer *t, xh::PolicyTrainArgs *pa) {
  hipStream_t s = t->ctx->stream;
  std::vector<long long> tr(kTraceN + 2 + 4096);
  if (hipMemcpyAsync(tr.data(), pa->trace, kTraceBytes, hipMemcpyDeviceToHost,
                     s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(XH_ERR_HIP, "trace read-back");
  pa->trace = nullptr;  // first epoch only
  double sum[xh::kTraceSlots + 1] = {0};
  const long n = phase_sums(tr, -1, sum);
  std::fprintf(stderr, "phase trace (%ld wave-groups, cycles): group %.0f |"
               " fwd %.0f bar1 %.0f softmax %.0f layer3 %.0f bar2 %.0f"
               " dH1 %.0f dW2 %.0f end+bar3 %.0f\n", n,
               sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n,
               sum[5] / n, sum[6] / n, sum[7] / n, sum[8] / n);
  if (std::getenv("XH_PHASE_TRACE_WAVES"))  // the same means per wave
    for (int w = 0; w < 8; ++w) {
      double sw[xh::kTraceSlots + 1] = {0};
      const long nw = phase_sums(tr, w, sw);
      if (!nw) continue;
      std::fprintf(stderr, "  wave %d:", w);
      for (int k = 0; k <= xh::kTraceSlots; ++k)
        std::fprintf(stderr, " %.0f", sw[k] / nw);
      std::fprintf(stderr, "\n");
    }
  report_kernel_stamps(tr);
  int wc = 0;
  (void)hipDeviceGetAttribute(&wc, hipDeviceAttributeWallClockRate,
                              t->ctx->device);
  if (tr[kTraceN + 1] && wc > 0) {
    std::fprintf(stderr, "workgroup span: %.1f us (wall clock %d kHz)\n",
                 (double)(tr[kTraceN + 1] - tr[kTraceN]) * 1e3 / wc, wc);
    report_workgroups(tr, wc);
  }
  return XH_OK;
}

}  // namespace host
}  // namespace xh
