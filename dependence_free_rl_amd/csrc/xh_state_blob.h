// xh_state_blob.h -- the host-side reader of a trainer-state blob
// (include/xylo_hip.h, "THE BLOB").  The one piece of the state code that
// reads untrusted bytes: no HIP dependency, nothing is dereferenced before it
// is bounded, every fixed part is copied out of the (possibly unaligned)
// buffer before it is read.  xh_trainer_load_state and xh_state_describe
// (state_api.cpp) both go through parse().
#ifndef XH_STATE_BLOB_H_
#define XH_STATE_BLOB_H_

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/xylo_hip.h"
#include "xh_digest.h"

namespace xh {
namespace state {

constexpr size_t kHeaderBytes = 144, kSectionBytes = 32, kAlign = 16;
static_assert(sizeof(xh_state_header) == kHeaderBytes, "blob header layout");
static_assert(sizeof(xh_state_section) == kSectionBytes, "blob section layout");
static_assert(sizeof(xh_config) == 108, "xh_config is part of the blob header");

inline const char *section_name(uint32_t id) {
  static const char *const names[XH_SEC_COUNT] = {
      "policy_params", "value_params", "policy_opt_m", "policy_opt_v",
      "value_opt_m",   "value_opt_v",  "env_bins",     "env_items",
      "rng",           "kl_beta",      "optimizers",   "episode_len"};
  return id < XH_SEC_COUNT ? names[id] : "?";
}

inline size_t align_up(size_t n) { return (n + kAlign - 1) & ~(kAlign - 1); }

struct Parsed {
  xh_state_header h{};
  uint32_t n = 0;  // sections
  xh_state_section sec[XH_SEC_COUNT]{};
  const unsigned char *base = nullptr;

  const xh_state_section *find(uint32_t id) const {
    for (uint32_t k = 0; k < n; ++k)
      if (sec[k].id == id) return &sec[k];
    return nullptr;
  }
  const unsigned char *data(const xh_state_section &s) const {
    return base + s.offset;
  }
};

inline bool refuse(char *err, size_t cap, const char *fmt, ...) {
  if (err && cap) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(err, cap, fmt, ap);
    va_end(ap);
  }
  return false;
}

// Bounds and digests of a whole blob.  True: *out describes it and every
// section lies inside [table end, bytes).  False: err says why.
inline bool parse(const void *blob, size_t bytes, Parsed *out, char *err,
                  size_t errcap) {
  if (!blob || bytes < kHeaderBytes)
    return refuse(err, errcap, "state blob too short: %zu bytes, the header has %zu",
                  blob ? bytes : (size_t)0, kHeaderBytes);
  Parsed p;
  p.base = static_cast<const unsigned char *>(blob);
  std::memcpy(&p.h, p.base, kHeaderBytes);
  if (p.h.magic != XH_STATE_MAGIC)
    return refuse(err, errcap, "state blob: bad magic 0x%08x", p.h.magic);
  if (p.h.version != XH_STATE_VERSION)
    return refuse(err, errcap, "state blob: unknown version %u (this library reads %d)",
                  p.h.version, XH_STATE_VERSION);
  if (p.h.header_bytes != kHeaderBytes)
    return refuse(err, errcap, "state blob: header of %u bytes, expected %zu",
                  p.h.header_bytes, kHeaderBytes);
  if (p.h.total_bytes != (uint64_t)bytes)
    return refuse(err, errcap, "state blob: %zu bytes given, the header says %llu%s",
                  bytes, (unsigned long long)p.h.total_bytes,
                  p.h.total_bytes > bytes ? " (truncated)" : "");
  if (p.h.sections > XH_SEC_COUNT)
    return refuse(err, errcap, "state blob: %u sections, at most %d", p.h.sections,
                  (int)XH_SEC_COUNT);
  p.n = p.h.sections;
  const size_t table_end = kHeaderBytes + (size_t)p.n * kSectionBytes;
  if (table_end > bytes)
    return refuse(err, errcap, "state blob: section table ends at %zu, past the "
                  "blob's %zu bytes", table_end, bytes);
  size_t lo = table_end;  // the next section starts here or later
  for (uint32_t k = 0; k < p.n; ++k) {
    xh_state_section &s = p.sec[k];
    std::memcpy(&s, p.base + kHeaderBytes + (size_t)k * kSectionBytes,
                kSectionBytes);
    if (s.id >= XH_SEC_COUNT || (k > 0 && s.id <= p.sec[k - 1].id))
      return refuse(err, errcap, "state blob: section %u has id %u (ids are "
                    "below %d and increase)", k, s.id, (int)XH_SEC_COUNT);
    if (s.offset % kAlign || s.offset < lo || s.offset > bytes ||
        s.bytes > bytes - s.offset)
      return refuse(err, errcap, "state blob: section %s [%llu, +%llu) does not "
                    "lie in [%zu, %zu) at a multiple of %zu", section_name(s.id),
                    (unsigned long long)s.offset, (unsigned long long)s.bytes,
                    lo, bytes, kAlign);
    lo = (size_t)(s.offset + s.bytes);
  }
  for (uint32_t k = 0; k < p.n; ++k) {
    const xh_state_section &s = p.sec[k];
    const uint64_t d = digest_host(p.base + s.offset, (size_t)s.bytes);
    if (d != s.digest)
      return refuse(err, errcap, "state blob: section %s has digest %016llx, its "
                    "table entry says %016llx", section_name(s.id),
                    (unsigned long long)d, (unsigned long long)s.digest);
  }
  const uint64_t got = digest_host(p.base + kHeaderBytes, bytes - kHeaderBytes);
  if (got != p.h.payload_digest)
    return refuse(err, errcap, "state blob: payload digest %016llx, the header "
                  "says %016llx (corrupted)", (unsigned long long)got,
                  (unsigned long long)p.h.payload_digest);
  *out = p;
  return true;
}

inline void put(std::string &js, const char *fmt, ...) {
  char buf[160];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  js += buf;
}

inline void put_float(std::string &js, const char *name, float v) {
  if (std::isfinite(v))
    put(js, "\"%s\": %.9g, ", name, (double)v);
  else
    put(js, "\"%s\": null, ", name);
}

// xh_state_describe's JSON of a parsed blob.
inline std::string describe(const Parsed &p) {
  const xh_config &c = p.h.cfg;
  std::string js;
  put(js, "{\"version\": %u, \"bytes\": %llu, \"config\": {", p.h.version,
      (unsigned long long)p.h.total_bytes);
  put(js, "\"algo\": %d, \"num_envs\": %d, \"num_envs_global\": %d, "
      "\"env_offset\": %d, ", c.algo, c.num_envs, c.num_envs_global, c.env_offset);
  put(js, "\"bins\": %d, \"dims\": %d, \"steps\": %d, \"epochs\": %d, ", c.bins,
      c.dims, c.steps, c.epochs);
  put(js, "\"policy_h1\": %d, \"policy_h2\": %d, \"value_h1\": %d, "
      "\"value_h2\": %d, ", c.policy_h1, c.policy_h2, c.value_h1, c.value_h2);
  put_float(js, "lr_policy", c.lr_policy);
  put_float(js, "lr_value", c.lr_value);
  put_float(js, "wd_policy", c.wd_policy);
  put_float(js, "wd_value", c.wd_value);
  put_float(js, "gamma", c.gamma);
  put_float(js, "lambda", c.lambda);
  put_float(js, "clip_eps", c.clip_eps);
  put(js, "\"rng_state\": %u, ", c.rng_state);
  put_float(js, "kl_beta", c.kl_beta);
  put_float(js, "kl_target", c.kl_target);
  put(js, "\"adv_normalize\": %d, \"lr_scale_rows\": %d, \"train_grid_cap\": %d, "
      "\"record_distrib\": %d, \"record_last_step\": %d}, \"sections\": [",
      c.adv_normalize, c.lr_scale_rows, c.train_grid_cap, c.record_distrib,
      c.record_last_step);
  for (uint32_t k = 0; k < p.n; ++k)
    put(js, "%s{\"id\": %u, \"name\": \"%s\", \"bytes\": %llu, \"digest\": "
        "\"%016llx\"}", k ? ", " : "", p.sec[k].id, section_name(p.sec[k].id),
        (unsigned long long)p.sec[k].bytes, (unsigned long long)p.sec[k].digest);
  js += "]}";
  return js;
}

}  // namespace state
}  // namespace xh

#endif  // XH_STATE_BLOB_H_
