// state_api.cpp -- trainer-state checkpoints of the C ABI (include/xylo_hip.h,
// "trainer state"): xh_trainer_state_bytes / save_state / load_state /
// state_digest, and the host-only xh_state_describe / xh_digest_host.  The
// blob is read through xh_state_blob.h only; the digest is xh_digest.h on the
// host and digest_kernels.hip on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/xylo_hip.h"
#include "xh_digest.h"
#include "xh_host.h"
#include "xh_kernels.h"
#include "xh_state_blob.h"
#include "xh_trainer.h"

using namespace xh::host;
namespace blob = xh::state;

static_assert(xh::kDigestMaxEntries == XH_DIG_COUNT, "digest table size");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "digest word");

namespace {

constexpr size_t kOptRecordBytes = 32;  // XH_SEC_OPT: one per net

// XH_SEC_OPT's record of one net
struct OptRecord {
  int32_t kind;
  float lr, wd, beta1, beta2, t;
  uint32_t zero[2];
};
static_assert(sizeof(OptRecord) == kOptRecordBytes, "optimizer record layout");

// The slot of bins / items that holds the states the next rollout starts from
// (xh_trainer_get_env_state's resolution; do_pg_rollout's for XH_PG).
size_t start_slot(const xh_trainer *t) {
  if (!t->need_shift) return 0;
  return t->cfg.algo == XH_PG ? (size_t)t->pg.slot_end : t->T();
}

// The trainer's state arrays: where section `id` lies in device memory (null:
// a host-side section) and its size (0: absent).
struct Sections {
  const void *dev[XH_SEC_COUNT] = {};
  size_t bytes[XH_SEC_COUNT] = {};
};

Sections sections_of(const xh_trainer *t) {
  Sections s;
  const size_t N = t->N(), slot = start_slot(t);
  s.dev[XH_DIG_POLICY_PARAMS] = t->pp;
  s.bytes[XH_DIG_POLICY_PARAMS] = (size_t)t->np * 4;
  if (t->vp) {
    s.dev[XH_DIG_VALUE_PARAMS] = t->vp;
    s.bytes[XH_DIG_VALUE_PARAMS] = (size_t)t->nv * 4;
  }
  for (int w = 0; w < 2; ++w) {
    const auto &o = t->opt[w];
    const size_t n = w == XH_POLICY ? (size_t)t->np : (size_t)t->nv;
    if (o.kind == XH_OPT_SGD || !o.m || n == 0) continue;
    s.dev[XH_DIG_POLICY_OPT_M + 2 * w] = o.m;
    s.dev[XH_DIG_POLICY_OPT_V + 2 * w] = o.v;
    s.bytes[XH_DIG_POLICY_OPT_M + 2 * w] = s.bytes[XH_DIG_POLICY_OPT_V + 2 * w] = n * 4;
  }
  s.dev[XH_DIG_ENV_BINS] = t->bins + slot * N * t->BD();
  s.bytes[XH_DIG_ENV_BINS] = N * t->BD();
  s.dev[XH_DIG_ENV_ITEMS] = t->items + slot * N * 4;
  s.bytes[XH_DIG_ENV_ITEMS] = N * 4;
  s.dev[XH_DIG_RNG] = t->rng;
  s.bytes[XH_DIG_RNG] = N * 4;
  if (t->beta) {
    s.dev[XH_DIG_KL_BETA] = t->beta;
    s.bytes[XH_DIG_KL_BETA] = 4;
  }
  s.bytes[XH_SEC_OPT] = 2 * kOptRecordBytes;
  if (t->stats.ep_len) {
    s.dev[XH_SEC_EP_LEN] = t->stats.ep_len;
    s.bytes[XH_SEC_EP_LEN] = N * 4;
  }
  return s;
}

// Offsets of the present sections in id order; returns the blob's size.
size_t place(const Sections &s, size_t offset[XH_SEC_COUNT], uint32_t *count) {
  uint32_t n = 0;
  for (int id = 0; id < XH_SEC_COUNT; ++id) n += s.bytes[id] != 0;
  size_t at = blob::kHeaderBytes + (size_t)n * blob::kSectionBytes;
  for (int id = 0; id < XH_SEC_COUNT; ++id) {
    if (!s.bytes[id]) continue;
    at = blob::align_up(at);
    offset[id] = at;
    at += s.bytes[id];
  }
  *count = n;
  return at;
}

int digest_workspace(xh_trainer *t) {
  if (t->dig_ws) return XH_OK;
  void *p = nullptr;
  HIPCHK(hipMalloc(&p, (size_t)xh::kDigestWsWords * 8));
  t->allocs.push_back(p);
  t->dig_ws = static_cast<uint64_t *>(p);
  return XH_OK;
}

// Digests of n <= XH_DIG_COUNT device arrays, on the trainer's stream;
// synchronises.
int device_digests(xh_trainer *t, const xh::DigestTable &tab, uint64_t *out) {
  CHK(digest_workspace(t));
  hipStream_t s = t->ctx->stream;
  auto *ws = reinterpret_cast<unsigned long long *>(t->dig_ws);
  const hipError_t e = xh::launch_digest(tab, ws, s);
  if (e != hipSuccess)
    return fail(XH_ERR_HIP, "launch digest: %s", hipGetErrorString(e));
  HIPCHK(copy_to_host(out, xh::digest_results(ws), (size_t)XH_DIG_COUNT * 8, s));
  return XH_OK;
}

bool is_item(const xh_trainer *t, const int8_t *it) {
  bool a = true, b = true;
  for (int d = 0; d < t->cfg.dims; ++d) {
    a &= it[d] == t->env.item_a[d];
    b &= it[d] == t->env.item_b[d];
  }
  return a || b;
}

struct Field {
  const char *name;
  int blob, mine;
};

int first_mismatch(const Field *f, int n) {
  for (int k = 0; k < n; ++k)
    if (f[k].blob != f[k].mine)
      return fail(XH_ERR_INVALID, "load_state: %s differs: the blob has %d, this "
                  "trainer %d", f[k].name, f[k].blob, f[k].mine);
  return XH_OK;
}

int need(const blob::Parsed &p, uint32_t id, size_t bytes,
         const xh_state_section **out) {
  const xh_state_section *s = p.find(id);
  if (!s)
    return fail(XH_ERR_INVALID, "load_state: the blob has no %s section",
                blob::section_name(id));
  if (s->bytes != bytes)
    return fail(XH_ERR_INVALID, "load_state: section %s has %llu bytes, this "
                "trainer's has %zu", blob::section_name(id),
                (unsigned long long)s->bytes, bytes);
  *out = s;
  return XH_OK;
}

// One upload of load_state and what the device digest of it has to be.
struct Upload {
  uint32_t id;
  void *dst;
  const unsigned char *src;
  size_t bytes;
  uint64_t digest;
};

}  // namespace

extern "C" {

size_t xh_trainer_state_bytes(const xh_trainer *t) {
  if (!t) return 0;
  size_t offset[XH_SEC_COUNT] = {};
  uint32_t n = 0;
  return place(sections_of(t), offset, &n);
}

int xh_trainer_save_state(xh_trainer *t, void *out, size_t cap, size_t *written) {
  return guard([&]() -> int {
    if (!t || !out) return fail(XH_ERR_INVALID, "save_state: null arg");
    if (t->rolled)
      return fail(XH_ERR_STATE, "save_state: a rollout window is waiting for its "
                  "learn() / forget(); a state is saved between iterations");
    const Sections sec = sections_of(t);
    size_t offset[XH_SEC_COUNT] = {};
    uint32_t n = 0;
    const size_t total = place(sec, offset, &n);
    if (cap < total)
      return fail(XH_ERR_INVALID, "save_state: %zu bytes given, the state has %zu",
                  cap, total);
    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    HIPCHK(hipStreamSynchronize(s));
    unsigned char *base = static_cast<unsigned char *>(out);
    std::memset(base, 0, total);
    for (int id = 0; id < XH_SEC_COUNT; ++id)
      if (sec.bytes[id] && sec.dev[id])
        HIPCHK(copy_to_host(base + offset[id], sec.dev[id], sec.bytes[id], s));
    // pending xh_trainer_set_env_state writes, as the next rollout applies them
    const size_t BD = t->BD(), D = (size_t)t->cfg.dims;
    for (const auto &kv : t->env_override) {
      const size_t e = (size_t)kv.first;
      std::memcpy(base + offset[XH_DIG_ENV_BINS] + e * BD, kv.second.data(), BD);
      unsigned char item[4] = {0, 0, 0, 0};
      std::memcpy(item, kv.second.data() + BD, D);
      std::memcpy(base + offset[XH_DIG_ENV_ITEMS] + e * 4, item, 4);
    }
    OptRecord rec[2] = {};
    for (int w = 0; w < 2; ++w) {
      const auto &o = t->opt[w];
      rec[w].kind = o.kind;
      rec[w].lr = o.lr;
      rec[w].wd = o.wd;
      rec[w].beta1 = o.beta1;
      rec[w].beta2 = o.beta2;
      rec[w].t = o.t;
    }
    std::memcpy(base + offset[XH_SEC_OPT], rec, sizeof rec);

    uint32_t k = 0;
    for (int id = 0; id < XH_SEC_COUNT; ++id) {
      if (!sec.bytes[id]) continue;
      xh_state_section row{};
      row.id = (uint32_t)id;
      row.offset = offset[id];
      row.bytes = sec.bytes[id];
      row.digest = xh::digest_host(base + offset[id], sec.bytes[id]);
      std::memcpy(base + blob::kHeaderBytes + (size_t)k++ * blob::kSectionBytes,
                  &row, sizeof row);
    }
    xh_state_header h{};
    h.magic = XH_STATE_MAGIC;
    h.version = XH_STATE_VERSION;
    h.header_bytes = (uint32_t)blob::kHeaderBytes;
    h.sections = n;
    h.total_bytes = total;
    h.payload_digest =
        xh::digest_host(base + blob::kHeaderBytes, total - blob::kHeaderBytes);
    h.cfg = t->cfg;
    std::memcpy(base, &h, sizeof h);
    if (written) *written = total;
    return XH_OK;
  });
}

int xh_trainer_load_state(xh_trainer *t, const void *data, size_t bytes, int what) {
  return guard([&]() -> int {
    if (!t || !data) return fail(XH_ERR_INVALID, "load_state: null arg");
    if (what != XH_STATE_ALL && what != XH_STATE_NETS)
      return fail(XH_ERR_INVALID, "load_state: what %d (XH_STATE_ALL or "
                  "XH_STATE_NETS)", what);
    // ---- everything below up to "accepted" reads only ----
    blob::Parsed p;
    char why[320];
    if (!blob::parse(data, bytes, &p, why, sizeof why))
      return fail(XH_ERR_INVALID, "load_state: %s", why);
    const xh_config &c = p.h.cfg, &m = t->cfg;
    const bool all = what == XH_STATE_ALL, pg = m.algo == XH_PG;
    if (all) {
      const Field f[] = {
          {"algo", c.algo, m.algo},
          {"bins", c.bins, m.bins},
          {"dims", c.dims, m.dims},
          {"steps", c.steps, m.steps},
          {"epochs", c.epochs, m.epochs},
          {"policy_h1", c.policy_h1, m.policy_h1},
          {"policy_h2", c.policy_h2, m.policy_h2},
          {"value_h1", pg ? 0 : c.value_h1, pg ? 0 : m.value_h1},
          {"value_h2", pg ? 0 : c.value_h2, pg ? 0 : m.value_h2},
          {"num_envs_global", c.num_envs_global, m.num_envs_global}};
      CHK(first_mismatch(f, (int)(sizeof f / sizeof f[0])));
      if (c.num_envs < 1 || c.env_offset < 0 || c.env_offset > m.env_offset ||
          (long)m.env_offset + m.num_envs > (long)c.env_offset + c.num_envs)
        return fail(XH_ERR_INVALID, "load_state: the blob holds envs [%d, %d), "
                    "this trainer needs [%d, %d)", c.env_offset,
                    c.env_offset + c.num_envs, m.env_offset,
                    m.env_offset + m.num_envs);
      if (t->rolled)
        return fail(XH_ERR_STATE, "load_state: a rollout window is waiting for "
                    "its learn() / forget(); a state is restored between "
                    "iterations");
    } else {
      const Field f[] = {
          {"algo family (XH_PG or not)", c.algo == XH_PG, pg},
          {"bins", c.bins, m.bins},
          {"dims", c.dims, m.dims},
          {"policy_h1", c.policy_h1, m.policy_h1},
          {"policy_h2", c.policy_h2, m.policy_h2},
          {"value_h1", pg ? 0 : c.value_h1, pg ? 0 : m.value_h1},
          {"value_h2", pg ? 0 : c.value_h2, pg ? 0 : m.value_h2}};
      CHK(first_mismatch(f, (int)(sizeof f / sizeof f[0])));
    }

    std::vector<Upload> up;
    auto whole = [&](const xh_state_section *s, void *dst) {
      up.push_back(Upload{s->id, dst, p.data(*s), (size_t)s->bytes, s->digest});
    };
    const xh_state_section *s = nullptr;
    CHK(need(p, XH_DIG_POLICY_PARAMS, (size_t)t->np * 4, &s));
    whole(s, t->pp);
    if (t->vp) {
      CHK(need(p, XH_DIG_VALUE_PARAMS, (size_t)t->nv * 4, &s));
      whole(s, t->vp);
    }
    CHK(need(p, XH_SEC_OPT, 2 * kOptRecordBytes, &s));
    OptRecord rec[2];
    std::memcpy(rec, p.data(*s), sizeof rec);
    const int nets = t->vp ? 2 : 1;
    const xh_state_section *mom[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    for (int w = 0; w < nets; ++w) {
      const OptRecord &r = rec[w];
      if (r.kind != XH_OPT_SGD && r.kind != XH_OPT_MOMENTUM && r.kind != XH_OPT_ADAM)
        return fail(XH_ERR_INVALID, "load_state: optimizer %d has kind %d", w, r.kind);
      if (r.kind != XH_OPT_SGD && r.wd != 0.0f)
        return fail(XH_ERR_INVALID, "load_state: optimizer %d: weight decay with "
                    "kind %d (an sgd parameter only)", w, r.kind);
      if (!std::isfinite(r.t) || r.t < 1.0f)
        return fail(XH_ERR_INVALID, "load_state: optimizer %d: step counter %g", w,
                    (double)r.t);
      if (r.kind == XH_OPT_SGD) continue;
      const size_t n = w == XH_POLICY ? (size_t)t->np : (size_t)t->nv;
      CHK(need(p, XH_DIG_POLICY_OPT_M + 2 * w, n * 4, &mom[w][0]));
      CHK(need(p, XH_DIG_POLICY_OPT_V + 2 * w, n * 4, &mom[w][1]));
    }
    const xh_state_section *beta = nullptr;
    if (t->beta && (all || p.find(XH_DIG_KL_BETA))) {
      CHK(need(p, XH_DIG_KL_BETA, 4, &beta));
      whole(beta, t->beta);
    }
    // the trainer's slice of the blob's envs
    const size_t N = t->N(), BD = t->BD(), Nb = (size_t)c.num_envs;
    const size_t skip = all ? (size_t)(m.env_offset - c.env_offset) : 0;
    const xh_state_section *ep = nullptr;
    bool wide = false;
    if (all) {
      auto slice = [&](const xh_state_section *sc, size_t per_env, void *dst) {
        if (Nb == N) return whole(sc, dst);
        const unsigned char *src = p.data(*sc) + skip * per_env;
        up.push_back(Upload{sc->id, dst, src, N * per_env,
                            xh::digest_host(src, N * per_env)});
      };
      CHK(need(p, XH_DIG_ENV_BINS, Nb * BD, &s));
      const int8_t *b = reinterpret_cast<const int8_t *>(p.data(*s)) + skip * BD;
      for (size_t i = 0; i < N * BD; ++i) {
        if (b[i] > kBinCapacity)
          return fail(XH_ERR_INVALID, "load_state: bin value %d above the "
                      "capacity %d", b[i], kBinCapacity);
        wide |= b[i] < -kBinCapacity;
      }
      slice(s, BD, t->bins);
      CHK(need(p, XH_DIG_ENV_ITEMS, Nb * 4, &s));
      const int8_t *it = reinterpret_cast<const int8_t *>(p.data(*s)) + skip * 4;
      for (size_t e = 0; e < N; ++e)
        if (!is_item(t, it + e * 4))
          return fail(XH_ERR_INVALID, "load_state: env %zu: item is not an "
                      "item-table entry", e);
      slice(s, 4, t->items);
      CHK(need(p, XH_DIG_RNG, Nb * 4, &s));
      for (size_t e = 0; e < N; ++e) {
        uint32_t x;
        std::memcpy(&x, p.data(*s) + (skip + e) * 4, 4);
        if (x == 0 || x >= 2147483647u)
          return fail(XH_ERR_INVALID, "load_state: env %zu: engine state %u is "
                      "no minstd_rand0 state", e, x);
      }
      slice(s, 4, t->rng);
      if (t->stats.ep_len && p.find(XH_SEC_EP_LEN)) {
        CHK(need(p, XH_SEC_EP_LEN, Nb * 4, &ep));
        for (size_t e = 0; e < N; ++e) {
          int32_t len;
          std::memcpy(&len, p.data(*ep) + (skip + e) * 4, 4);
          if (len < 0)
            return fail(XH_ERR_INVALID, "load_state: env %zu: episode length %d",
                        e, len);
        }
        slice(ep, 4, t->stats.ep_len);
      }
    }

    HIPCHK(hipSetDevice(t->ctx->device));
    hipStream_t st = t->ctx->stream;
    HIPCHK(hipStreamSynchronize(st));
    CHK(digest_workspace(t));
    // moments as xh_trainer_set_optimizer allocates them (kept once they exist)
    for (int w = 0; w < nets; ++w) {
      auto &o = t->opt[w];
      if (rec[w].kind == XH_OPT_SGD) continue;
      const size_t n = w == XH_POLICY ? (size_t)t->np : (size_t)t->nv;
      if (!o.m) {
        void *pm = nullptr, *pv = nullptr;
        HIPCHK(hipMalloc(&pm, n * 4));
        t->allocs.push_back(pm);
        HIPCHK(hipMalloc(&pv, n * 4));
        t->allocs.push_back(pv);
        o.m = static_cast<float *>(pm);
        o.v = static_cast<float *>(pv);
      }
      whole(mom[w][0], o.m);
      whole(mom[w][1], o.v);
    }

    // ---- accepted: the first write ----
    wrote(t, kWrotePolicy | kWroteValue | kWroteBatch);
    for (const Upload &u : up)
      HIPCHK(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, st));
    if (all && t->stats.ep_len && !ep)  // no lengths saved: episodes start anew
      HIPCHK(hipMemsetAsync(t->stats.ep_len, 0, N * 4, st));
    for (int w = 0; w < nets; ++w) {
      auto &o = t->opt[w];
      o.kind = rec[w].kind;
      o.lr = rec[w].lr;
      o.wd = rec[w].wd;
      o.beta1 = rec[w].beta1;
      o.beta2 = rec[w].beta2;
      o.t = rec[w].t;
      (w == XH_POLICY ? t->cfg.lr_policy : t->cfg.lr_value) = o.lr;
      (w == XH_POLICY ? t->cfg.wd_policy : t->cfg.wd_value) = o.wd;
    }
    if (all) {
      t->env_override.clear();
      t->need_shift = false;  // the states went to slot 0
      if (!pg) {
        // as do_rollout sizes them; slot 0 as the setters derive it: whole
        // item-table entries, wide where a bin lies below -capacity
        t->items_ok.resize(t->T() + 1, 0);
        t->bins_wide.resize(t->T() + 1, 0);
        t->items_ok[0] = 1;
        t->bins_wide[0] = wide ? 1 : 0;
      }
    }
    // the caller's (pageable) blob is read until here
    HIPCHK(hipStreamSynchronize(st));

    // every restored array digested where it landed, against the blob's digest
    for (size_t first = 0; first < up.size(); first += XH_DIG_COUNT) {
      xh::DigestTable tab{};
      const size_t cnt = std::min(up.size() - first, (size_t)XH_DIG_COUNT);
      for (size_t k = 0; k < cnt; ++k) {
        tab.e[k].ptr = up[first + k].dst;
        tab.e[k].bytes = up[first + k].bytes;
      }
      tab.n = (int)cnt;
      uint64_t got[XH_DIG_COUNT];
      CHK(device_digests(t, tab, got));
      for (size_t k = 0; k < cnt; ++k)
        if (got[k] != up[first + k].digest)
          return fail(XH_ERR_HIP, "load_state: section %s reads back with digest "
                      "%016llx on the device, the blob's is %016llx (an upload "
                      "did not land as ordered)",
                      blob::section_name(up[first + k].id),
                      (unsigned long long)got[k],
                      (unsigned long long)up[first + k].digest);
    }
    return XH_OK;
  });
}

int xh_state_describe(const void *data, size_t bytes, char *buf, size_t cap) {
  return guard([&]() -> int {
    if (!buf || cap == 0) return fail(XH_ERR_INVALID, "state_describe: null buffer");
    blob::Parsed p;
    char why[320];
    if (!blob::parse(data, bytes, &p, why, sizeof why))
      return fail(XH_ERR_INVALID, "%s", why);
    const std::string js = blob::describe(p);
    if (js.size() + 1 > cap)
      return fail(XH_ERR_INVALID, "state_describe: %zu bytes needed", js.size() + 1);
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return XH_OK;
  });
}

int xh_trainer_state_digest(xh_trainer *t, uint64_t *out) {
  return guard([&]() -> int {
    if (!t || !out) return fail(XH_ERR_INVALID, "state_digest: null arg");
    if (!t->env_override.empty())
      return fail(XH_ERR_STATE, "state_digest: %zu xh_trainer_set_env_state "
                  "overrides are pending; the device holds them after the next "
                  "rollout", t->env_override.size());
    HIPCHK(hipSetDevice(t->ctx->device));
    const Sections sec = sections_of(t);
    xh::DigestTable tab{};
    for (int id = 0; id < XH_DIG_COUNT; ++id) {
      tab.e[id].ptr = sec.bytes[id] ? sec.dev[id] : nullptr;
      tab.e[id].bytes = sec.bytes[id];
    }
    tab.n = XH_DIG_COUNT;
    uint64_t got[XH_DIG_COUNT];
    CHK(device_digests(t, tab, got));
    std::memcpy(out, got, sizeof got);
    return XH_OK;
  });
}

int xh_digest_host(const void *data, size_t bytes, uint64_t *out) {
  return guard([&]() -> int {
    if (!out || (!data && bytes))
      return fail(XH_ERR_INVALID, "digest_host: null arg");
    *out = xh::digest_host(data, bytes);
    return XH_OK;
  });
}

}  // extern "C"
