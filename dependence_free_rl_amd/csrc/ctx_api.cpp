// ctx_api.cpp -- the calls of the C ABI that need no trainer: the error slot,
// version and runtime info, struct sizes, the context with its communicator,
// and the default configuration.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstring>

#include "../../include/xylo_hip.h"
#include "xh_host.h"

using namespace xh::host;

extern "C" {

const char *xh_last_error(void) { return g_err.c_str(); }
const char *xh_version(void) { return "xylo-hip 0.2 (gfx950)"; }

int xh_device_count(int *out) {
  return guard([&]() -> int {
    if (!out) return fail(XH_ERR_INVALID, "null out");
    *out = 0;
    HIPCHK(hipGetDeviceCount(out));
    return XH_OK;
  });
}

// Which HIP / RCCL shared objects this process actually bound (a process that
// loaded another copy under the same soname first, e.g. a framework's bundled
// runtime, makes the library bind that one).
int xh_runtime_info(char *buf, size_t cap) {
  return guard([&]() -> int {
    if (!buf || cap == 0) return fail(XH_ERR_INVALID, "null buffer");
    Dl_info hi{}, ri{};
    const char *hp = dladdr(reinterpret_cast<void *>(&hipRuntimeGetVersion), &hi) &&
                             hi.dli_fname ? hi.dli_fname : "?";
    const char *rp = dladdr(reinterpret_cast<void *>(&ncclAllReduce), &ri) &&
                             ri.dli_fname ? ri.dli_fname : "?";
    int hv = 0, rv = 0;
    (void)hipRuntimeGetVersion(&hv);
    (void)ncclGetVersion(&rv);
    const int n = std::snprintf(buf, cap,
                                "{\"libamdhip64\": \"%s\", \"hip_runtime\": %d, "
                                "\"librccl\": \"%s\", \"rccl_version\": %d}",
                                hp, hv, rp, rv);
    if (n < 0 || (size_t)n >= cap)
      return fail(XH_ERR_INVALID, "runtime info needs %d bytes", n + 1);
    return XH_OK;
  });
}

size_t xh_struct_size(const char *name) {
  if (!name) return 0;
  if (!std::strcmp(name, "xh_config")) return sizeof(xh_config);
  if (!std::strcmp(name, "xh_eval")) return sizeof(xh_eval);
  if (!std::strcmp(name, "xh_layer")) return sizeof(xh_layer);
  if (!std::strcmp(name, "xh_stat_row")) return XH_STAT_COUNT * sizeof(double);
  if (!std::strcmp(name, "xh_upd_row")) return XH_UPD_COUNT * sizeof(double);
  if (!std::strcmp(name, "xh_state_header")) return sizeof(xh_state_header);
  if (!std::strcmp(name, "xh_state_section")) return sizeof(xh_state_section);
  if (!std::strcmp(name, "xh_venv_adv")) return sizeof(xh_venv_adv);
  if (!std::strcmp(name, "xh_venv_loss")) return sizeof(xh_venv_loss);
  if (!std::strcmp(name, "xh_venv_loss_ext")) return sizeof(xh_venv_loss_ext);
  if (!std::strcmp(name, "xh_vep_row")) return XH_VEP_COUNT * sizeof(double);
  if (!std::strcmp(name, "xh_item_set")) return sizeof(xh_item_set);
  if (!std::strcmp(name, "xh_venv_table_info"))
    return sizeof(struct xh_venv_table_info);
  return 0;
}

int xh_comm_unique_id(void *out128) {
  return guard([&]() -> int {
    if (!out128) return fail(XH_ERR_INVALID, "null out");
    ncclUniqueId id;
    RCCLCHK(ncclGetUniqueId(&id));
    static_assert(sizeof(id) == 128, "nccl unique id size");
    std::memcpy(out128, &id, sizeof id);
    return XH_OK;
  });
}

int xh_ctx_create(int device, int rank, int world, const void *uid128,
                  xh_ctx **out) {
  return guard([&]() -> int {
    if (!out) return fail(XH_ERR_INVALID, "null out");
    if (world < 1 || rank < 0 || rank >= world)
      return fail(XH_ERR_INVALID, "bad rank %d / world %d", rank, world);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
      return fail(XH_ERR_INVALID, "device %d of %d", device, ndev);
    HIPCHK(hipSetDevice(device));
    auto *c = new xh_ctx;
    c->device = device;
    c->rank = rank;
    c->world = world;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      return fail(XH_ERR_HIP, "stream: %s", hipGetErrorString(e));
    }
    // a communicator for world > 1, and for world == 1 when a unique id is
    // given (a one-rank RCCL comm: the multi-GPU code path on one device)
    if (world > 1 || uid128) {
      if (!uid128) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(XH_ERR_INVALID, "world > 1 needs the RCCL unique id");
      }
      ncclUniqueId id;
      std::memcpy(&id, uid128, sizeof id);
      ncclResult_t r = ncclCommInitRank(&c->comm, world, id, rank);
      if (r != ncclSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(XH_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
      }
    }
    *out = c;
    return XH_OK;
  });
}

// A context outlives its trainers: destroying it with live trainers defers
// the release to the last xh_trainer_destroy.
int xh_ctx_destroy(xh_ctx *c) {
  return guard([&]() -> int {
    if (!c) return XH_OK;
    if (c->trainers > 0) {
      c->closing = true;
      return XH_OK;
    }
    ctx_free(c);
    return XH_OK;
  });
}

int xh_ctx_synchronize(xh_ctx *c) {
  return guard([&]() -> int {
    if (!c) return fail(XH_ERR_INVALID, "null ctx");
    HIPCHK(hipStreamSynchronize(c->stream));
    return XH_OK;
  });
}

int xh_ctx_allreduce_host(xh_ctx *c, float *data, size_t n) {
  return guard([&]() -> int {
    if (!c || (!data && n)) return fail(XH_ERR_INVALID, "null arg");
    if (!c->comm || n == 0) return XH_OK;
    float *d = nullptr;
    HIPCHK(hipMalloc(&d, n * sizeof(float)));
    // the device buffer is freed on every path (the stream drained first)
    int st = copy_ok(copy_to_device(d, data, n * sizeof(float), c->stream));
    if (st == XH_OK) {
      const ncclResult_t r =
          ncclAllReduce(d, d, n, ncclFloat32, ncclSum, c->comm, c->stream);
      if (r != ncclSuccess)
        st = fail(XH_ERR_RCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
    }
    if (st == XH_OK)
      st = copy_ok(copy_to_host(data, d, n * sizeof(float), c->stream));
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (st == XH_OK && se != hipSuccess)
      st = fail(XH_ERR_HIP, "synchronize: %s", hipGetErrorString(se));
    (void)hipFree(d);
    return st;
  });
}

int xh_ctx_inject_fault(xh_ctx *c, int kind) {
  return guard([&]() -> int {
    if (!c) return fail(XH_ERR_INVALID, "null ctx");
    if (kind != XH_FAULT_NONE && kind != XH_FAULT_RCCL_ARG)
      return fail(XH_ERR_INVALID, "unknown fault %d", kind);
    if (kind == XH_FAULT_RCCL_ARG && !c->comm)
      return fail(XH_ERR_STATE, "inject_fault: the context has no communicator");
    c->fault = kind;
    return XH_OK;
  });
}

void xh_config_default(xh_config *c, int algo, int bins, int dims, int num_envs,
                       int steps) {
  std::memset(c, 0, sizeof *c);
  c->algo = algo;
  c->num_envs = c->num_envs_global = num_envs;
  c->env_offset = 0;
  c->bins = bins;
  c->dims = dims;
  c->steps = steps;
  c->epochs = algo == XH_AC ? 1 : 4;
  c->policy_h1 = 128;
  c->policy_h2 = algo == XH_AC ? 32 : 64;
  if (algo == XH_AC) c->policy_h1 = 64;
  c->value_h1 = 64;
  c->value_h2 = 32;
  // ppo_training.cc:17,26 / ac_training.cc:17,26
  c->lr_policy = algo == XH_AC ? 1e-5f : 1e-4f;
  c->lr_value = algo == XH_AC ? 1e-4f : 1e-5f;
  if (algo == XH_KLPPO) c->wd_policy = 1e-5f;  // ppo2_training.cc:20
  if (algo == XH_PG) {  // pg_training.cc:10-20: full 4B->256->128->B, 1e-4
    c->policy_h1 = 256;
    c->policy_h2 = 128;
    c->epochs = 1;
    c->lr_policy = 1e-4f;
    c->lr_value = 0.0f;
  }
  c->gamma = 0.99f;
  c->lambda = 0.95f;
  c->clip_eps = 0.2f;
  c->rng_state = 1;
  c->kl_beta = 1.0f;
  c->kl_target = 1e-9f;
}

}  // extern "C"
