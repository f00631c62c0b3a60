// net_api.cpp -- device-resident policy and value nets for venv learners
// (include/xylo_hip.h, "device-resident nets"): an xh_net owns its parameters,
// gradient and optimizer state in HBM; forward, backward and step are launches
// on the context's stream with no host synchronisation.  The policy runs the
// fused kernels of net_kernels.hip; the value net composes the layer launches
// of dense_kernels.hip (the ones xh_model_forward / xh_model_gradient run) on
// device buffers -- or, for widths (64, 32), the fused kernels of
// net_value_kernels.hip straight on a venv's recorded window
// (xh_net_forward_record / xh_net_backward_record); step is the trainer's clip
// and optimizer launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "xh_host.h"
#include "xh_kernels.h"

using namespace xh::host;

struct xh_net {
  xh_ctx *ctx = nullptr;
  int kind = 0, B = 0, D = 0, h1 = 0, h2 = 0;
  int np = 0;
  float *buf[XH_NET_COUNT] = {};  // params, grad, m, v: np floats each
  float *tmp = nullptr;           // np floats: a backward's sum before it is added
  double *clip = nullptr;         // kClipMaxParts partials, then {norm, scale}
  int opt_kind = XH_OPT_SGD;
  float lr = 0.0f, wd = 0.0f, beta1 = 0.9f, beta2 = 0.999f;
  long t = 0;                     // steps taken
  int grid_cap = 0, cus = 1;
  // policy, and the value net on the record (allocated at its first
  // backward): one slab per workgroup of the backward
  float *slab = nullptr;
  int slab_stride = 0, slab_cap = 0;
  // value: activations, backprop ping-pong and split-K slabs for rows_cap rows
  long rows_cap = 0;
  float *vbuf = nullptr;
  int vstride = 0;
  // what the last forward / backward launched (xh_net_info)
  int grid_fwd = 0, grid_bwd = 0, slabs = 0;
  bool on_record = false;  // the last one was a *_record call
};

namespace {

int launched(hipError_t e, const char *what) {
  return e == hipSuccess ? XH_OK : fail(XH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

xh::PolicyLayout policy_layout(const xh_net *n) {
  return xh::PolicyLayout{2 * n->D, n->h1, n->h2};
}
// the layer-launch nets: the value net reads an observation row as one point
// of 2BD features; XH_NET_POLICY_LAYERS reads it as B points of 2D (conv1d_1 is
// the same Dense over rows * points, nn.h:127-186), the same flat layout
int net_points(const xh_net *n) { return n->kind == XH_NET_VALUE ? 1 : n->B; }
xh::ValueLayout value_layout(const xh_net *n) {
  return xh::ValueLayout{n->B * 2 * n->D / net_points(n), n->h1, n->h2};
}

// the value net's chain and where its dense layers' parameters start
struct ValueChain {
  xh::ModelLayer L[5];
  size_t poff[5];
  int width[6];
};
ValueChain value_chain(const xh_net *n) {
  const xh::ValueLayout VL = value_layout(n);
  ValueChain c;
  c.L[0] = xh::ModelLayer{xh::kLayerFull, VL.Fin, VL.V1};
  c.L[1] = xh::ModelLayer{xh::kLayerRelu, 0, 0};
  c.L[2] = xh::ModelLayer{xh::kLayerFull, VL.V1, VL.V2};
  c.L[3] = xh::ModelLayer{xh::kLayerRelu, 0, 0};
  c.L[4] = xh::ModelLayer{xh::kLayerFull, VL.V2, 1};
  const size_t po[5] = {(size_t)VL.oW1(), 0, (size_t)VL.oW2(), 0, (size_t)VL.ow3()};
  const int w[6] = {VL.Fin, VL.V1, VL.V1, VL.V2, VL.V2, 1};
  std::memcpy(c.poff, po, sizeof po);
  std::memcpy(c.width, w, sizeof w);
  return c;
}

// the value net's scratch for `rows` rows: [a1 r1 a2 r2 | bp bq | out | slabs]
struct ValueScratch {
  float *act[5];  // act[l] = the output of layer l - 1 (l >= 1)
  float *bp, *bq, *out, *slab;
};
ValueScratch value_scratch(const xh_net *n, long rows) {
  const size_t r = (size_t)rows, v1 = (size_t)n->h1, v2 = (size_t)n->h2;
  ValueScratch s;
  float *p = n->vbuf;
  s.act[0] = nullptr;
  s.act[1] = p, p += r * v1;
  s.act[2] = p, p += r * v1;
  s.act[3] = p, p += r * v2;
  s.act[4] = p, p += r * v2;
  s.bp = p, p += r * std::max(v1, v2);
  s.bq = p, p += r * std::max(v1, v2);
  s.out = p, p += (r + 63) & ~(size_t)63;
  s.slab = p;
  return s;
}
size_t value_scratch_floats(const xh_net *n, long rows) {
  const size_t r = (size_t)rows, v1 = (size_t)n->h1, v2 = (size_t)n->h2;
  return 2 * r * v1 + 2 * r * v2 + 2 * r * std::max(v1, v2) + ((r + 63) & ~(size_t)63) +
         (size_t)n->vstride * 64;  // layer_gradient_splits(...) <= 64
}

// Grows the value net's scratch to `rows` rows: outside the stream's critical
// path (one synchronisation, on the first call with more rows than before).
int value_reserve(xh_net *n, long rows) {
  if (rows <= n->rows_cap) return XH_OK;
  hipStream_t s = n->ctx->stream;
  HIPCHK(hipStreamSynchronize(s));
  if (n->vbuf) HIPCHK(hipFree(n->vbuf));
  n->vbuf = nullptr;
  n->rows_cap = 0;
  HIPCHK(hipMalloc((void **)&n->vbuf, 4 * value_scratch_floats(n, rows)));
  n->rows_cap = rows;
  return XH_OK;
}

int value_forward(xh_net *n, const float *obs, int rows, float *out) {
  hipStream_t s = n->ctx->stream;
  const ValueChain c = value_chain(n);
  const ValueScratch sc = value_scratch(n, n->rows_cap);
  const float *P = n->buf[XH_NET_PARAMS];
  const float *x = obs;
  for (int l = 0; l < 5; ++l) {
    float *y = l == 4 ? out : sc.act[l + 1];
    CHK(launched(xh::layer_forward(c.L[l], P + c.poff[l], x, rows, c.width[l], y, s),
                 "net_forward"));
    x = y;
  }
  return XH_OK;
}

// model::gradient's loop (nn.h:510-528) on the chain: gradient, then backward,
// from the last layer down; layer 0 gets its gradient only
int value_backward(xh_net *n, const float *obs, int rows, const float *dout, float *grad) {
  hipStream_t s = n->ctx->stream;
  const ValueChain c = value_chain(n);
  const ValueScratch sc = value_scratch(n, n->rows_cap);
  CHK(value_forward(n, obs, rows, sc.out));
  const float *P = n->buf[XH_NET_PARAMS];
  const float *bp = dout;
  float *free_a = sc.bp, *free_b = sc.bq;
  int splits = 0;
  for (int l = 4; l >= 0; --l) {
    const float *x = l == 0 ? obs : sc.act[l];
    CHK(launched(xh::layer_gradient(c.L[l], x, rows, c.width[l], bp, sc.slab, n->vstride,
                                    grad + c.poff[l], s),
                 "net_backward"));
    splits = std::max(splits, xh::layer_gradient_splits(c.L[l], rows, c.width[l]));
    if (l == 0) break;
    CHK(launched(xh::layer_backward(c.L[l], P + c.poff[l], x, rows, c.width[l], bp, free_a, s),
                 "net_backward"));
    bp = free_a;
    std::swap(free_a, free_b);
  }
  n->slabs = splits;
  return XH_OK;
}

int policy_grid(const xh_net *n, long R, int per_cu) {
  const long tiles = xh::net_policy_tiles(R);
  long g = (long)n->cus * per_cu;
  if (n->grid_cap > 0) g = std::min<long>(g, n->grid_cap);
  return (int)std::max<long>(1, std::min(g, tiles));
}

int check_which(const xh_net *n, int which, const char *who) {
  if (!n) return fail(XH_ERR_INVALID, "%s: null net", who);
  if (which < 0 || which >= XH_NET_COUNT)
    return fail(XH_ERR_INVALID, "%s: which %d", who, which);
  return XH_OK;
}

void net_free(xh_net *n) {
  (void)hipSetDevice(n->ctx->device);
  (void)hipStreamSynchronize(n->ctx->stream);
  for (float *p : n->buf)
    if (p) (void)hipFree(p);
  if (n->tmp) (void)hipFree(n->tmp);
  if (n->clip) (void)hipFree(n->clip);
  if (n->slab) (void)hipFree(n->slab);
  if (n->vbuf) (void)hipFree(n->vbuf);
  delete n;
}

}  // namespace

int xh_net_create(xh_ctx *ctx, int kind, int bins, int dims, int h1, int h2, xh_net **out) {
  return guard([&]() -> int {
    if (out) *out = nullptr;
    if (kind != XH_NET_POLICY && kind != XH_NET_VALUE && kind != XH_NET_POLICY_LAYERS)
      return fail(XH_ERR_INVALID, "net_create: kind %d", kind);
    if (dims < 1 || dims > 3 || !xh::venv_shape_supported(bins, dims))
      return fail(XH_ERR_INVALID, "net_create: shape %d bins x %d dims (bins in {8, 16, 32, "
                  "64, 128}, dims in {1, 2, 3})", bins, dims);
    if (kind == XH_NET_POLICY && !xh::net_policy_shape_supported(2 * dims, h1, h2))
      return fail(XH_ERR_INVALID, "net_create: policy widths [%d, %d] (one of [128,128], "
                  "[128,64], [64,64], [64,32])", h1, h2);
    if (kind != XH_NET_POLICY && (h1 < 1 || h2 < 1 || h1 > 4096 || h2 > 4096))
      return fail(XH_ERR_INVALID, "net_create: %s widths [%d, %d]",
                  kind == XH_NET_VALUE ? "value" : "layer-launch policy", h1, h2);
    if (!ctx || !out) return fail(XH_ERR_INVALID, "net_create: null arg");
    HIPCHK(hipSetDevice(ctx->device));
    xh_net *n = new xh_net;
    n->ctx = ctx;
    n->kind = kind;
    n->B = bins;
    n->D = dims;
    n->h1 = h1;
    n->h2 = h2;
    n->np = kind == XH_NET_POLICY ? policy_layout(n).size() : value_layout(n).size();
    hipStream_t s = ctx->stream;
    auto build = [&]() -> int {
      int cus = 0;
      HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
      n->cus = std::max(cus, 1);
      for (float *&p : n->buf) CHK(dev_zalloc(s, (void **)&p, (size_t)n->np * 4, "net_create"));
      CHK(dev_zalloc(s, (void **)&n->tmp, (size_t)n->np * 4, "net_create"));
      CHK(dev_zalloc(s, (void **)&n->clip, (xh::kClipMaxParts + 2) * sizeof(double),
                     "net_create"));
      if (kind == XH_NET_POLICY) {
        n->slab_stride = (n->np + 63) & ~63;
        n->slab_cap = n->cus;
        CHK(dev_zalloc(s, (void **)&n->slab, (size_t)n->slab_cap * n->slab_stride * 4,
                       "net_create"));
      } else {
        const xh::ValueLayout VL = value_layout(n);
        const int widest = std::max({VL.V1 * VL.Fin + VL.V1, VL.V2 * VL.V1 + VL.V2, VL.V2 + 1});
        n->vstride = (widest + 63) & ~63;
      }
      HIPCHK(hipStreamSynchronize(s));
      return XH_OK;
    };
    const int st = build();
    if (st != XH_OK) return fail_after(st, [&]() { net_free(n); });
    ++ctx->trainers;
    *out = n;
    return XH_OK;
  });
}

int xh_net_destroy(xh_net *n) {
  return guard([&]() -> int {
    if (!n) return XH_OK;
    xh_ctx *c = n->ctx;
    net_free(n);
    ctx_release(c, true);
    return XH_OK;
  });
}

size_t xh_net_num_params(const xh_net *n) { return n ? (size_t)n->np : 0; }

int xh_net_get(xh_net *n, int which, float *host, size_t count) {
  return guard([&]() -> int {
    CHK(check_which(n, which, "net_get"));
    if (!host || count != (size_t)n->np)
      return fail(XH_ERR_INVALID, "net_get: %zu floats, the net has %d", count, n->np);
    HIPCHK(hipSetDevice(n->ctx->device));
    return copy_ok(copy_to_host(host, n->buf[which], count * 4, n->ctx->stream));
  });
}

int xh_net_set(xh_net *n, int which, const float *host, size_t count) {
  return guard([&]() -> int {
    CHK(check_which(n, which, "net_set"));
    if (!host || count != (size_t)n->np)
      return fail(XH_ERR_INVALID, "net_set: %zu floats, the net has %d", count, n->np);
    HIPCHK(hipSetDevice(n->ctx->device));
    return copy_ok(copy_to_device(n->buf[which], host, count * 4, n->ctx->stream));
  });
}

float *xh_net_device_ptr(xh_net *n, int which) {
  return n && which >= 0 && which < XH_NET_COUNT ? n->buf[which] : nullptr;
}

int xh_net_get_step(xh_net *n, long *t) {
  return guard([&]() -> int {
    if (!n || !t) return fail(XH_ERR_INVALID, "net_get_step: null arg");
    *t = n->t;
    return XH_OK;
  });
}

int xh_net_set_step(xh_net *n, long t) {
  return guard([&]() -> int {
    if (!n) return fail(XH_ERR_INVALID, "net_set_step: null net");
    if (t < 0) return fail(XH_ERR_INVALID, "net_set_step: step %ld", t);
    n->t = t;
    return XH_OK;
  });
}

// rows of the call, checked: the flat per-bin rows and the value net's GEMM
// dimensions are ints
static int check_rows(const xh_net *n, long rows, const char *who) {
  if (rows < 1 || rows > (long)0x7fffffff / (n->B * 2 * n->D))
    return fail(XH_ERR_INVALID, "%s: %ld rows", who, rows);
  return XH_OK;
}

int xh_net_forward(xh_net *n, const float *obs_dev, long rows, float *out_dev) {
  return guard([&]() -> int {
    if (!n || !obs_dev || !out_dev) return fail(XH_ERR_INVALID, "net_forward: null arg");
    CHK(check_rows(n, rows, "net_forward"));
    HIPCHK(hipSetDevice(n->ctx->device));
    if (n->kind != XH_NET_POLICY) {
      const long m = rows * net_points(n);
      CHK(value_reserve(n, m));
      n->on_record = false;
      return value_forward(n, obs_dev, (int)m, out_dev);
    }
    xh::NetPolicyArgs a{};
    a.F0 = 2 * n->D, a.H1 = n->h1, a.H2 = n->h2;
    a.params = n->buf[XH_NET_PARAMS];
    a.obs = obs_dev;
    a.R = rows * n->B;
    a.logits = out_dev;
    n->grid_fwd = policy_grid(n, a.R, 2);
    return launched(xh::launch_net_policy_fwd(a, n->grid_fwd, n->ctx->stream), "net_forward");
  });
}

int xh_net_backward(xh_net *n, const float *obs_dev, long rows, const float *dout_dev,
                    int accumulate) {
  return guard([&]() -> int {
    if (!n || !obs_dev || !dout_dev) return fail(XH_ERR_INVALID, "net_backward: null arg");
    CHK(check_rows(n, rows, "net_backward"));
    HIPCHK(hipSetDevice(n->ctx->device));
    hipStream_t s = n->ctx->stream;
    float *dst = accumulate ? n->tmp : n->buf[XH_NET_GRAD];
    if (n->kind != XH_NET_POLICY) {
      const long m = rows * net_points(n);
      CHK(value_reserve(n, m));
      n->on_record = false;
      CHK(value_backward(n, obs_dev, (int)m, dout_dev, dst));
    } else {
      xh::NetPolicyArgs a{};
      a.F0 = 2 * n->D, a.H1 = n->h1, a.H2 = n->h2;
      a.params = n->buf[XH_NET_PARAMS];
      a.obs = obs_dev;
      a.R = rows * n->B;
      a.dout = dout_dev;
      a.slab = n->slab;
      a.slab_stride = n->slab_stride;
      n->grid_bwd = std::min(policy_grid(n, a.R, 1), n->slab_cap);
      n->slabs = n->grid_bwd;
      CHK(launched(xh::launch_net_policy_bwd(a, n->grid_bwd, s), "net_backward"));
      CHK(launched(xh::launch_slab_reduce(n->slab, n->grid_bwd, n->slab_stride, n->np, dst, s),
                   "net_backward"));
    }
    if (accumulate)  // grad[i] += this call's sum: one f32 add per entry
      CHK(launched(xh::launch_tensor_map(xh::kTensorAdd, n->buf[XH_NET_GRAD], n->tmp, 0.0f,
                                         n->buf[XH_NET_GRAD], n->np, s),
                   "net_backward"));
    return XH_OK;
  });
}

// ---- the value net on a venv's recorded window (net_value_kernels.hip) ----
namespace {

// the refusals of both calls and the launch's arguments; a->rec.count == 0:
// nothing to launch
int record_args(xh_net *n, xh_venv *v, const char *who, int view, const int32_t *rows_dev,
                long first, long count, xh::NetValueArgs *a) {
  if (!n) return fail(XH_ERR_INVALID, "%s: null net", who);
  if (n->kind != XH_NET_VALUE)
    return fail(XH_ERR_INVALID, "%s: the net is not a value net (XH_NET_VALUE); the policy "
                "reads observations or runs on the venv's logit table", who);
  if (n->h1 != xh::kNetValueV1 || n->h2 != xh::kNetValueV2)
    return fail(XH_ERR_INVALID, "%s: value widths [%d, %d], the fused kernels are built for "
                "[%d, %d] (other widths: xh_venv_record_obs and xh_net_forward / backward)",
                who, n->h1, n->h2, xh::kNetValueV1, xh::kNetValueV2);
  const int32_t *cap = nullptr;
  xh_ctx *vctx = nullptr;
  CHK(venv_record_rows(v, who, view, rows_dev, first, count, &a->rec, &cap, &vctx));
  if (a->rec.B != n->B || a->rec.D != n->D)
    return fail(XH_ERR_INVALID, "%s: the venv is %d bins x %d dims, the net %d x %d", who,
                a->rec.B, a->rec.D, n->B, n->D);
  if (vctx != n->ctx)
    return fail(XH_ERR_INVALID, "%s: the net and the venv live on different contexts", who);
  for (int d = 0; d < 4; ++d) a->cap[d] = d < n->D ? cap[d] : 1;
  a->params = n->buf[XH_NET_PARAMS];
  return XH_OK;
}

// tiles and CUs decide the grid, capped by xh_net_set_grid_cap
int record_grid(const xh_net *n, long count, int per_cu) {
  long g = (long)n->cus * per_cu;
  if (n->grid_cap > 0) g = std::min<long>(g, n->grid_cap);
  return (int)std::max<long>(1, std::min(g, xh::net_value_tiles(count)));
}

}  // namespace

int xh_net_forward_record(xh_net *n, xh_venv *v, int view, const int32_t *rows_dev, long first,
                          long count, float *out_dev) {
  return guard([&]() -> int {
    xh::NetValueArgs a{};
    CHK(record_args(n, v, "net_forward_record", view, rows_dev, first, count, &a));
    if (!out_dev) return fail(XH_ERR_INVALID, "net_forward_record: null out_dev");
    if (a.rec.count == 0) return XH_OK;
    HIPCHK(hipSetDevice(n->ctx->device));
    a.out = out_dev;
    n->grid_fwd = record_grid(n, count, 2);
    n->on_record = true;
    return launched(xh::launch_net_value_fwd(a, n->grid_fwd, n->ctx->stream),
                    "net_forward_record");
  });
}

int xh_net_backward_record(xh_net *n, xh_venv *v, int view, const int32_t *rows_dev, long first,
                           long count, const float *dout_dev, int accumulate) {
  return guard([&]() -> int {
    xh::NetValueArgs a{};
    CHK(record_args(n, v, "net_backward_record", view, rows_dev, first, count, &a));
    if (!dout_dev) return fail(XH_ERR_INVALID, "net_backward_record: null dout_dev");
    HIPCHK(hipSetDevice(n->ctx->device));
    hipStream_t s = n->ctx->stream;
    if (a.rec.count == 0) {  // an empty sum
      if (!accumulate) HIPCHK(hipMemsetAsync(n->buf[XH_NET_GRAD], 0, (size_t)n->np * 4, s));
      return XH_OK;
    }
    if (!n->slab) {  // at the first backward on the record, as value_reserve
      n->slab_stride = (n->np + 63) & ~63;
      HIPCHK(hipStreamSynchronize(s));
      CHK(dev_zalloc(s, (void **)&n->slab, (size_t)n->cus * n->slab_stride * 4,
                     "net_backward_record"));
      n->slab_cap = n->cus;
    }
    a.dout = dout_dev;
    a.slab = n->slab;
    a.slab_stride = n->slab_stride;
    n->grid_bwd = std::min(record_grid(n, count, 1), n->slab_cap);
    n->slabs = n->grid_bwd;
    n->on_record = true;
    float *dst = accumulate ? n->tmp : n->buf[XH_NET_GRAD];
    CHK(launched(xh::launch_net_value_bwd(a, n->grid_bwd, s), "net_backward_record"));
    CHK(launched(xh::launch_slab_reduce(n->slab, n->grid_bwd, n->slab_stride, n->np, dst, s),
                 "net_backward_record"));
    if (accumulate)  // grad[i] += this call's sum: one f32 add per entry
      CHK(launched(xh::launch_tensor_map(xh::kTensorAdd, n->buf[XH_NET_GRAD], n->tmp, 0.0f,
                                         n->buf[XH_NET_GRAD], n->np, s),
                   "net_backward_record"));
    return XH_OK;
  });
}

int xh_net_set_optimizer(xh_net *n, int kind, float lr, float weight_decay, float beta1,
                         float beta2) {
  return guard([&]() -> int {
    if (!n) return fail(XH_ERR_INVALID, "net_set_optimizer: null net");
    if (kind != XH_OPT_SGD && kind != XH_OPT_MOMENTUM && kind != XH_OPT_ADAM)
      return fail(XH_ERR_INVALID, "net_set_optimizer: kind %d", kind);
    if (kind != XH_OPT_SGD && weight_decay != 0.0f)
      return fail(XH_ERR_INVALID, "net_set_optimizer: weight decay is an sgd_optimizer "
                  "parameter only (nn.h:616-628)");
    HIPCHK(hipSetDevice(n->ctx->device));
    HIPCHK(hipMemsetAsync(n->buf[XH_NET_M], 0, (size_t)n->np * 4, n->ctx->stream));
    HIPCHK(hipMemsetAsync(n->buf[XH_NET_V], 0, (size_t)n->np * 4, n->ctx->stream));
    n->opt_kind = kind;
    n->lr = lr;
    n->wd = weight_decay;
    n->beta1 = beta1;
    n->beta2 = beta2;
    n->t = 0;
    return XH_OK;
  });
}

int xh_net_step(xh_net *n, float max_norm, double *clip_log_dev) {
  return guard([&]() -> int {
    if (!n) return fail(XH_ERR_INVALID, "net_step: null net");
    if (!(max_norm >= 0.0f) || std::isinf(max_norm))
      return fail(XH_ERR_INVALID, "net_step: max_norm %g (0, or a finite norm > 0)",
                  (double)max_norm);
    HIPCHK(hipSetDevice(n->ctx->device));
    hipStream_t s = n->ctx->stream;
    xh::OptStep st{n->opt_kind, n->lr, n->beta1, n->beta2, 1.0f, 1.0f, n->wd};
    if (n->opt_kind == XH_OPT_ADAM) {  // host float powf, as the reference (nn.h:684)
      st.c1 = 1 - powf(n->beta1, (float)(n->t + 1));
      st.c2 = 1 - powf(n->beta2, (float)(n->t + 1));
    }
    float *p = n->buf[XH_NET_PARAMS], *g = n->buf[XH_NET_GRAD];
    float *m = n->buf[XH_NET_M], *v = n->buf[XH_NET_V];
    if (max_norm > 0.0f) {
      double *log = clip_log_dev ? clip_log_dev : n->clip + xh::kClipMaxParts;
      CHK(launched(xh::launch_clip_sumsq(g, n->np, n->clip, s), "net_step"));
      CHK(launched(xh::launch_clip_step(n->clip, 1.0, max_norm, g, p, m, v, n->np, st, nullptr,
                                        log, s),
                   "net_step"));
    } else if (n->opt_kind == XH_OPT_SGD) {
      CHK(launched(xh::launch_sgd(p, g, n->np, st.lr, st.wd, s), "net_step"));
    } else {
      CHK(launched(xh::launch_opt(p, g, m, v, n->np, st, s), "net_step"));
    }
    n->t += 1;
    return XH_OK;
  });
}

int xh_net_set_grid_cap(xh_net *n, int cap) {
  return guard([&]() -> int {
    if (!n) return fail(XH_ERR_INVALID, "net_set_grid_cap: null net");
    if (cap < 0) return fail(XH_ERR_INVALID, "net_set_grid_cap: cap %d", cap);
    n->grid_cap = cap;
    return XH_OK;
  });
}

int xh_net_info(xh_net *n, char *buf, size_t cap) {
  return guard([&]() -> int {
    if (!n || !buf || !cap) return fail(XH_ERR_INVALID, "net_info: null arg");
    int len;
    if (n->kind == XH_NET_POLICY)
      len = std::snprintf(
          buf, cap,
          "{\"kind\": \"policy\", \"kernels\": [\"net_policy_fwd_kernel\", "
          "\"net_policy_bwd_kernel\", \"slab_reduce\"], \"math\": \"f32_mfma_16x16x4\", "
          "\"grid\": {\"forward\": %d, \"backward\": %d}, \"grid_cap\": %d, "
          "\"lds\": {\"forward\": %d, \"backward\": %d}, \"slabs\": %d}",
          n->grid_fwd, n->grid_bwd, n->grid_cap,
          xh::net_policy_lds_bytes(2 * n->D, n->h1, n->h2, 0),
          xh::net_policy_lds_bytes(2 * n->D, n->h1, n->h2, 1), n->slabs);
    else if (n->on_record)
      len = std::snprintf(
          buf, cap,
          "{\"kind\": \"value\", \"kernels\": [\"net_value_fwd_kernel\", "
          "\"net_value_bwd_kernel\", \"slab_reduce\"], \"math\": \"f32_mfma_16x16x4\", "
          "\"grid\": {\"forward\": %d, \"backward\": %d}, \"grid_cap\": %d, "
          "\"lds\": {\"forward\": %d, \"backward\": %d}, \"slabs\": %d}",
          n->grid_fwd, n->grid_bwd, n->grid_cap, xh::net_value_lds_bytes(0),
          xh::net_value_lds_bytes(1), n->slabs);
    else
      len = std::snprintf(
          buf, cap,
          "{\"kind\": \"%s\", \"kernels\": [\"layer_forward\", \"layer_gradient\", "
          "\"layer_backward\", \"slab_reduce\"], \"math\": \"f32_mfma_gemm\", "
          "\"grid\": {\"forward\": 0, \"backward\": 0}, \"grid_cap\": %d, "
          "\"lds\": {\"forward\": 0, \"backward\": 0}, \"slabs\": %d}",
          n->kind == XH_NET_VALUE ? "value" : "policy_layers", n->grid_cap, n->slabs);
    if (len < 0 || (size_t)len >= cap)
      return fail(XH_ERR_INVALID, "net_info: buffer of %zu bytes is too small", cap);
    return XH_OK;
  });
}
