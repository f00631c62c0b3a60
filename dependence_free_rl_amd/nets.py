"""Device-resident policy and value nets for VecEnv learners (xh_net_*).

PolicyNet is the reference's per-bin conv1d_1 chain 2D -> h1 -> relu -> h2 ->
relu -> 1, ValueNet its full-layer MLP 2BD -> v1 -> relu -> v2 -> relu -> 1,
both in the flat model::parameters() layout of a Trainer of the same shape:
``net.params = trainer.params(POLICY)`` and back.  forward / backward / step
are launches on the context's stream; array arguments are host numpy arrays
(staged into the net's device scratch, as VecEnv does) or integer device
pointers (used as they are)."""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import NET_GRAD, NET_M, NET_PARAMS, NET_POLICY, NET_V, NET_VALUE, check
from .trainer import init_policy, init_value
from .venv import VENV_OBS, VecEnv

_WHICH = {"params": NET_PARAMS, "grad": NET_GRAD, "m": NET_M, "v": NET_V}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Net:
    KIND = None

    def __init__(self, ctx, bins, dims, widths):
        self.ctx = ctx
        self.B, self.D = bins, dims
        self.widths = tuple(int(w) for w in widths)
        if len(self.widths) != 2:
            raise ValueError("widths: two hidden widths, got %r" % (widths,))
        self.h = C.c_void_p()
        self._dev = {}  # device scratch: name -> (address, bytes)
        check(_lib.lib.xh_net_create(ctx.h, self.KIND, bins, dims,
                                     self.widths[0], self.widths[1],
                                     C.byref(self.h)))
        self.num_params = int(_lib.lib.xh_net_num_params(self.h))

    # ---- shapes -----------------------------------------------------------
    def _obs_shape(self, rows):
        return (rows, self.B, 2 * self.D)

    def _out_shape(self, rows):
        raise NotImplementedError

    # ---- device scratch (VecEnv._scratch / _upload / _download) ----------
    def _scratch(self, name, nbytes):
        have = self._dev.get(name)
        if have and have[1] >= nbytes:
            return have[0]
        if have:
            check(_lib.tensor_free(self.ctx.h, have[0]))
            del self._dev[name]
        p = C.c_void_p()
        n = (max(nbytes, 16) + 3) // 4
        check(_lib.tensor_alloc(self.ctx.h, n, C.byref(p)))
        self._dev[name] = (p.value, 4 * n)
        return p.value

    def _upload(self, ptr, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        check(_lib.tensor_copy(self.ctx.h, ptr, _ptr(a), a.size, _lib.COPY_H2D))

    def _download(self, ptr, shape):
        out = np.zeros(shape, np.float32)
        if out.size:
            check(_lib.tensor_copy(self.ctx.h, _ptr(out), ptr, out.size,
                                   _lib.COPY_D2H))
        return out

    def _obs(self, obs, rows):
        """(device address, rows) of an observation argument."""
        if isinstance(obs, VecEnv):
            if (obs.B, obs.D) != (self.B, self.D):
                raise ValueError("the venv is %d bins x %d dims, the net %d x %d"
                                 % (obs.B, obs.D, self.B, self.D))
            return obs.device_ptr(VENV_OBS), obs.N if rows is None else rows
        if isinstance(obs, (int, np.integer)):
            if rows is None:
                raise ValueError("rows is needed with a device pointer")
            return int(obs), int(rows)
        a = np.ascontiguousarray(obs, np.float32)
        if a.ndim != 3 or a.shape[1:] != (self.B, 2 * self.D):
            raise ValueError("obs: shape %s, expected [rows]%s"
                             % (a.shape, self._obs_shape("")[1:]))
        rows = a.shape[0] if rows is None else int(rows)
        if rows > a.shape[0]:
            raise ValueError("obs: %d rows asked, %d given" % (rows, a.shape[0]))
        ptr = self._scratch("obs", a.nbytes)
        self._upload(ptr, a)
        return ptr, rows

    # ---- the net ---------------------------------------------------------------
    def forward(self, obs, rows=None, out=None):
        """xh_net_forward.  obs: a VecEnv (its XH_VENV_OBS block, num_envs
        rows), a host array [rows][B][2D] or an integer device pointer (with
        rows).  out: an integer device pointer that receives the result
        (nothing is returned), or None for a host array: policy [rows][B]
        logits, value [rows]."""
        ptr, rows = self._obs(obs, rows)
        shape = self._out_shape(rows)
        dst = out if out is not None else self._scratch(
            "out", int(np.prod(shape)) * 4)
        check(_lib.lib.xh_net_forward(self.h, ptr, rows, int(dst)))
        if out is not None:
            return None
        return self._download(dst, shape)

    def backward(self, obs, dout, rows=None, accumulate=False):
        """xh_net_backward: the parameter gradient of sum(dout * out) into
        `grad` (added to it when accumulate).  dout: a host array of the
        output's shape or an integer device pointer."""
        ptr, rows = self._obs(obs, rows)
        if isinstance(dout, (int, np.integer)):
            dptr = int(dout)
        else:
            d = np.ascontiguousarray(dout, np.float32)
            if d.shape != self._out_shape(rows):
                raise ValueError("dout: shape %s, expected %s"
                                 % (d.shape, self._out_shape(rows)))
            dptr = self._scratch("dout", d.nbytes)
            self._upload(dptr, d)
        check(_lib.lib.xh_net_backward(self.h, ptr, rows, dptr,
                                       1 if accumulate else 0))

    def set_optimizer(self, kind, lr, weight_decay=0.0, beta1=0.9,
                      beta2=0.999):
        """kind "sgd" | "momentum" | "adam" (xh_net_set_optimizer): zeroes the
        moments and the step counter."""
        check(_lib.lib.xh_net_set_optimizer(self.h, _lib.OPTIMIZERS[kind], lr,
                                            weight_decay, beta1, beta2))

    def step(self, max_norm=0.0, clip_log=None):
        """Clip `grad` to the global norm max_norm (0: no clipping) and apply
        the optimizer (xh_net_step).  clip_log: an integer device pointer to
        two doubles {norm, scale}, or True to get them back as a host pair."""
        if clip_log is True:
            p = self._scratch("clip_log", 16)
            check(_lib.lib.xh_net_step(self.h, max_norm, p))
            raw = self._download(p, (4,))
            return tuple(raw.view(np.float64))
        check(_lib.lib.xh_net_step(self.h, max_norm,
                                   None if clip_log is None else int(clip_log)))
        return None

    # ---- state -----------------------------------------------------------------
    def get(self, which):
        out = np.zeros(self.num_params, np.float32)
        check(_lib.lib.xh_net_get(self.h, _WHICH[which], _ptr(out), out.size))
        return out

    def set(self, which, arr):
        a = np.ascontiguousarray(arr, np.float32).reshape(-1)
        check(_lib.lib.xh_net_set(self.h, _WHICH[which], _ptr(a), a.size))

    params = property(lambda self: self.get("params"),
                      lambda self, a: self.set("params", a))
    grad = property(lambda self: self.get("grad"),
                    lambda self, a: self.set("grad", a))

    @property
    def moments(self):
        """(m, v): momentum's velocity / adam's first moment, adam's second."""
        return self.get("m"), self.get("v")

    @moments.setter
    def moments(self, mv):
        self.set("m", mv[0])
        self.set("v", mv[1])

    @property
    def step_count(self):
        t = C.c_long()
        check(_lib.lib.xh_net_get_step(self.h, C.byref(t)))
        return t.value

    @step_count.setter
    def step_count(self, t):
        check(_lib.lib.xh_net_set_step(self.h, int(t)))

    def device_ptr(self, which="params"):
        return _lib.lib.xh_net_device_ptr(self.h, _WHICH[which])

    def set_grid_cap(self, cap):
        """Test only: at most `cap` workgroups per policy launch (0: default)."""
        check(_lib.lib.xh_net_set_grid_cap(self.h, int(cap)))

    def info(self):
        buf = C.create_string_buffer(1024)
        check(_lib.lib.xh_net_info(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    def close(self):
        if self.h:
            for ptr, _ in self._dev.values():
                _lib.tensor_free(self.ctx.h, ptr)
            self._dev = {}
            check(_lib.lib.xh_net_destroy(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PolicyNet(_Net):
    """The per-bin policy: [rows][B][2D] observations -> [rows][B] logits."""
    KIND = NET_POLICY

    def __init__(self, ctx, bins, dims, widths=(128, 128)):
        super().__init__(ctx, bins, dims, widths)

    def _out_shape(self, rows):
        return (rows, self.B)

    def init(self, seed=0):
        """He initialisation, the reference's scheme for conv1d_1 layers:
        weights N(0, sqrt(2 / fan_in)), biases 0 (trainer.init_policy; drawn
        with numpy on the host, not the reference's stream)."""
        self.params = init_policy(self.D, self.widths[0], self.widths[1],
                                  seed=seed)


class LayerPolicyNet(PolicyNet):
    """The policy through the layer-by-layer launches (XH_NET_POLICY_LAYERS):
    every activation materialised in HBM.  The comparator the fused kernels
    are measured against (tools/venv_net_time.py), not a path to train on."""
    KIND = _lib.NET_POLICY_LAYERS


class ValueNet(_Net):
    """The full-layer value net: [rows][B][2D] observations -> [rows]."""
    KIND = NET_VALUE

    def __init__(self, ctx, bins, dims, widths=(64, 32)):
        super().__init__(ctx, bins, dims, widths)

    def _out_shape(self, rows):
        return (rows,)

    def init(self, seed=1):
        """The reference's full_layer scheme: weights N(0, 0.01), biases 0
        (trainer.init_value; drawn with numpy on the host)."""
        self.params = init_value(self.B, self.D, self.widths[0],
                                 self.widths[1], seed=seed)

    # ---- straight from a venv's recorded window (widths (64, 32)) ------------
    def forward_record(self, venv, view="state", rows=None, first=0,
                       count=None, out=None):
        """forward(venv.record_obs(view, rows, first, count)) without the
        observations (xh_net_forward_record): the fused kernel reads the int8
        record.  view, rows, first and count as VecEnv.record_obs.  out: an
        integer device pointer that receives the [count] values (nothing is
        returned), or None for a host array.  With out=None an index outside
        the view gives NaN in its entry."""
        view_id, rows_ptr, count = venv._record_rows("forward_record", view,
                                                     rows, first, count)
        dst = out
        if out is None:
            dst = self._scratch("out", count * 4)
            if count:
                self._upload(dst, np.full(count, np.nan, np.float32))
        check(_lib.lib.xh_net_forward_record(self.h, venv.h, view_id, rows_ptr,
                                             first, count, int(dst)))
        if out is not None:
            return None
        return self._download(dst, (count,))

    def backward_record(self, venv, dout, view="state", rows=None, first=0,
                        count=None, accumulate=False):
        """backward(venv.record_obs(view, rows, first, count), dout) without
        the observations (xh_net_backward_record).  dout: a host array [count]
        or an integer device pointer."""
        view_id, rows_ptr, count = venv._record_rows("backward_record", view,
                                                     rows, first, count)
        if isinstance(dout, (int, np.integer)):
            dptr = int(dout)
        else:
            d = np.ascontiguousarray(dout, np.float32)
            if d.shape != (count,):
                raise ValueError("dout: shape %s, expected %s"
                                 % (d.shape, (count,)))
            dptr = self._scratch("dout", d.nbytes)
            self._upload(dptr, d)
        check(_lib.lib.xh_net_backward_record(self.h, venv.h, view_id, rows_ptr,
                                              first, count, dptr,
                                              1 if accumulate else 0))
