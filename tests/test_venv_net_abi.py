"""ABI of the device-resident nets (xh_net_*): the header's declarations, the
library's exports, the ctypes prototypes, the enumerators, status codes for
bad arguments, and the parameter counts' formula; no GPU compute.  (That a
net's xh_net_num_params equals xh_trainer_num_params of a trainer of the same
shape needs a device: tests/test_gpu_venv_net.py.)"""
import ctypes as C
import os

from test_stats_abi import _header_enum

CALLS = ("xh_net_create", "xh_net_destroy", "xh_net_num_params", "xh_net_get",
         "xh_net_set", "xh_net_device_ptr", "xh_net_get_step",
         "xh_net_set_step", "xh_net_forward", "xh_net_backward",
         "xh_net_set_optimizer", "xh_net_step", "xh_net_set_grid_cap",
         "xh_net_info")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.xh_net_num_params.restype is C.c_size_t
    assert _lib.lib.xh_net_device_ptr.restype is C.c_void_p
    assert _lib.lib.xh_net_forward.argtypes == [C.c_void_p, C.c_void_p,
                                                C.c_long, C.c_void_p]
    assert _lib.lib.xh_net_backward.argtypes == [C.c_void_p, C.c_void_p,
                                                 C.c_long, C.c_void_p, C.c_int]


def test_enumerators_and_their_mirror():
    import dependence_free_rl_amd as pkg
    enum = _header_enum("XH_NET_")
    assert enum == {"XH_NET_POLICY": 0, "XH_NET_VALUE": 1,
                    "XH_NET_POLICY_LAYERS": 2, "XH_NET_PARAMS": 0,
                    "XH_NET_GRAD": 1, "XH_NET_M": 2, "XH_NET_V": 3,
                    "XH_NET_COUNT": 4}
    for k, v in enum.items():
        if k != "XH_NET_COUNT":
            assert getattr(pkg, k[3:]) == v, k
    assert callable(pkg.PolicyNet) and callable(pkg.ValueNet)
    for name in ("forward", "backward", "set_optimizer", "step", "device_ptr",
                 "info", "close", "init", "set_grid_cap"):
        assert callable(getattr(pkg.PolicyNet, name)), name
        assert callable(getattr(pkg.ValueNet, name)), name
    for name in ("params", "grad", "moments", "step_count"):
        assert isinstance(getattr(pkg.PolicyNet, name), property), name


def _create(kind, bins, dims, h1, h2, ctx=None):
    from dependence_free_rl_amd import _lib
    h = C.c_void_p(1)
    st = _lib.lib.xh_net_create(ctx, kind, bins, dims, h1, h2, C.byref(h))
    return st, h.value, _lib.lib.xh_last_error().decode()


def test_bad_shapes_and_widths_are_status_codes():
    """The shape is checked before anything touches a device, so a bad one is
    named even without a context."""
    from dependence_free_rl_amd import _lib
    INV = _lib.XH_ERR_INVALID
    for bins, dims in ((7, 2), (0, 2), (256, 2), (64, 0), (64, 4), (12, 1)):
        st, h, msg = _create(0, bins, dims, 128, 128)
        assert st == INV and h is None and "shape" in msg, (bins, dims, msg)
        st, h, msg = _create(1, bins, dims, 64, 32)
        assert st == INV and h is None and "shape" in msg, (bins, dims, msg)
    for h1, h2 in ((128, 32), (64, 128), (32, 32), (100, 100), (0, 0),
                   (256, 128), (128, 96)):
        st, h, msg = _create(0, 64, 2, h1, h2)
        assert st == INV and h is None and "policy widths" in msg, (h1, h2, msg)
    for h1, h2 in ((0, 32), (64, 0), (-1, 5)):
        st, h, msg = _create(1, 64, 2, h1, h2)
        assert st == INV and h is None and "value widths" in msg, (h1, h2, msg)
    for kind in (-1, 3):
        st, h, msg = _create(kind, 64, 2, 128, 128)
        assert st == INV and "kind" in msg
    # every supported shape gets past the shape checks (and stops at the
    # missing context)
    for bins in (8, 16, 32, 64, 128):
        for dims in (1, 2, 3):
            for h1, h2 in ((128, 128), (128, 64), (64, 64), (64, 32)):
                st, h, msg = _create(0, bins, dims, h1, h2)
                assert st == INV and msg == "net_create: null arg", msg
            st, h, msg = _create(1, bins, dims, 64, 32)
            assert st == INV and msg == "net_create: null arg", msg


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    buf = C.create_string_buffer(64)
    t = C.c_long()
    assert lib.xh_net_num_params(None) == 0
    assert lib.xh_net_device_ptr(None, 0) is None
    assert lib.xh_net_destroy(None) == _lib.XH_OK
    for call in (lambda: lib.xh_net_get(None, 0, buf, 16),
                 lambda: lib.xh_net_set(None, 0, buf, 16),
                 lambda: lib.xh_net_get_step(None, C.byref(t)),
                 lambda: lib.xh_net_set_step(None, 0),
                 lambda: lib.xh_net_forward(None, buf, 1, buf),
                 lambda: lib.xh_net_backward(None, buf, 1, buf, 0),
                 lambda: lib.xh_net_set_optimizer(None, 0, 0.1, 0, 0.9, 0.999),
                 lambda: lib.xh_net_step(None, 0.0, None),
                 lambda: lib.xh_net_set_grid_cap(None, 1),
                 lambda: lib.xh_net_info(None, buf, 64)):
        assert call() == INV
        assert lib.xh_last_error()


def test_parameter_count_formulas():
    """The flat layouts' sizes (PolicyLayout / ValueLayout), which a Trainer's
    parameters and a net's share."""
    from dependence_free_rl_amd import (init_policy, init_value,
                                        policy_param_count, value_param_count)
    assert policy_param_count(2, 128, 128) == 128 * 4 + 128 + 128 * 128 + 128 + 129
    assert init_policy(3, 64, 32).size == policy_param_count(3, 64, 32)
    assert init_value(16, 3, 64, 32).size == value_param_count(16, 3, 64, 32)
