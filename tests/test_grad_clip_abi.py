"""CPU-side checks of the gradient-clipping ABI (xh_trainer_set_grad_clip /
xh_trainer_get_grad_clip_log / xh_clip_grad_norm and the XH_STAT_* entries
they added); no GPU compute."""
import ctypes as C
import os

from test_stats_abi import _header_enum

CALLS = ("xh_trainer_set_grad_clip", "xh_trainer_get_grad_clip_log",
         "xh_clip_grad_norm")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for s in CALLS:
        assert s in syms, "%s is not declared in xylo_hip.h" % s
        assert (" T %s\n" % s) in out, "%s is not exported" % s
        assert getattr(_lib.lib, s).argtypes is not None, s


def test_package_exposes_the_python_calls():
    import dependence_free_rl_amd as pkg
    assert callable(pkg.clip_grad_norm)
    assert callable(pkg.Trainer.set_grad_clip)
    assert callable(pkg.Trainer.grad_clip_log)


def test_null_handles_are_a_status_code():
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    assert lib.xh_trainer_set_grad_clip(None, _lib.XH_POLICY, 1.0) == \
        _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    rows = C.c_int(-1)
    out = (C.c_double * 8)()
    assert lib.xh_trainer_get_grad_clip_log(
        None, _lib.XH_POLICY, out, 4, C.byref(rows)) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert rows.value == -1
    g = (C.c_float * 4)(1, 2, 3, 4)
    norm, scale = C.c_double(-1), C.c_float(-1)
    assert lib.xh_clip_grad_norm(None, g, 4, 1.0, C.byref(norm),
                                 C.byref(scale)) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert (norm.value, scale.value, list(g)) == (-1, -1, [1, 2, 3, 4])


def test_stat_indices_mirror_the_header_enum():
    from dependence_free_rl_amd import _lib
    import dependence_free_rl_amd as pkg
    enum = _header_enum("XH_STAT_")
    assert enum["XH_STAT_COUNT"] == 21 == len(enum) - 1
    mirror = {k: v for k, v in vars(_lib).items() if k.startswith("STAT_")}
    assert {"XH_" + k: v for k, v in mirror.items()} == enum
    # the earlier entries keep their values, the new ones follow KL_MEAN
    assert (_lib.STAT_ITER, _lib.STAT_KL_MEAN) == (0, 17)
    assert (_lib.STAT_PCLIP_STEPS, _lib.STAT_PCLIP_SCALE_MIN,
            _lib.STAT_VCLIP_SCALE) == (18, 19, 20)
    for k, v in mirror.items():
        assert getattr(pkg, k) == v, k
    assert _lib.lib.xh_struct_size(b"xh_stat_row") == 21 * 8
