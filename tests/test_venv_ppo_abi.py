"""CPU-side checks of xh_venv_policy_loss_ex's ABI (the entropy bonus and the
clipped value loss of the VecEnv loss head): the call is declared, exported
and typed, its enum and struct have their mirrors, xh_venv_loss is as it was,
NULL arguments give status codes, and VecEnv.policy_loss has the keywords; no
GPU compute."""
import ctypes as C
import inspect
import os

from test_stats_abi import _header_enum


def test_header_declares_and_library_exports_the_call():
    from dependence_free_rl_amd import _lib
    name = "xh_venv_policy_loss_ex"
    assert name in _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    assert (" T %s\n" % name) in out
    f = getattr(_lib.lib, name)
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.POINTER(_lib.VenvLoss),
                          C.POINTER(_lib.VenvLossExt)]


def test_enum_and_struct_mirrors():
    import dependence_free_rl_amd as pkg
    from dependence_free_rl_amd import _lib
    names = ("ROWS", "ENTROPY_SUM", "VCLIP_ROWS", "VLOSS_SUM", "COUNT")
    enum = _header_enum("XH_VEXT_")
    assert enum == {"XH_VEXT_" + n: k for k, n in enumerate(names)}
    for k, n in enumerate(names):
        assert getattr(_lib, "VEXT_" + n) == k
        assert getattr(pkg, "VEXT_" + n) == k
    assert (_lib.lib.xh_struct_size(b"xh_venv_loss_ext") ==
            C.sizeof(_lib.VenvLossExt) == 56)
    assert [f[0] for f in _lib.VenvLossExt._fields_] == [
        "masked", "legal_dev", "ent_coef", "ent_coef_dev", "v_old", "vclip",
        "ext_stats"]
    # the frozen ones
    assert _lib.lib.xh_struct_size(b"xh_venv_loss") == C.sizeof(_lib.VenvLoss)
    assert C.sizeof(_lib.VenvLoss) == 176
    assert len(_header_enum("XH_VLOSS_")) == 11
    assert len(_header_enum("XH_VKL_")) == 4


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    a, x = _lib.VenvLoss(), _lib.VenvLossExt()
    for call in (lambda: lib.xh_venv_policy_loss_ex(None, None, None),
                 lambda: lib.xh_venv_policy_loss_ex(None, C.byref(a), None),
                 lambda: lib.xh_venv_policy_loss_ex(None, C.byref(a),
                                                    C.byref(x))):
        assert call() == INV
        assert b"null" in lib.xh_last_error()


def test_python_keywords_and_defaults():
    import dependence_free_rl_amd as pkg
    loss = inspect.signature(pkg.VecEnv.policy_loss).parameters
    assert loss["ent_coef"].default == 0.0
    assert isinstance(loss["ent_coef"].default, float)
    assert loss["v_old"].default is None
    assert loss["vclip"].default is None
    assert loss["want_ext"].default is False
    assert loss["legal"].default is None  # as before
