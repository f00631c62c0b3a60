"""CPU-side checks of the VecEnv's KL-PPO ABI: the distribution record's
calls, xh_venv_kl_beta and the XH_VKL_* enumerators exist with their values,
xh_venv_loss's mirror has the appended fields, and the argument checks that
need no device; no GPU compute."""
import ctypes as C
import os

from test_stats_abi import _header_enum

CALLS = ("xh_venv_set_record_distrib", "xh_venv_record_distrib_bytes",
         "xh_venv_record_distrib_ptr", "xh_venv_get_record_distrib",
         "xh_venv_kl_beta")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
        assert getattr(_lib.lib, name).argtypes is not None, name


def test_enumerators_and_their_mirror():
    from dependence_free_rl_amd import _lib
    import dependence_free_rl_amd as pkg
    enum = _header_enum("XH_VKL_")
    assert enum == {"XH_VKL_KL_SUM": 0, "XH_VKL_ROWS": 1, "XH_VKL_KL_SQSUM": 2,
                    "XH_VKL_COUNT": 3}
    for name, v in enum.items():
        assert getattr(_lib, name[3:]) == v, name
        assert getattr(pkg, name[3:]) == v, name  # exported from the package
    # the sets the earlier calls pinned are as they were
    assert len(_header_enum("XH_VREC_")) == 7    # 6 arrays + COUNT
    assert len(_header_enum("XH_VLOSS_")) == 11  # 10 sums + COUNT
    assert _header_enum("XH_VENV_BUF")["XH_VENV_BUF_COUNT"] == 10


def test_struct_mirror_has_the_appended_fields():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_venv_loss") == C.sizeof(_lib.VenvLoss)
    names = [f[0] for f in _lib.VenvLoss._fields_]
    assert names[-5:] == ["accumulate", "distrib", "beta", "beta_dev",
                          "kl_stats"]
    a = _lib.VenvLoss()  # zeroed: the calls behave as before
    assert not a.distrib and a.beta == 0.0 and not a.beta_dev
    assert not a.kl_stats


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    assert lib.xh_venv_set_record_distrib(None, 1) == INV
    assert b"null" in lib.xh_last_error()
    assert lib.xh_venv_record_distrib_bytes(None) == 0
    assert lib.xh_venv_record_distrib_ptr(None) is None
    buf = C.create_string_buffer(16)
    assert lib.xh_venv_get_record_distrib(None, buf, 16) == INV
    assert lib.xh_venv_kl_beta(None, buf, 0.01, buf, None) == INV
    assert b"null" in lib.xh_last_error()


def test_python_methods():
    import inspect

    import dependence_free_rl_amd as pkg
    assert callable(pkg.VecEnv.kl_beta)
    assert "distrib" in inspect.signature(pkg.VecEnv.set_record).parameters
    params = inspect.signature(pkg.VecEnv.policy_loss).parameters
    for name in ("beta", "distrib", "want_kl"):
        assert name in params, name
