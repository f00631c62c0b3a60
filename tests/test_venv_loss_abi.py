"""CPU-side checks of the xh_venv_policy_loss ABI: the symbol, its struct and
its enumerators exist with their values, the Python mirror matches, and the
argument check that needs no device; no GPU compute."""
import ctypes as C
import os

from test_stats_abi import _header_enum

NAMES = ("ROWS", "SKIPPED", "LOGR_SUM", "LOGR_SQSUM", "K3_SUM", "CLIPPED",
         "SURR_SUM", "ENTROPY_SUM", "VERR_SUM", "VERR_SQSUM", "COUNT")


def test_header_declares_and_library_exports_the_call():
    from dependence_free_rl_amd import _lib
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    assert "xh_venv_policy_loss" in _lib.header_symbols()
    assert " T xh_venv_policy_loss\n" in out
    assert _lib.lib.xh_venv_policy_loss.argtypes is not None


def test_enumerators_and_their_mirror():
    from dependence_free_rl_amd import _lib
    import dependence_free_rl_amd as pkg
    enum = _header_enum("XH_VLOSS_")
    assert enum == {"XH_VLOSS_" + n: i for i, n in enumerate(NAMES)}
    assert enum["XH_VLOSS_COUNT"] == 10
    for name, v in enum.items():
        assert getattr(_lib, name[3:]) == v, name
        assert getattr(pkg, name[3:]) == v, name  # exported from the package


def test_struct_size_matches_the_mirror():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_venv_loss") == C.sizeof(_lib.VenvLoss)
    assert C.sizeof(_lib.VenvLoss) > 0


def test_null_venv_is_a_status_code():
    from dependence_free_rl_amd import _lib
    a = _lib.VenvLoss()
    assert _lib.lib.xh_venv_policy_loss(None, C.byref(a)) == \
        _lib.XH_ERR_INVALID
    assert b"null" in _lib.lib.xh_last_error()
    assert _lib.lib.xh_venv_policy_loss(None, None) == _lib.XH_ERR_INVALID


def test_python_method():
    import dependence_free_rl_amd as pkg
    assert callable(pkg.VecEnv.policy_loss)
