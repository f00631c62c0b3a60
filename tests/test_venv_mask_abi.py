"""CPU-side checks of the VecEnv's invalid-action-masking ABI: the new calls
are declared, exported and typed, NULL arguments give status codes, the sets
the earlier calls pinned are as they were, and the Python methods and keywords
exist; no GPU compute."""
import ctypes as C
import inspect
import os
import re

from test_stats_abi import _header_enum

CALLS = ("xh_venv_legal_words", "xh_venv_set_action_mask", "xh_venv_legal",
         "xh_venv_legal_ptr", "xh_venv_record_legal_bytes",
         "xh_venv_record_legal_ptr", "xh_venv_get_record_legal",
         "xh_venv_policy_loss_masked")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.xh_venv_legal_ptr.restype is C.c_void_p
    assert _lib.lib.xh_venv_record_legal_ptr.restype is C.c_void_p
    assert _lib.lib.xh_venv_record_legal_bytes.restype is C.c_size_t


def test_the_library_exports_exactly_the_declared_calls():
    """Every xh_* call the header declares is defined by some object of the
    library, and nothing else is exported under that prefix."""
    from dependence_free_rl_amd import _lib
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    exported = sorted(set(re.findall(r" T (xh_[a-z0-9_]+)$", out, flags=re.M)))
    assert exported == _lib.header_symbols()


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    buf = C.create_string_buffer(64)
    assert lib.xh_venv_legal_words(None) == 0
    for call in (lambda: lib.xh_venv_set_action_mask(None, 1),
                 lambda: lib.xh_venv_set_action_mask(None, 0),
                 lambda: lib.xh_venv_legal(None, None),
                 lambda: lib.xh_venv_legal(None, buf),
                 lambda: lib.xh_venv_get_record_legal(None, buf, 64),
                 lambda: lib.xh_venv_policy_loss_masked(
                     None, C.byref(_lib.VenvLoss()), None)):
        assert call() == INV
        assert b"null" in lib.xh_last_error()
    assert lib.xh_venv_legal_ptr(None) is None
    assert lib.xh_venv_record_legal_bytes(None) == 0
    assert lib.xh_venv_record_legal_ptr(None) is None


def test_the_pinned_sets_are_as_before():
    from dependence_free_rl_amd import _lib
    assert len(_header_enum("XH_VREC_")) == 7    # 6 arrays + COUNT
    assert len(_header_enum("XH_VLOSS_")) == 11  # 10 sums + COUNT
    assert len(_header_enum("XH_VKL_")) == 4
    assert _header_enum("XH_VENV_BUF")["XH_VENV_BUF_COUNT"] == 10
    assert _lib.lib.xh_struct_size(b"xh_venv_loss") == C.sizeof(_lib.VenvLoss)
    assert C.sizeof(_lib.VenvLoss) == 176  # what it was before these calls
    names = [f[0] for f in _lib.VenvLoss._fields_]
    assert names[-5:] == ["accumulate", "distrib", "beta", "beta_dev",
                          "kl_stats"]


def test_python_methods_and_keywords():
    import dependence_free_rl_amd as pkg
    assert callable(pkg.VecEnv.set_action_mask)
    assert "on" in inspect.signature(pkg.VecEnv.set_action_mask).parameters
    legal = inspect.signature(pkg.VecEnv.legal).parameters
    assert legal["packed"].default is False
    loss = inspect.signature(pkg.VecEnv.policy_loss).parameters
    assert loss["legal"].default is None
    for name in ("legal_words", "pack_legal", "unpack_legal"):
        assert callable(getattr(pkg, name)), name
    assert [pkg.legal_words(B) for B in (8, 16, 32, 64, 128)] == [1, 1, 1, 2, 4]
