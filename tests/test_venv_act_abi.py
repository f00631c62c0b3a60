"""CPU-side checks of the xh_venv_act / trajectory-record ABI: the symbols and
enumerators exist, the earlier enumerators keep their values, and the
argument checks that need no device; no GPU compute."""
import ctypes as C
import os

from test_stats_abi import _header_enum

CALLS = ("xh_venv_act", "xh_venv_set_record", "xh_venv_record_pos",
         "xh_venv_record_rewind", "xh_venv_record_bytes", "xh_venv_record_ptr",
         "xh_venv_get_record")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for s in CALLS:
        assert s in syms, "%s is not declared in xylo_hip.h" % s
        assert (" T %s\n" % s) in out, "%s is not exported" % s
        assert getattr(_lib.lib, s).argtypes is not None, s


def test_venv_buffer_enumerators_keep_their_values():
    from dependence_free_rl_amd import _lib
    enum = _header_enum("XH_VENV_")
    assert [enum[k] for k in ("XH_VENV_ACTIONS", "XH_VENV_REWARD",
                              "XH_VENV_DONE", "XH_VENV_BINS", "XH_VENV_ITEMS",
                              "XH_VENV_RNG", "XH_VENV_OBS", "XH_VENV_MASK")] \
        == list(range(8))
    # the new buffers follow XH_VENV_MASK
    assert (enum["XH_VENV_POLICY"], enum["XH_VENV_PCHOICE"],
            enum["XH_VENV_BUF_COUNT"]) == (8, 9, 10)
    mirror = {"XH_" + k: v for k, v in vars(_lib).items()
              if k.startswith("VENV_")}
    enum.pop("XH_VENV_BUF_COUNT")
    assert mirror == enum


def test_act_and_record_enumerators():
    from dependence_free_rl_amd import _lib
    import dependence_free_rl_amd as pkg
    act = _header_enum("XH_ACT_")
    assert act == {"XH_ACT_PROBS": 0, "XH_ACT_LOGITS": 1, "XH_ACT_SAMPLE": 0,
                   "XH_ACT_ARGMAX": 1}
    rec = _header_enum("XH_VREC_")
    assert rec == {"XH_VREC_ACTION": 0, "XH_VREC_PCHOICE": 1,
                   "XH_VREC_REWARD": 2, "XH_VREC_DONE": 3, "XH_VREC_BINS": 4,
                   "XH_VREC_ITEMS": 5, "XH_VREC_COUNT": 6}
    for name, v in list(act.items()) + list(rec.items()):
        assert getattr(_lib, name[3:]) == v, name
        assert getattr(pkg, name[3:]) == v, name  # exported from the package
    assert (pkg.VENV_POLICY, pkg.VENV_PCHOICE) == (8, 9)
    for m in ("act", "set_record", "record", "rewind"):
        assert callable(getattr(pkg.VecEnv, m)), m


def test_null_handles_are_a_status_code():
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    assert lib.xh_venv_act(None, None, _lib.ACT_PROBS, _lib.ACT_SAMPLE, 0) == \
        _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert lib.xh_venv_set_record(None, 4, 1) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_record_rewind(None) == _lib.XH_ERR_INVALID
    pos = C.c_int(-1)
    assert lib.xh_venv_record_pos(None, C.byref(pos)) == _lib.XH_ERR_INVALID
    assert pos.value == -1
    buf = (C.c_float * 4)()
    assert lib.xh_venv_get_record(None, _lib.VREC_ACTION, buf, 16) == \
        _lib.XH_ERR_INVALID
    for which in range(-1, _lib.VREC_COUNT + 1):
        assert lib.xh_venv_record_bytes(None, which) == 0
        assert lib.xh_venv_record_ptr(None, which) is None
    assert lib.xh_venv_bytes(None, _lib.VENV_POLICY) == 0
    assert lib.xh_venv_device_ptr(None, _lib.VENV_PCHOICE) is None
