"""CPU-side checks of the training-statistics ABI (xh_trainer_set_stats /
stats_count / get_stats and the XH_STAT_* row layout); no GPU compute."""
import ctypes as C
import os
import re


def _header_enum(prefix):
    """{name: value} of the header's enumerators starting with `prefix`
    (explicit values, or the previous one + 1)."""
    from dependence_free_rl_amd import _lib
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for body in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S):
        if prefix not in body:
            continue
        nxt = 0
        for item in body.split(","):
            m = re.match(r"\s*(\w+)\s*(?:=\s*(\d+))?\s*$", item)
            if not m:
                continue
            nxt = int(m.group(2)) if m.group(2) is not None else nxt
            if m.group(1).startswith(prefix):
                out[m.group(1)] = nxt
            nxt += 1
    return out


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for s in ("xh_trainer_set_stats", "xh_trainer_stats_count",
              "xh_trainer_get_stats"):
        assert s in syms, "%s is not declared in xylo_hip.h" % s
        assert (" T %s\n" % s) in out, "%s is not exported" % s
        assert getattr(_lib.lib, s).argtypes is not None, s


def test_python_indices_mirror_the_header_enum():
    from dependence_free_rl_amd import _lib
    enum = _header_enum("XH_STAT_")
    assert enum["XH_STAT_COUNT"] == len(enum) - 1 >= 18
    mirror = {k: v for k, v in vars(_lib).items() if k.startswith("STAT_")}
    assert {"XH_" + k: v for k, v in mirror.items()} == enum
    # the package re-exports every index
    import dependence_free_rl_amd as pkg
    for k, v in mirror.items():
        assert getattr(pkg, k) == v, k


def test_row_size_is_reported():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_stat_row") == _lib.STAT_COUNT * 8


def test_null_trainer_is_a_status_code():
    from dependence_free_rl_amd import _lib
    n = C.c_long(-1)
    row = (C.c_double * _lib.STAT_COUNT)()
    assert _lib.lib.xh_trainer_set_stats(None, 8) == _lib.XH_ERR_INVALID
    assert b"null" in _lib.lib.xh_last_error()
    assert _lib.lib.xh_trainer_stats_count(None, C.byref(n)) == _lib.XH_ERR_INVALID
    assert n.value == -1
    assert _lib.lib.xh_trainer_get_stats(None, 0, 1, row) == _lib.XH_ERR_INVALID
