"""CPU-side checks of the update-diagnostics ABI (xh_trainer_set_update_diag
and its four readers, the XH_UPD_* row layout); no GPU compute."""
import ctypes as C
import os
import re

CALLS = ("xh_trainer_set_update_diag", "xh_trainer_update_diag_count",
         "xh_trainer_get_update_diag", "xh_trainer_get_update_diag_rows",
         "xh_trainer_update_diag_info")


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
    for s in CALLS:
        assert s in syms, "%s is not declared in xylo_hip.h" % s
        assert (" T %s\n" % s) in out, "%s is not exported" % s
        assert getattr(_lib.lib, s).argtypes is not None, s


def test_python_indices_mirror_the_header_enum():
    from dependence_free_rl_amd import _lib
    enum = _header_enum("XH_UPD_")
    assert enum["XH_UPD_COUNT"] == len(enum) - 1 == 9
    mirror = {k: v for k, v in vars(_lib).items() if k.startswith("UPD_")}
    assert {"XH_" + k: v for k, v in mirror.items()} == enum
    # the statistics row did not grow, and its enum does not hold these
    assert not any(k.startswith("XH_UPD_") for k in _header_enum("XH_STAT_"))
    # the package re-exports every index and the Trainer methods
    import dependence_free_rl_amd as pkg
    for k, v in mirror.items():
        assert getattr(pkg, k) == v, k
    for m in ("set_update_diag", "update_diag_count", "update_diag",
              "update_diag_rows", "update_diag_info", "update_curve"):
        assert callable(getattr(pkg.Trainer, m)), m


def test_row_size_is_reported():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_upd_row") == 72 == _lib.UPD_COUNT * 8


def test_null_trainer_is_a_status_code():
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    n = C.c_long(-1)
    row = (C.c_double * _lib.UPD_COUNT)(*([-1.0] * _lib.UPD_COUNT))
    p = (C.c_float * 4)(*([-1.0] * 4))
    h = (C.c_double * 4)(*([-1.0] * 4))
    kl = (C.c_double * 4)(*([-1.0] * 4))
    buf = C.create_string_buffer(b"untouched", 64)
    assert lib.xh_trainer_set_update_diag(None, 8, 1) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert lib.xh_trainer_update_diag_count(None, C.byref(n)) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert n.value == -1
    assert lib.xh_trainer_get_update_diag(None, 0, 1, row) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert list(row) == [-1.0] * _lib.UPD_COUNT
    assert lib.xh_trainer_get_update_diag_rows(None, p, h, kl, 4) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert list(p) == [-1.0] * 4 and list(h) == [-1.0] * 4 and list(kl) == [-1.0] * 4
    assert lib.xh_trainer_update_diag_info(None, buf, len(buf)) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert buf.value == b"untouched"
