"""ABI of the record-reading value net (xh_net_forward_record /
xh_net_backward_record): the header's declarations with their signatures, the
library's exports, the ctypes prototypes, the Python methods and the status
codes of null arguments; no GPU compute."""
import ctypes as C
import inspect
import os
import re

CALLS = ("xh_net_forward_record", "xh_net_backward_record")


def _declaration(name):
    from dependence_free_rl_amd import _lib
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
    assert _declaration("xh_net_forward_record") == [
        "xh_net *n", "xh_venv *v", "int view", "const int32_t *rows_dev",
        "long first", "long count", "float *out_dev"]
    assert _declaration("xh_net_backward_record") == [
        "xh_net *n", "xh_venv *v", "int view", "const int32_t *rows_dev",
        "long first", "long count", "const float *dout_dev", "int accumulate"]
    vp = C.c_void_p
    assert _lib.lib.xh_net_forward_record.restype is C.c_int
    assert _lib.lib.xh_net_forward_record.argtypes == [
        vp, vp, C.c_int, vp, C.c_long, C.c_long, vp]
    assert _lib.lib.xh_net_backward_record.restype is C.c_int
    assert _lib.lib.xh_net_backward_record.argtypes == [
        vp, vp, C.c_int, vp, C.c_long, C.c_long, vp, C.c_int]


def test_the_python_methods_exist_with_their_arguments():
    import dependence_free_rl_amd as pkg
    fwd = inspect.signature(pkg.ValueNet.forward_record)
    assert list(fwd.parameters) == ["self", "venv", "view", "rows", "first",
                                    "count", "out"]
    assert [fwd.parameters[k].default for k in ("view", "rows", "first", "count",
                                                "out")] == ["state", None, 0,
                                                            None, None]
    bwd = inspect.signature(pkg.ValueNet.backward_record)
    assert list(bwd.parameters) == ["self", "venv", "dout", "view", "rows",
                                    "first", "count", "accumulate"]
    assert bwd.parameters["accumulate"].default is False
    # the policy has its table; only the value net reads the record
    assert not hasattr(pkg.PolicyNet, "forward_record")
    assert callable(pkg.VecEnv._record_rows)


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    buf = C.create_string_buffer(64)
    assert lib.xh_net_forward_record(None, None, 0, None, 0, 1, buf) == INV
    assert b"null net" in lib.xh_last_error()
    assert lib.xh_net_backward_record(None, None, 0, None, 0, 1, buf, 0) == INV
    assert b"null net" in lib.xh_last_error()
