"""CPU-side checks of the logit-table ABI (xh_venv_table_*): the calls are
declared and exported, the Python binding's prototypes and struct mirror are
the header's, xh_item_set_table_info equals tests/venv_table_ref.py and
refuses an invalid set and a domain past XH_VTAB_MAX_ENTRIES; no GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import venv_table_ref as tr
from test_venv_table_ref import SETS

CALLS = {
    "xh_item_set_table_info": ["const xh_item_set *", "int", "int",
                               "struct xh_venv_table_info *"],
    "xh_venv_table_info": ["const xh_venv *", "struct xh_venv_table_info *"],
    "xh_venv_table_obs": ["xh_venv *", "float *"],
    "xh_venv_act_table": ["xh_venv *", "const float *", "int", "int"],
    "xh_venv_table_gather": ["xh_venv *", "const float *", "const int32_t *",
                             "long", "long", "float *"],
    "xh_venv_table_grad": ["xh_venv *", "const int32_t *", "long", "long",
                           "const float *", "float *", "int"],
}


def _header_text():
    from dependence_free_rl_amd import _lib
    with open(_lib.HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for call in CALLS:
        assert call in _lib.header_symbols()
        assert (" T %s\n" % call) in out, "%s is not exported" % call


def test_binding_prototypes_are_the_headers():
    from dependence_free_rl_amd import _lib
    text = _header_text()
    ctype = {"int": C.c_int, "long": C.c_long, "xh_venv *": C.c_void_p,
             "const xh_venv *": C.c_void_p, "float *": C.c_void_p,
             "const float *": C.c_void_p, "const int32_t *": C.c_void_p,
             "const xh_item_set *": C.POINTER(_lib.ItemSet),
             "struct xh_venv_table_info *": C.POINTER(_lib.VenvTableInfo)}
    for call, want in CALLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % call, text)
        assert m, "%s is not declared in xylo_hip.h" % call
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).strip() for p in params]
        assert types == want, call
        fn = getattr(_lib.lib, call)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [ctype[p] for p in want], call


def test_struct_mirror_and_limit():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_venv_table_info") == \
        C.sizeof(_lib.VenvTableInfo) == 32
    text = _header_text()
    m = re.search(r"struct xh_venv_table_info \{(.*?)\};", text, flags=re.S)
    fields = re.findall(r"int (\w+)(?:\[(\d)\])?;", m.group(1))
    assert fields == [("entries", ""), ("states", ""), ("items", ""),
                      ("rows", ""), ("side", "4")]
    assert [f[0] for f in _lib.VenvTableInfo._fields_] == \
        [f[0] for f in fields]
    assert re.search(r"#define XH_VTAB_MAX_ENTRIES 16384\b", text)
    assert _lib.VTAB_MAX_ENTRIES == tr.MAX_ENTRIES == 16384
    with open(os.path.join(_lib.HERE, "csrc", "xh_venv_table.h")) as f:
        assert re.search(r"#define XH_VTAB_MAX_ENTRIES 16384\b", f.read())


@pytest.mark.parametrize("name", sorted(set(SETS) - {"over"}))
@pytest.mark.parametrize("bins", [8, 64, 128])
def test_table_info_is_the_references(name, bins):
    import dependence_free_rl_amd as pkg
    items, cap, D = SETS[name]
    m = tr.Domain(items, cap, D)
    got = pkg.item_set_table_info(items, capacity=cap, bins=bins)
    assert got["entries"] == m.E and got["states"] == m.S
    assert got["items"] == m.K and got["rows"] == m.rows(bins)
    assert np.array_equal(got["side"], m.side)


def test_the_limit_itself_is_a_table():
    import dependence_free_rl_amd as pkg
    # 16 items x 16 * 16 * 4 states = 16384 entries
    items = [(1, 1, 1 + k % 3) if k < 3 else (2 + k % 13, 1 + k // 13, 1)
             for k in range(16)]
    got = pkg.item_set_table_info(items, capacity=(15, 15, 3), bins=8)
    assert got["entries"] == 16384 and got["rows"] == 2048


def test_refusals_are_status_codes():
    import dependence_free_rl_amd as pkg
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    items, cap, D = SETS["over"]
    with pytest.raises(pkg.XhError, match=r"E = 16400 entries"):
        pkg.item_set_table_info(items, capacity=cap, bins=64)
    assert b"16384" in lib.xh_last_error()
    # an invalid set: an item above its dim's capacity; an all-zero item
    with pytest.raises(pkg.XhError, match="item 0 is 6 in dim 0"):
        pkg.item_set_table_info([(6, 1)], capacity=(5, 7))
    with pytest.raises(pkg.XhError, match="zero in every dim"):
        pkg.item_set_table_info([(0, 0)], capacity=(5, 7))
    with pytest.raises(pkg.XhError, match="bins 12"):
        pkg.item_set_table_info([(1, 1)], capacity=(5, 7), bins=12)
    ti = _lib.VenvTableInfo()
    s = _lib.ItemSet()
    lib.xh_item_set_default(C.byref(s), 2)
    assert lib.xh_item_set_table_info(C.byref(s), 2, 64, None) == \
        _lib.XH_ERR_INVALID
    assert lib.xh_item_set_table_info(None, 2, 64, C.byref(ti)) == \
        _lib.XH_ERR_INVALID
    assert lib.xh_item_set_table_info(C.byref(s), 2, 64, C.byref(ti)) == 0
    assert (ti.entries, ti.states, ti.items, ti.rows) == (162, 81, 2, 3)
    assert list(ti.side) == [9, 9, 1, 1]
    # null handles
    assert lib.xh_venv_table_info(None, C.byref(ti)) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_table_obs(None, None) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_act_table(None, None, 0, 0) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_table_gather(None, None, None, 0, 0, None) == \
        _lib.XH_ERR_INVALID
    assert lib.xh_venv_table_grad(None, None, 0, 0, None, None, 0) == \
        _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()


def test_python_signatures():
    import dependence_free_rl_amd as pkg
    sig = lambda f: inspect.signature(f).parameters  # noqa: E731
    assert list(sig(pkg.VecEnv.table_info)) == ["self"]
    p = sig(pkg.VecEnv.table_obs)
    assert list(p) == ["self", "out"] and p["out"].default is None
    p = sig(pkg.VecEnv.act_table)
    assert list(p) == ["self", "table", "mode", "write_obs", "fetch"]
    assert (p["mode"].default, p["write_obs"].default, p["fetch"].default) \
        == ("sample", False, False)
    p = sig(pkg.VecEnv.table_logits)
    assert list(p) == ["self", "table", "rows", "first", "count", "out"]
    p = sig(pkg.VecEnv.table_grad)
    assert list(p) == ["self", "dout", "rows", "first", "count", "accumulate",
                       "out"]
    assert p["accumulate"].default is False and p["first"].default == 0
    for name in ("item_set_table_info", "VenvTableInfo", "VTAB_MAX_ENTRIES"):
        assert name in pkg.__all__
