"""CPU-side checks of the VecEnv's item-set ABI (xh_item_set, xh_item_set_
default / _thresholds, xh_venv_create_ex, xh_venv_set_item_set / _get_item_set):
the calls are declared, exported and typed, the struct's size equals the
ctypes mirror, the default set is make_env's, the thresholds are the
restatement's doubles, every invalid set is XH_ERR_INVALID, the pinned sets are
as they were and the Python signatures are as documented; no GPU compute."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_stats_abi import _header_enum
from venv_items_ref import DEFAULT_ITEMS, DEFAULT_WEIGHTS, thresholds

CALLS = ("xh_item_set_default", "xh_item_set_thresholds", "xh_venv_create_ex",
         "xh_venv_set_item_set", "xh_venv_get_item_set")

ITEMS5 = [(3, 1), (2, 2), (1, 4), (5, 7), (1, 1)]
WEIGHTS5 = [2.0, 0.0, 1.0, 0.5, 3.25]


def _set(items, weights, capacity, dims):
    from dependence_free_rl_amd.venv import _item_set
    return _item_set(items, weights, capacity, dims)


def _thresholds(s, dims):
    from dependence_free_rl_amd import _lib
    out = (C.c_double * 16)(*([-1.0] * 16))
    st = _lib.lib.xh_item_set_thresholds(C.byref(s), dims, out)
    return st, np.array(out[:], np.float64)


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.xh_item_set_default.restype is None
    assert len(_lib.lib.xh_venv_create_ex.argtypes) == 10
    assert _header_enum("XH_ITEMS_")["XH_ITEMS_MAX"] == _lib.ITEMS_MAX == 16


def test_struct_size_equals_the_mirror():
    from dependence_free_rl_amd import _lib
    assert _lib.lib.xh_struct_size(b"xh_item_set") == C.sizeof(_lib.ItemSet)
    assert C.sizeof(_lib.ItemSet) == 4 + 16 + 16 * 16 + 4 + 16 * 8  # 4: padding
    assert [n for n, _ in _lib.ItemSet._fields_] == [
        "num_items", "capacity", "item", "weight"]


@pytest.mark.parametrize("dims", [1, 2, 3])
def test_default_set_is_make_envs(dims):
    from dependence_free_rl_amd import _lib
    s = _lib.ItemSet()
    C.memset(C.byref(s), 0xFF, C.sizeof(s))
    _lib.lib.xh_item_set_default(C.byref(s), dims)
    assert s.num_items == 2
    assert list(s.capacity) == [8] * dims + [0] * (4 - dims)
    for k in range(2):
        assert list(s.item[k]) == list(DEFAULT_ITEMS[dims][k]) + [0] * (4 - dims)
    assert list(s.weight) == DEFAULT_WEIGHTS + [0.0] * 14
    assert all(list(s.item[k]) == [0] * 4 for k in range(2, 16))
    st, c = _thresholds(s, dims)
    assert st == _lib.XH_OK and c[:2].tolist() == [0.4, 1.0]


def test_thresholds_equal_the_restatement_bit_for_bit():
    import dependence_free_rl_amd as pkg
    from dependence_free_rl_amd import _lib
    g = np.random.default_rng(5)
    items16 = [(1 + k % 5, 1 + k % 7) for k in range(16)]
    w16 = g.random(16) * 3.0 + 0.01
    w16[[2, 15]] = 0.0  # a zero weight inside and one at the end
    for items, weights, cap in ((DEFAULT_ITEMS[2], DEFAULT_WEIGHTS, 8),
                                (ITEMS5, WEIGHTS5, (5, 7)),
                                (items16, w16, (5, 7))):
        K = len(items)
        st, c = _thresholds(_set(items, weights, cap, 2), 2)
        want = thresholds(weights)
        assert st == _lib.XH_OK
        assert c[:K].tobytes() == want.tobytes()
        assert (c[K:] == -1.0).all()  # K doubles are written
        got = pkg.item_set_thresholds(items, weights, cap)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
        assert want[-1] == 1.0
    assert thresholds(w16)[14] == 1.0  # nothing left for the trailing zero
    assert pkg.item_set_thresholds([4, 1], [0.4, 0.6]).tolist() == [0.4, 1.0]


def _invalid_sets():
    ok = dict(items=ITEMS5, weights=WEIGHTS5, capacity=(5, 7))

    def make(edit):
        s = _set(ok["items"], ok["weights"], ok["capacity"], 2)
        edit(s)
        return s

    def field(name, *idx_value):
        *idx, value = idx_value

        def edit(s):
            a = getattr(s, name)
            for i in idx[:-1]:
                a = a[i]
            a[idx[-1]] = value
        return edit

    def k_items(k):
        def edit(s):
            s.num_items = k
        return edit
    return {
        "K = 0": make(k_items(0)), "K = 17": make(k_items(17)),
        "K = -1": make(k_items(-1)),
        "capacity 0": make(field("capacity", 0, 0)),
        "capacity 65": make(field("capacity", 1, 65)),
        "capacity -3": make(field("capacity", 1, -3)),
        "item above its capacity": make(field("item", 2, 0, 6)),
        "item below zero": make(field("item", 0, 1, -1)),
        "all-zero item": make(lambda s: (field("item", 4, 0, 0)(s),
                                         field("item", 4, 1, 0)(s))),
        "negative weight": make(field("weight", 0, -0.5)),
        "NaN weight": make(field("weight", 3, float("nan"))),
        "infinite weight": make(field("weight", 3, float("inf"))),
        "zero sum": make(lambda s: [field("weight", k, 0.0)(s)
                                    for k in range(5)]),
    }


def test_every_invalid_set_is_refused():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    st, _ = _thresholds(_set(ITEMS5, WEIGHTS5, (5, 7), 2), 2)
    assert st == _lib.XH_OK
    for name, s in _invalid_sets().items():
        st, c = _thresholds(s, 2)
        assert st == INV, name
        assert b"item set" in lib.xh_last_error(), name
        assert (c == -1.0).all(), name  # nothing written
    # entries past D and past K are ignored
    s = _set(ITEMS5, WEIGHTS5, (5, 7), 2)
    s.capacity[2], s.item[0][3], s.item[7][0], s.weight[9] = -1, 99, 99, -1.0
    assert _thresholds(s, 2)[0] == _lib.XH_OK
    for dims in (0, 4):
        assert _thresholds(s, dims)[0] == INV


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    s = _set(ITEMS5, WEIGHTS5, (5, 7), 2)
    out = (C.c_double * 16)()
    h = C.c_void_p()
    lib.xh_item_set_default(None, 2)  # returns
    for call in (lambda: lib.xh_item_set_thresholds(None, 2, out),
                 lambda: lib.xh_item_set_thresholds(C.byref(s), 2, None),
                 lambda: lib.xh_venv_create_ex(None, 4, 8, 2, 1, 0, 4, 2,
                                               C.byref(s), C.byref(h)),
                 lambda: lib.xh_venv_create_ex(None, 4, 8, 2, 1, 0, 4, 2, None,
                                               C.byref(h)),
                 lambda: lib.xh_venv_set_item_set(None, C.byref(s)),
                 lambda: lib.xh_venv_get_item_set(None, C.byref(s))):
        assert call() == INV
        assert b"null" in lib.xh_last_error()
    assert h.value is None


def test_the_pinned_sets_are_as_before():
    assert _header_enum("XH_VENV_BUF")["XH_VENV_BUF_COUNT"] == 10
    assert len(_header_enum("XH_VREC_")) == 7    # 6 arrays + COUNT


def test_python_signatures():
    import dependence_free_rl_amd as pkg
    V = pkg.VecEnv
    p = inspect.signature(V.__init__).parameters
    assert list(p)[-3:] == ["items", "weights", "capacity"]
    for name in ("items", "weights", "capacity"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert p[name].default is None
    assert list(p)[:9] == ["self", "ctx", "num_envs", "bins", "dims",
                           "rng_state", "env_offset", "num_envs_global",
                           "policy_draws"]
    q = inspect.signature(V.set_item_set).parameters
    assert list(q) == ["self", "items", "weights"]
    assert q["weights"].default is None
    assert list(inspect.signature(V.item_set).parameters) == ["self"]
    r = inspect.signature(pkg.item_set_thresholds).parameters
    assert list(r) == ["items", "weights", "capacity"]
    assert "item_set_thresholds" in pkg.__all__
