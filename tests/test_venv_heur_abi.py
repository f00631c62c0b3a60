"""CPU-side checks of the xh_venv_act_heuristic ABI: the symbol is declared
and exported, the Python binding's prototype is the header's, the heuristic
enumerators are the evaluator's, the argument check that needs no device
returns its code, and the Python signatures are as documented; no GPU
compute."""
import ctypes as C
import inspect
import os
import re

from test_stats_abi import _header_enum

CALL = "xh_venv_act_heuristic"


def _header_prototype(name):
    """(return type, [parameter types]) of `name` in include/xylo_hip.h."""
    from dependence_free_rl_amd import _lib
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in xylo_hip.h" % name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    # drop the parameter names
    types = [re.sub(r"\s*\w+$", "", p).strip() for p in params]
    return m.group(1).strip(), types


def test_header_declares_and_library_exports_the_call():
    from dependence_free_rl_amd import _lib
    assert CALL in _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    assert (" T %s\n" % CALL) in out, "%s is not exported" % CALL


def test_binding_prototype_is_the_headers():
    from dependence_free_rl_amd import _lib
    ret, params = _header_prototype(CALL)
    assert ret == "int"
    assert params == ["xh_venv *", "int", "int"]
    ctype = {"int": C.c_int, "xh_venv *": C.c_void_p}
    fn = getattr(_lib.lib, CALL)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [ctype[p] for p in params]
    # next to xh_venv_act, and documented there
    with open(_lib.HEADER) as f:
        text = f.read()
    assert text.index("int xh_venv_act(") < text.index("int " + CALL + "(") \
        < text.index("int xh_venv_set_record(")
    assert "the venv's own heuristics (xh_venv_act_heuristic)" in \
        " ".join(text.split()).replace("* ", "")


def test_heuristic_enumerators_are_the_evaluators():
    from dependence_free_rl_amd import _lib
    enum = _header_enum("XH_HEUR_")
    assert enum == {"XH_HEUR_RANDOM": 0, "XH_HEUR_FIRSTFIT": 1,
                    "XH_HEUR_BESTFIT": 2, "XH_HEUR_MINWASTE": 3}
    assert _lib.HEURISTICS == {k[len("XH_HEUR_"):].lower(): v
                               for k, v in enum.items()}


def test_null_handle_is_a_status_code():
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    for heur in (-1, 0, 1, 2, 3, 4):
        for obs in (0, 1):
            assert lib.xh_venv_act_heuristic(None, heur, obs) == \
                _lib.XH_ERR_INVALID
            assert b"null" in lib.xh_last_error()


def test_python_signatures():
    import dependence_free_rl_amd as pkg
    p = inspect.signature(pkg.VecEnv.act_heuristic).parameters
    assert list(p) == ["self", "kind", "write_obs", "fetch"]
    assert (p["write_obs"].default, p["fetch"].default) == (False, False)
    q = inspect.signature(pkg.heuristic_baseline).parameters
    assert list(q) == ["ctx", "kind", "bins", "dims", "num_envs", "items",
                       "weights", "capacity", "rng_state", "max_steps",
                       "row_every"]
    assert q["row_every"].default == 64
    assert all(q[n].default is None for n in ("items", "weights", "capacity"))
    assert "heuristic_baseline" in pkg.__all__


def test_unknown_kind_is_refused_before_the_library_is_called():
    import pytest

    import dependence_free_rl_amd as pkg
    env = pkg.VecEnv.__new__(pkg.VecEnv)  # no device: the check comes first
    env.h = None
    with pytest.raises(ValueError, match="kind"):
        env.act_heuristic("worstfit")
