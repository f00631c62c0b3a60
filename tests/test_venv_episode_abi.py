"""CPU-side checks of the VecEnv's episode-statistics ABI (xh_venv_set_episode_
stats / xh_venv_episode_row / ...): the calls are declared, exported and
typed, the header's enums equal the Python mirror, NULL arguments give status
codes, the pinned sets are as they were, and the Python methods exist; no GPU
compute."""
import ctypes as C
import inspect
import os

from test_stats_abi import _header_enum

CALLS = ("xh_venv_set_episode_stats", "xh_venv_episode_row",
         "xh_venv_episode_count", "xh_venv_get_episode_rows",
         "xh_venv_episode_bytes", "xh_venv_episode_ptr",
         "xh_venv_episode_get", "xh_venv_episode_set")


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for name in CALLS:
        assert name in syms, name
        assert (" T %s\n" % name) in out, name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.xh_venv_episode_ptr.restype is C.c_void_p
    assert _lib.lib.xh_venv_episode_bytes.restype is C.c_size_t


def test_header_enums_equal_the_mirror():
    import dependence_free_rl_amd as pkg
    from dependence_free_rl_amd import _lib
    row = _header_enum("XH_VEP_")
    assert len(row) == 13                      # 12 entries + COUNT
    for name, value in row.items():
        assert getattr(_lib, name[3:]) == value, name
        assert getattr(pkg, name[3:]) == value, name
    assert list(row) == ["XH_VEP_ROW", "XH_VEP_CALLS", "XH_VEP_EPISODES",
                         "XH_VEP_LEN_SUM", "XH_VEP_LEN_SQSUM",
                         "XH_VEP_LEN_MIN", "XH_VEP_LEN_MAX",
                         "XH_VEP_ENVS_FINISHED", "XH_VEP_FIRST_LEN_SUM",
                         "XH_VEP_FIRST_LEN_SQSUM", "XH_VEP_RUNNING_SUM",
                         "XH_VEP_RUNNING_MAX", "XH_VEP_COUNT"]
    state = _header_enum("XH_VEPS_")
    assert state == {"XH_VEPS_RUNNING": 0, "XH_VEPS_FIRST": 1,
                     "XH_VEPS_COUNT": 2}
    for name, value in state.items():
        assert getattr(_lib, name[3:]) == value, name
    assert _lib.lib.xh_struct_size(b"xh_vep_row") == _lib.VEP_COUNT * 8 == 96


def test_the_restatement_uses_the_same_indices():
    import venv_episode_ref as er
    from dependence_free_rl_amd import _lib
    for name in ("ROW", "CALLS", "EPISODES", "LEN_SUM", "LEN_SQSUM", "LEN_MIN",
                 "LEN_MAX", "ENVS_FINISHED", "FIRST_LEN_SUM",
                 "FIRST_LEN_SQSUM", "RUNNING_SUM", "RUNNING_MAX", "COUNT"):
        assert getattr(er, name) == getattr(_lib, "VEP_" + name), name


def test_null_arguments_are_status_codes():
    from dependence_free_rl_amd import _lib
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    buf = C.create_string_buffer(96)
    n = C.c_long()
    for call in (lambda: lib.xh_venv_set_episode_stats(None, 8),
                 lambda: lib.xh_venv_set_episode_stats(None, 0),
                 lambda: lib.xh_venv_episode_row(None),
                 lambda: lib.xh_venv_episode_count(None, C.byref(n)),
                 lambda: lib.xh_venv_get_episode_rows(None, 0, 1, buf),
                 lambda: lib.xh_venv_episode_get(None, 0, buf, 96),
                 lambda: lib.xh_venv_episode_set(None, 0, buf, 96)):
        assert call() == INV
        assert b"null" in lib.xh_last_error()
    for which in (_lib.VEPS_RUNNING, _lib.VEPS_FIRST, -1, _lib.VEPS_COUNT):
        assert lib.xh_venv_episode_bytes(None, which) == 0
        assert lib.xh_venv_episode_ptr(None, which) is None


def test_the_pinned_sets_are_as_before():
    assert _header_enum("XH_VENV_BUF")["XH_VENV_BUF_COUNT"] == 10
    assert len(_header_enum("XH_VREC_")) == 7    # 6 arrays + COUNT
    assert len(_header_enum("XH_STAT_")) == 22   # the trainer's row


def test_python_methods():
    import dependence_free_rl_amd as pkg
    V = pkg.VecEnv
    for name in ("set_episode_stats", "episode_row", "episode_count",
                 "episode_stats", "episode_curve", "episode_state",
                 "set_episode_state", "first_episode_lengths"):
        assert callable(getattr(V, name)), name
    assert "rows" in inspect.signature(V.set_episode_stats).parameters
    stats = inspect.signature(V.episode_stats).parameters
    assert stats["first"].default is None and stats["count"].default is None
    assert list(inspect.signature(V.set_episode_state).parameters)[1:] == [
        "running", "first"]
