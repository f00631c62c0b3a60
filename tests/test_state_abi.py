"""CPU-side checks of the trainer-state ABI (xh_trainer_state_bytes /
save_state / load_state / state_digest, xh_state_describe, xh_digest_host and
the blob layout of include/xylo_hip.h); no GPU compute.  The digest is checked
against a numpy restatement of its formula; the blob reader against blobs built
here by hand from the documented layout."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from test_stats_abi import _header_enum

CALLS = ("xh_trainer_state_bytes", "xh_trainer_save_state",
         "xh_trainer_load_state", "xh_state_describe",
         "xh_trainer_state_digest", "xh_digest_host")
M64 = (1 << 64) - 1


def np_digest(data, first=0):
    """sum_i splitmix64(((first + i) << 32) | w_i) mod 2^64 over the 32-bit
    little-endian words of `data`, a byte tail zero-padded to a word."""
    b = bytes(data)
    b += b"\0" * (-len(b) % 4)
    w = np.frombuffer(b, "<u4").astype(np.uint64)
    i = np.arange(first, first + w.size, dtype=np.uint64)
    x = (i << np.uint64(32)) | w
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return int(x.sum(dtype=np.uint64)) if x.size else 0


def lib_digest(data):
    from dependence_free_rl_amd import _lib
    b = bytes(data)
    buf = (C.c_char * max(len(b), 1)).from_buffer_copy(b or b"\0")
    out = C.c_uint64(12345)
    assert _lib.lib.xh_digest_host(buf, len(b), C.byref(out)) == _lib.XH_OK
    return out.value


def make_blob(sections, magic=0x31534858, version=1):
    """A blob in the documented layout: header (144 bytes), table of
    {id, 0, offset, bytes, digest}, sections at multiples of 16."""
    from dependence_free_rl_amd import _lib
    cfg = _lib.Config()
    _lib.lib.xh_config_default(C.byref(cfg), _lib.XH_PPO, 8, 2, 16, 4)
    table_end = 144 + 32 * len(sections)
    body, rows, at = b"", [], table_end
    for sid, data in sections:
        pad = -at % 16
        body += b"\0" * pad + data
        at += pad
        rows.append(struct.pack("<IIQQQ", sid, 0, at, len(data), np_digest(data)))
        at += len(data)
    payload = b"".join(rows) + body
    head = struct.pack("<IIIIQQ", magic, version, 144, len(sections),
                       144 + len(payload), np_digest(payload))
    head += bytes(cfg) + struct.pack("<I", 0)
    assert len(head) == 144
    return head + payload


def describe(blob, cap=4096):
    from dependence_free_rl_amd import _lib
    buf = C.create_string_buffer(cap)
    src = (C.c_char * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    st = _lib.lib.xh_state_describe(src, len(blob), buf, cap)
    return st, buf.value.decode(), _lib.lib.xh_last_error().decode()


def test_header_declares_and_library_exports_the_calls():
    from dependence_free_rl_amd import _lib
    syms = _lib.header_symbols()
    out = os.popen("nm -D --defined-only %s" % _lib.LIB_PATH).read()
    for s in CALLS:
        assert s in syms, "%s is not declared in xylo_hip.h" % s
        assert (" T %s\n" % s) in out, "%s is not exported" % s
        assert getattr(_lib.lib, s).argtypes is not None, s


def test_null_handles_are_status_codes_and_outputs_untouched():
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    assert lib.xh_trainer_state_bytes(None) == 0
    buf = C.create_string_buffer(b"\x5a" * 64, 64)
    n = C.c_size_t(777)
    assert lib.xh_trainer_save_state(None, buf, 64, C.byref(n)) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert n.value == 777 and buf.raw == b"\x5a" * 64
    assert lib.xh_trainer_load_state(None, buf, 64, _lib.STATE_ALL) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    dig = (C.c_uint64 * _lib.DIG_COUNT)(*([9] * _lib.DIG_COUNT))
    assert lib.xh_trainer_state_digest(None, dig) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    assert list(dig) == [9] * _lib.DIG_COUNT
    assert lib.xh_digest_host(buf, 64, None) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()
    out = C.c_uint64(5)
    assert lib.xh_digest_host(None, 4, C.byref(out)) == _lib.XH_ERR_INVALID
    assert out.value == 5
    assert lib.xh_state_describe(buf, 64, None, 0) == _lib.XH_ERR_INVALID
    assert b"null" in lib.xh_last_error()


def test_header_size_is_the_documented_one():
    from dependence_free_rl_amd import _lib
    # 4 x uint32 + 2 x uint64 + xh_config + uint32
    assert _lib.lib.xh_struct_size(b"xh_state_header") == 144
    assert 16 + 16 + C.sizeof(_lib.Config) + 4 == 144
    assert _lib.lib.xh_struct_size(b"xh_state_section") == 32
    assert _lib.STATE_HEADER_BYTES == 144


def test_python_constants_mirror_the_header():
    from dependence_free_rl_amd import _lib
    import dependence_free_rl_amd as pkg
    enum = _header_enum("XH_DIG_")
    assert enum["XH_DIG_COUNT"] == len(enum) - 1 == 10
    mirror = {k: v for k, v in vars(_lib).items() if k.startswith("DIG_")}
    assert {"XH_" + k: v for k, v in mirror.items()} == enum
    states = _header_enum("XH_STATE_")
    assert states == {"XH_STATE_ALL": _lib.STATE_ALL, "XH_STATE_NETS": _lib.STATE_NETS}
    with open(_lib.HEADER) as f:
        assert "#define XH_STATE_VERSION %d\n" % _lib.STATE_VERSION in f.read()
    for k, v in list(mirror.items()) + [("STATE_ALL", 0), ("STATE_NETS", 1),
                                        ("STATE_VERSION", 1)]:
        assert getattr(pkg, k) == v, k
    from dependence_free_rl_amd.trainer import DIGEST_NAMES
    assert len(DIGEST_NAMES) == _lib.DIG_COUNT
    for k, name in enumerate(DIGEST_NAMES):
        assert mirror["DIG_" + name.upper()] == k


@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 5, 4099])
def test_digest_host_is_the_formula(nbytes):
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes, np.uint8).tobytes()
    assert lib_digest(data) == np_digest(data)
    if nbytes:
        from dependence_free_rl_amd import digest
        assert digest(data) == np_digest(data)
        assert digest(np.frombuffer(data, np.uint8)) == np_digest(data)


def test_digest_of_known_words():
    # one zero word: splitmix64(0) of the published generator's first output
    assert np_digest(b"\0\0\0\0") == 0xE220A8397B1DCDAF
    assert lib_digest(b"\0\0\0\0") == 0xE220A8397B1DCDAF


def test_digest_depends_on_word_positions():
    w = np.arange(1, 65, dtype="<u4")
    s = w.copy()
    s[[3, 40]] = s[[40, 3]]
    assert lib_digest(w.tobytes()) != lib_digest(s.tobytes())
    # ... while a plain sum of the words would not
    assert int(w.sum()) == int(s.sum())


def test_digest_is_a_sum_over_any_split():
    """The associativity the device reduction relies on: the digest of a
    buffer is the sum mod 2^64 of the digests of its parts, each part's words
    indexed from where it starts."""
    data = np.random.default_rng(7).integers(0, 256, 4096 + 3, np.uint8).tobytes()
    whole = lib_digest(data)
    for cut in (4, 2048, 4092):
        first = lib_digest(data[:cut])
        second = np_digest(data[cut:], first=cut // 4)
        assert (first + second) & M64 == whole, cut


def test_describe_reads_a_hand_built_blob():
    rng = struct.pack("<4I", 1, 2, 3, 4)
    blob = make_blob([(8, rng), (10, b"\x01" * 64)])
    st, js, err = describe(blob)
    assert st == 0, err
    d = json.loads(js)
    assert d["version"] == 1 and d["bytes"] == len(blob)
    assert d["config"]["bins"] == 8 and d["config"]["num_envs"] == 16
    assert [s["name"] for s in d["sections"]] == ["rng", "optimizers"]
    assert d["sections"][0]["bytes"] == 16
    assert int(d["sections"][0]["digest"], 16) == np_digest(rng)
    from dependence_free_rl_amd import describe_state
    assert describe_state(blob) == d


def test_describe_refuses_malformed_blobs():
    from dependence_free_rl_amd import _lib, describe_state
    good = make_blob([(8, struct.pack("<4I", 1, 2, 3, 4))])
    assert describe(good)[0] == 0
    cases = {
        "empty": b"",
        "short": good[:100],
        "magic": make_blob([(8, b"\1\0\0\0")], magic=0x12345678),
        "version": make_blob([(8, b"\1\0\0\0")], version=2),
        "truncated": good[:-4],
        "flipped": good[:-1] + bytes([good[-1] ^ 1]),
    }
    # a section table that points past the end, with a consistent payload
    # digest: the bounds check has to catch it, not the digest
    row = struct.pack("<IIQQQ", 8, 0, 176, 1 << 40, 0)
    head = struct.pack("<IIIIQQ", 0x31534858, 1, 144, 1, 176, np_digest(row))
    cases["past_end"] = head + good[32:144] + row
    # offset + bytes overflowing 64 bits
    row = struct.pack("<IIQQQ", 8, 0, 176, M64 - 8, 0)
    head = struct.pack("<IIIIQQ", 0x31534858, 1, 144, 1, 176, np_digest(row))
    cases["wraps"] = head + good[32:144] + row
    # more sections announced than the blob has room for
    head = struct.pack("<IIIIQQ", 0x31534858, 1, 144, 12, 144, 0)
    cases["table_past_end"] = head + good[32:144]
    for name, blob in cases.items():
        st, js, err = describe(blob)
        assert st == _lib.XH_ERR_INVALID, name
        assert err, name
        with pytest.raises(_lib.XhError, match="status 1"):
            describe_state(blob)
    assert "section" in describe(cases["past_end"])[2]
    assert "magic" in describe(cases["magic"])[2]
    assert "version" in describe(cases["version"])[2]
