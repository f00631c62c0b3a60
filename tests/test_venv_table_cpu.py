"""CPU check of the logit table's domain and quantiser as the kernels compile
them (dependence_free_rl_amd/csrc/xh_venv_table.h): tests/venv_table_check.cc
built with the host compiler prints the index, its inverse and the
fixed-point sum for the cases below, and every number is compared with
tests/venv_table_ref.py's numpy value."""
import os
import subprocess

import numpy as np
import pytest

import venv_table_ref as tr
from test_venv_table_ref import SETS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vtab") / "venv_table_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "venv_table_check.cc"),
                    "-o", path], check=True)
    return path


def _run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.split("\n")
    assert lines[-2] == "venv table check: done"
    return lines[:-2]


def _set_text(m):
    return " ".join(str(int(x)) for x in list(m.cap) + list(m.shapes.reshape(-1)))


@pytest.mark.parametrize("name", sorted(SETS))
def test_index_and_inverse(exe, name):
    items, cap, D = SETS[name]
    m = tr.Domain(items, cap, D)
    B = 64
    lines = _run(exe, "I %d %d %d %s\n" % (D, m.K, B, _set_text(m)))
    assert lines[0] == "dom %d %d %d" % (m.E, m.S, m.rows(B))
    assert len(lines) == 1 + m.E
    got = np.array([[int(x) for x in ln.split()] for ln in lines[1:]])
    assert np.array_equal(got[:, 0], np.arange(m.E))
    for e in range(m.E):
        k, b = m.decode(e)
        assert got[e, 1] == k and np.array_equal(got[e, 2:2 + D], b), e
        assert got[e, 2 + D] == m.entry(b, m.shapes[k]), e
    if name != "duplicate":  # a bijection onto [0, E)
        assert np.array_equal(got[:, 2 + D], np.arange(m.E))


def test_outside_the_domain(exe):
    m = tr.Domain(*SETS["cap57"])
    cases = [((3, 1), (5, 7)), ((1, 4), (0, 0)), ((2, 2), (3, 4)),
             ((3, 1), (-1, 0)), ((3, 1), (0, -1)), ((3, 1), (6, 0)),
             ((3, 1), (0, 8)), ((4, 2), (1, 1)), ((0, 0), (1, 1)),
             ((3, 1), (-128, 127))]
    text = "".join("X 2 %d %s %d %d %d %d\n" % ((m.K, _set_text(m)) + it + b)
                   for it, b in cases)
    lines = _run(exe, text)
    want = [int(m.entry(np.array(b), it)) for it, b in cases]
    assert [int(ln.split()[1]) for ln in lines] == want
    assert want[:3] == [47, 96, 48 + 28] and set(want[3:]) == {-1}


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _quant_case(exe, values, n=None):
    v = np.asarray(values, np.float32)
    n = v.size if n is None else n
    lines = _run(exe, "Q %d %d %s\n" % (n, v.size, " ".join(
        "%08x" % b for b in _bits(v))))
    m = np.abs(v).max()
    assert lines[0] == "max %08x" % _bits(m)
    if m == 0 or not np.isfinite(m):
        assert len(lines) == 1
        return None
    s = tr.quant_shift(n, float(m))
    assert lines[1] == "shift %d" % s
    q = tr.quantise(v, s)
    assert [int(ln.split()[1]) for ln in lines[2:2 + v.size]] == q.tolist()
    total = int(q.sum(dtype=np.int64))
    assert lines[2 + v.size] == "sum %d" % total
    G = tr.dequantise(np.int64(total), s)
    assert lines[3 + v.size] == "G %08x" % _bits(G)
    return s, total, G


def test_quantiser(exe):
    tiny = np.float32(2.0 ** -149)
    # n = 1
    s, total, G = _quant_case(exe, [0.3])
    assert s == 62 - 0 - (-1) and G == np.float32(0.3)
    # denormal and signed-zero addends
    s, total, G = _quant_case(exe, [tiny, -0.0, 0.0, 3 * tiny, -tiny])
    assert G == np.float32(3 * tiny) and s == 62 - 3 - (-147)
    _quant_case(exe, [1.0, tiny, -0.0, -tiny, 0.0])
    # n a power of two, and one past it
    rng = np.random.default_rng(3)
    for n in (4, 5, 1024, 1025):
        v = (rng.standard_normal(n) *
             np.ldexp(1.0, rng.integers(-20, 21, n))).astype(np.float32)
        s, _, _ = _quant_case(exe, v)
        assert s == 62 - tr.quant_log2(n) - tr.quant_exponent(
            float(np.abs(v).max()))
    assert tr.quant_log2(1024) == 10 and tr.quant_log2(1025) == 11
    # the addend count may exceed the addends shown (the other entries')
    _quant_case(exe, [0.5, -0.25, 1.5], n=1000)
    # an entry whose sum exceeds 2^53: the int64 -> double rounding counts
    s, total, G = _quant_case(exe, [1.0, 1.0, 2.0 ** -58, 0.99999994])
    assert s == 59 and abs(total) > 2 ** 53
    assert float(total) != total  # not representable: the conversion rounds
    # the largest finite magnitudes stay inside the int64
    big = np.float32(3.4028235e38)
    s, total, G = _quant_case(exe, [big, -big, big, big / -2])
    assert s == 62 - 2 - 128 and abs(total) < 2 ** 62
    assert G == big / np.float32(2)
    # all zero, and a NaN / an infinity: no shift is formed
    assert _quant_case(exe, [0.0, -0.0]) is None
    assert _quant_case(exe, [1.0, np.nan]) is None
    assert _quant_case(exe, [np.inf, 1.0]) is None
