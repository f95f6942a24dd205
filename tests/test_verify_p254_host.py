"""Poseidon254 openings of the device receipt check, the part that needs no GPU
(include/r0hip.h: r0hip_set_verify_device_poseidon254): the setter and where it is declared, the
op's refusals for suite 2 with the switch off (today's suite error) and on (the Poseidon2 checks
with the same field names, all on the host before any device call), and tests/native/
p254_open_host.cpp: hash_tops against the serial top-layer loop, plain and under
AddressSanitizer + UBSan as a stand-alone host program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_verify_device_host import _msg, _open

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "r0hip_set_verify_device_poseidon254"
P = 15 * 2**27 + 1


@pytest.fixture(scope="module")
def r():
    import risc0_amd as r
    return r


@pytest.fixture
def switch_on(r):
    """the switch is process-wide and every other test relies on its default"""
    r.set_verify_device_poseidon254(1)
    try:
        yield
    finally:
        r.set_verify_device_poseidon254(0)


def test_setter_is_declared_everywhere(r):
    assert NAME in r.exported_symbols() and hasattr(r.lib(), NAME)
    py = open(os.path.join(ROOT, "risc0_amd", "hal.py")).read()
    assert f'"{NAME}"' in py and "def set_verify_device_poseidon254(on)" in py
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    assert re.search(r"pub fn " + NAME + r"\(on: c_int\) -> \*const c_char;", rs)
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    assert re.search(r"/\* \[host-only\] \*/\nconst char\* " + NAME + r"\(int on\);", hdr)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_setter_takes_0_and_1_only_and_needs_no_device(r):
    L = r.lib()
    try:
        for on in (1, 0, 1, 1, 0):
            assert _msg(r, getattr(L, NAME)(on)) is None
        for on in (-1, 2):
            m = _msg(r, getattr(L, NAME)(on))
            assert m and "on" in m.split() and str(on) in m, m
            with pytest.raises(r.R0HipError):
                r.set_verify_device_poseidon254(on)
        # a refused value leaves the switch as it was (off): suite 2 is still today's error
        m = _open(r, 2, np.zeros(300, np.uint32), [(0, 16, 5, 16, 2)])
        assert m and "suite" in m and "2" in m and "no device form" in m, m
    finally:
        r.set_verify_device_poseidon254(0)


def test_switch_off_suite_2_is_todays_error(r):
    words = np.zeros(300, np.uint32)
    good = (0, 16, 5, 16, 2)
    m = _open(r, 2, words, [good])
    assert m and "suite" in m and "2" in m and "no device form" in m, m
    # and it is the suite that is refused, before anything else is looked at
    assert _open(r, 2, words, [good], words_null=True) == m
    assert _open(r, 2, words, [(0, 16, 5, 257, 2)]) == m


def test_switch_on_refuses_malformed_tables_without_a_device(r, switch_on):
    """test_merkle_open_digests_refuses_malformed_tables_without_a_device's tables at suite 2: the
    same field names as Poseidon2 gets (and the same messages, compared with suite 0's)"""
    words = np.zeros(300, np.uint32)
    good = (0, 16, 5, 16, 2)  # row [0, 16), path [16, 32)
    for suite in (3, -1):
        m = _open(r, suite, words, [good])
        assert m and "suite" in m and str(suite) in m, m
    cases = []
    m = _open(r, 2, words, [good], words_null=True)
    assert m and "h_words is NULL" in m, m
    m = _open(r, 2, words, [good], table_null=True)
    assert m and "h_open is NULL" in m, m
    m = _open(r, 2, words, [good], digests=False)
    assert m and "h_digests is NULL" in m, m
    m = _open(r, 2, words, [good], status=False)
    assert m and "h_status is NULL" in m, m
    for cols in (0, 257):
        table = [good, (0, 16, 5, cols, 2)]
        m = _open(r, 2, words, table)
        assert m and "h_open[1].cols" in m and str(cols) in m, m
        cases.append((table, m))
    table = [good, good, (0, 16, 5, 16, 41)]
    m = _open(r, 2, words, table)
    assert m and "h_open[2].levels" in m and "41" in m, m
    cases.append((table, m))
    # a row, then a path, that ends one word past n_words
    table = [(300 - 16 + 1, 0, 5, 16, 2)]
    m = _open(r, 2, words, table)
    assert m and "h_open[0].row_off" in m and "n_words" in m, m
    cases.append((table, m))
    table = [good, (0, 300 - 16 + 1, 5, 16, 2)]
    m = _open(r, 2, words, table)
    assert m and "h_open[1].path_off" in m and "n_words" in m, m
    cases.append((table, m))
    # offsets that would wrap a 64-bit sum
    table = [(2**64 - 8, 0, 5, 16, 0)]
    m = _open(r, 2, words, table)
    assert m and "h_open[0].row_off" in m, m
    cases.append((table, m))
    table = [(0, 2**64 - 8, 5, 16, 2)]
    m = _open(r, 2, words, table)
    assert m and "h_open[0].path_off" in m, m
    cases.append((table, m))
    for table, m in cases:
        assert _open(r, 0, words, table) == m, table
    # rows are field elements: p254_pack8's column bound assumes values below 2^31
    bad = words.copy()
    bad[7] = P
    m = _open(r, 2, bad, [good])
    assert m and "h_words[7]" in m and "canonical" in m, m
    assert _open(r, 0, bad, [good]) == m


def test_switch_is_read_at_each_call(r):
    words, good = np.zeros(300, np.uint32), (0, 16, 5, 257, 2)
    try:
        assert "suite" in _open(r, 2, words, [good])
        r.set_verify_device_poseidon254(True)
        assert "h_open[0].cols" in _open(r, 2, words, [good])
        r.set_verify_device_poseidon254(False)
        assert "suite" in _open(r, 2, words, [good])
    finally:
        r.set_verify_device_poseidon254(0)


# ---- tests/native/p254_open_host.cpp ------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "native", "p254_open_host.cpp")
INC = os.path.join(ROOT, "risc0_amd", "csrc")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build_and_run(exe, *flags):
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", *flags, "-I", INC, "-o", str(exe), SRC], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@needs_gxx
def test_hash_tops_equals_the_serial_loop(tmp_path):
    out = _build_and_run(tmp_path / "p254_open_host")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK")


@needs_gxx
def test_hash_tops_under_asan_and_ubsan(tmp_path):
    """a plain host binary with its own main: no sanitizer goes near code loaded into Python"""
    out = _build_and_run(tmp_path / "p254_open_host_san", "-g", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK") and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
