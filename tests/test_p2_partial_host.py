"""Host-side check of Poseidon2's block-linear partial rounds (p2_partial_rounds in
risc0_amd/csrc/poseidon2.h) against 21 rounds of p2_sbox / p2_m_int, on inputs at the edges
of its documented range. Builds tests/native/p2_partial_equiv.cpp with g++, once plain and once
as a stand-alone program under the undefined-behaviour sanitizer, where any 64-bit accumulator
overflow on the host path traps."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "p2_partial_equiv.cpp")
INC = os.path.join(ROOT, "risc0_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, *flags):
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, "-I", INC, "-o", str(exe), SRC], check=True)


def test_partial_rounds_equivalence(tmp_path):
    exe = tmp_path / "p2_partial_equiv"
    _build(exe)
    out = subprocess.run([str(exe), "4000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK")


def test_partial_rounds_no_signed_overflow(tmp_path):
    exe = tmp_path / "p2_partial_equiv_ubsan"
    _build(exe, "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([str(exe), "1000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK") and "runtime error" not in out.stderr
