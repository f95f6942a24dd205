"""Host-side check of the NTT's range-typed field helpers and of the butterfly network of one
register group (risc0_amd/csrc/ntt_bfly.h, the code ntt.hip's stage_group runs): every helper
against 128-bit reference arithmetic with its documented output range asserted, the network
word for word against the same network in canonical fp_add / fp_sub / fp_mul for NST 1..3,
forward and inverse, with and without the skipped first-stage twiddles, with the header's own
range assertions compiled in. Builds tests/native/ntt_bfly_equiv.cpp with g++, once plain and
once as a stand-alone program under the undefined-behaviour sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntt_bfly_equiv.cpp")
INC = os.path.join(ROOT, "risc0_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, *flags):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-I", INC, "-o", str(exe), SRC],
                   check=True)


def test_helpers_and_group_network(tmp_path):
    exe = tmp_path / "ntt_bfly_equiv"
    _build(exe)
    out = subprocess.run([str(exe), "1000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK")


def test_helpers_and_group_network_ubsan(tmp_path):
    exe = tmp_path / "ntt_bfly_equiv_ubsan"
    _build(exe, "-fsanitize=undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([str(exe), "1000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK") and "runtime error" not in out.stderr
