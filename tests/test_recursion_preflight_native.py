"""The native recursion preflight under AddressSanitizer and UBSan, as a stand-alone program:
tests/native/recursion_preflight_host.cpp is built with g++ -fsanitize=address,undefined against
risc0_amd/csrc/recursion_preflight.cpp (plain C++, no HIP) and fed the hand-encoded programs and
the failing programs of tests/recursion_input_programs.py, then programs of random rows, which
must be refused or run. Its report per program must be the library's: the same counts and the
same words (an FNV-1a hash over the C ABI's arrays), or the same message."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import recursion_input_programs as IP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "native", "recursion_preflight_host.cpp"),
       os.path.join(ROOT, "risc0_amd", "csrc", "recursion_preflight.cpp")]
INC = os.path.join(ROOT, "risc0_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _fnv(h, a):
    for b in np.ascontiguousarray(a, dtype="<u4").tobytes():
        h = ((h ^ b) * 0x100000001B3) & (2**64 - 1)
    return h


def _library_report(prog, inp, po2):
    import risc0_amd as r
    try:
        wom, cyc, iops, out = r.recursion_preflight(prog.encoded(), po2, inp)
    except r.R0HipError as e:
        return "err " + str(e)
    h = 0xCBF29CE484222325
    for a in (cyc, wom, iops, out):
        h = _fnv(h, a)
    return f"ok {wom.shape[0]} {iops.shape[0]} {out.size} {h}"


def test_stand_alone_preflight_under_asan_and_ubsan(tmp_path):
    exe, cases = tmp_path / "recursion_preflight_host", tmp_path / "cases.txt"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", INC, "-o", str(exe), *SRC], check=True)
    IP.write_cases(str(cases))
    out = subprocess.run([str(exe), str(cases), "1500"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = dict(ln.split(" ", 1) for ln in out.stdout.strip().split("\n"))
    want = {n: (*f(), 11) for n, f in IP.CASES.items()}
    want.update({"err_" + n: f()[:3] for n, f in IP.ERRORS.items()})
    assert set(want) | {"fuzz"} == set(lines)
    for name, (prog, inp, po2) in want.items():
        assert lines[name] == _library_report(prog, inp, po2), name
        assert lines[name].startswith("err " if name.startswith("err_") else "ok "), (name, lines[name])
    ran, refused = (int(x) for x in re.search(r"(\d+) ran, (\d+) refused", lines["fuzz"]).groups())
    assert ran + refused == 2 * 1500 and ran > 0 and refused > 0
