"""The Back-record ABI without a GPU: the ctypes mirrors and the Rust structs have the header's
layout (the probe of tests/test_abi_layout.py), the constants agree on every side, the new entry
points are declared, exported and bound, and the host check refuses bad records with no device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirrors():
    from risc0_amd import hal
    return {"r0hip_back": hal.Back, "r0hip_backs": hal.BacksStruct}


def test_ctypes_structs_match_the_c_header():
    mirrors = _mirrors()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', "int main(void) {"]
    for cname, py in mirrors.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                             src, "-o", exe], capture_output=True, text=True)
        if cc.returncode:
            pytest.fail("the header does not compile as C11 with these field names:\n" + cc.stderr)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {}
    for ln in out:
        if ln:
            cname, field, val = ln.split()
            got[(cname, field)] = int(val)
    for cname, py in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    assert C.sizeof(mirrors["r0hip_back"]) == 12


def test_constants_and_rust_structs_follow_the_header():
    from risc0_amd import hal
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    kinds = {"ECALL": (1, 3), "POSEIDON2": (2, 39), "SHA2": (3, 10), "BIGINT": (4, 22)}
    for name, (kind, words) in kinds.items():
        assert re.search(rf"#define R0HIP_BACK_{name}\s+{kind}\s+/\*\s*{words} words", hdr), name
        assert re.search(rf"pub const R0HIP_BACK_{name}: u32 = {kind};", rs), name
        assert getattr(hal, "BACK_" + name) == kind and hal.BACK_WORDS[kind] == words
    assert re.search(r"#define R0HIP_JOB_RV32IM_BACKS 2\b", hdr) and hal.JOB_RV32IM_BACKS == 2
    assert re.search(r"pub const R0HIP_JOB_RV32IM_BACKS: u32 = 2;", rs)
    for rname, py in (("R0HipBack", hal.Back), ("R0HipBacks", hal.BacksStruct)):
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct " + rname + r" \{(.*?)\n\}", rs, flags=re.S)
        assert m, rname
        assert re.findall(r"pub (\w+):", m.group(1)) == [f[0] for f in py._fields_], rname
    # the worker job's new field is its last: every earlier offset is unchanged
    assert hal.WorkerJobStruct._fields_[-1][0] == "backs" and hal.WorkerJobStruct._fields_[-2][0] == "ticket"


def test_entry_points_are_declared_exported_and_bound():
    import risc0_amd as r
    L = r.lib()
    for n in ("r0hip_rv32im_inject_backs", "r0hip_prove_segment_trace_backs"):
        assert n in r.exported_symbols(), n
        assert getattr(L, n).argtypes is not None, n


def test_host_check_names_the_record_without_a_device():
    """the record check runs before any device call: it answers here too, naming the record"""
    import risc0_amd as r
    recs = np.array([[0, 2, 0], [5, 2, 39], [5, 3, 78]], np.uint32)
    backs = r.Backs(recs, np.zeros(88, np.uint32), 8)
    cyc = np.zeros(8 * 9, np.uint32)
    pf = r.hal.RawPreflightTrace(cyc.ctypes.data, None, None, 0, 0, 8)
    glob = np.zeros(90, np.uint32)
    seal = np.zeros(4, np.uint32)
    n = C.c_size_t(0)
    u32p = C.POINTER(C.c_uint32)
    err = r.lib().r0hip_prove_segment_trace_backs(0, 3, 0, glob.ctypes.data_as(u32p), C.byref(pf), C.byref(backs.struct),
                                                  seal.ctypes.data_as(u32p), 4, C.byref(n), None)
    with pytest.raises(r.R0HipError, match=r"record 2 \(row 5\): rows must strictly increase"):
        r.check(err)
    err = r.lib().r0hip_rv32im_inject_backs(None, 8, cyc.ctypes.data, C.byref(backs.struct))
    with pytest.raises(r.R0HipError, match="d_data is NULL"):
        r.check(err)
