"""Host-side checks of the GPU worker and its keyed noise (no device needed): the ChaCha20 model
the GPU tests compare the kernel with reproduces RFC 8439's test vector and the element
definition of r0hip_fill_chacha20; the new ctypes mirrors and Rust structs have the header's
layout; the header is still C11; and without a device the worker's entry points return error
strings."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import chacha_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RFC_BLOCK = ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
             "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")
RFC_ELEMENTS = [728272357, 838115523, 261376304, 378995873]


def test_chacha20_model_reproduces_rfc_8439_2_3_2():
    """key bytes 00..1f, nonce words 0x09000000 0x4a000000 0, counter 1: the RFC's block, and its
    four field elements (128-bit little-endian integers of words 4j..4j+3, mod p)"""
    assert M.RFC_KEY.tobytes() == bytes(range(32))
    words = M.block(M.RFC_KEY, 1, M.RFC_NONCE)
    assert " ".join(f"{w:08x}" for w in words) == RFC_BLOCK
    assert M.block_elements(words) == RFC_ELEMENTS
    assert M.P == 2013265921
    # block b of the stream is elements 4b..4b+3: the vectorised model agrees with the plain one
    el = M.elements(M.RFC_KEY, M.RFC_NONCE, 4 * 70 + 1)
    assert [int(v) for v in el[4:8]] == RFC_ELEMENTS
    for b in (0, 2, 69):
        assert [int(v) for v in el[4 * b:4 * b + 4]] == M.block_elements(M.block(M.RFC_KEY, b, M.RFC_NONCE))
    assert int(el[280]) == M.block_elements(M.block(M.RFC_KEY, 70, M.RFC_NONCE))[0]
    assert el.dtype == np.uint32 and int(el.max()) < M.P


def _mirrors():
    from risc0_amd import hal
    return {"r0hip_recursion_input": hal.RecursionInput, "r0hip_worker_job": hal.WorkerJobStruct}


def test_worker_ctypes_structs_match_the_c_header():
    """sizeof and every offsetof of the two new mirrors, from a C program compiled with gcc
    against the header (the probe of tests/test_abi_layout.py); the header compiles as C11"""
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


def _c_fields(hdr, cname):
    m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S)
    assert m, cname
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_worker_structs_list_the_header_fields_in_order():
    """the ctypes mirrors and the #[repr(C)] structs of integration/rust/sys_hip.rs name the
    header's fields in the header's order"""
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    mirrors = _mirrors()
    for rname, cname in (("R0HipRecursionInput", "r0hip_recursion_input"), ("R0HipWorkerJob", "r0hip_worker_job")):
        cfields = _c_fields(hdr, cname)
        m = re.search(r"pub struct " + rname + r" \{(.*?)\n\}", rs, flags=re.S)
        assert m, rname
        assert re.search(r"#\[repr\(C\)\]\s*pub struct " + rname + r"\b", rs), rname
        assert re.findall(r"pub (\w+):", m.group(1)) == cfields, rname
        assert [f[0] for f in mirrors[cname]._fields_] == cfields, cname
    assert re.search(r"#define R0HIP_JOB_RV32IM_TRACE 0\b", hdr) and re.search(r"#define R0HIP_JOB_RECURSION 1\b", hdr)
    from risc0_amd import hal
    assert (hal.JOB_RV32IM_TRACE, hal.JOB_RECURSION) == (0, 1)


def test_new_entry_points_are_declared_exported_and_bound():
    import risc0_amd as r
    L = r.lib()
    names = ["r0hip_fill_chacha20", "r0hip_prove_recursion_keyed", "r0hip_worker_create", "r0hip_worker_submit",
             "r0hip_worker_wait", "r0hip_worker_destroy"]
    declared = r.exported_symbols()
    for n in names:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n


def _no_device():
    return not (os.environ.get("HIP_VISIBLE_DEVICES") is None and os.path.exists("/dev/kfd"))


def test_worker_entry_points_report_errors_without_a_device():
    """r0hip_worker_submit / _wait / _destroy on a NULL worker return error strings; without a
    visible device r0hip_worker_create returns one too (no abort) and leaves *out NULL"""
    import risc0_amd as r
    L = r.lib()
    job = r.WorkerJobStruct()
    for err in (L.r0hip_worker_submit(None, C.byref(job)), L.r0hip_worker_submit(None, None),
                L.r0hip_worker_wait(None, None, 0), L.r0hip_worker_destroy(None)):
        assert err
        assert b"null argument" in C.cast(err, C.c_char_p).value
        L.r0hip_free_error(err)
    h = C.c_void_p(1)
    err = L.r0hip_worker_create(C.byref(h), 25, 2, 1, None)  # refused before any device call
    assert err and b"max_po2" in C.cast(err, C.c_char_p).value and not h.value
    L.r0hip_free_error(err)
    if not _no_device():
        return  # a GPU may be present; create is covered by the gpu tests
    h = C.c_void_p(1)
    err = L.r0hip_worker_create(C.byref(h), 14, 2, 1, None)
    assert err and not h.value
    L.r0hip_free_error(err)
    with pytest.raises(r.R0HipError):
        r.Worker(None, 14)
