"""The opt-in device receipt check, the part that needs no GPU (include/r0hip.h:
r0hip_verify_seal_on, r0hip_testing_verify_seal_structure_on, r0hip_merkle_open_digests):
where = HOST is r0hip_verify_seal in verdict and message, every malformed argument is refused on
the host before a device is touched, and struct r0hip_opening has one layout in the header, the
ctypes mirror and the Rust binding."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = 0, 1
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def r():
    import risc0_amd as r
    return r


def _msg(r, err):
    """the C ABI's verdict as Python data: None (accepted) or the message, freed"""
    if not err:
        return None
    msg = C.cast(err, C.c_char_p).value.decode()
    r.lib().r0hip_free_error(err)
    return msg


def _p(a):
    return a.ctypes.data_as(u32p)


def _verify(r, circuit, suite, seal):
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    po2, root = C.c_uint32(0), np.zeros(8, np.uint32)
    m = _msg(r, r.lib().r0hip_verify_seal(circuit.encode(), suite, _p(seal), seal.size, None, 0, _p(root),
                                          C.byref(po2)))
    return m, po2.value, root.tobytes()


def _verify_on(r, where, circuit, suite, seal):
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    po2, root = C.c_uint32(0), np.zeros(8, np.uint32)
    m = _msg(r, r.lib().r0hip_verify_seal_on(where, circuit.encode(), suite, _p(seal), seal.size, None, 0, _p(root),
                                             C.byref(po2)))
    return m, po2.value, root.tobytes()


def _structure(r, circuit, suite, seal):
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    po2 = C.c_uint32(0)
    m = _msg(r, r.lib().r0hip_testing_verify_seal_structure(circuit.encode(), suite, _p(seal), seal.size,
                                                            C.byref(po2)))
    return m, po2.value


def _structure_on(r, where, circuit, suite, seal):
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    po2 = C.c_uint32(0)
    m = _msg(r, r.lib().r0hip_testing_verify_seal_structure_on(where, circuit.encode(), suite, _p(seal), seal.size,
                                                               C.byref(po2)))
    return m, po2.value


def zero_witness_seal(oracle, suite, po2):
    """test_verifier.py's accepted seal: the all-zero recursion witness satisfies the constraints"""
    d = oracle.load_circuit_json("recursion")
    n, gs = 1 << po2, d["group_sizes"]
    code, data, accum = (np.zeros(gs[g] * n, np.uint32) for g in (1, 2, 0))
    glob = oracle.rand_elems(np.random.default_rng(5), d["output_size"])
    seal, _mix, _ = oracle.prove_segment("recursion", suite, po2, code, data, accum, glob, version=None)
    return seal


@pytest.mark.parametrize("suite", [0, 1, 2])
def test_host_leg_is_verify_seal_on_the_accepted_seal(r, oracle, suite):
    seal = zero_witness_seal(oracle, suite, 8)
    want = _verify(r, "recursion", suite, seal)
    assert want[0] is None and want[1] == 8
    assert _verify_on(r, HOST, "recursion", suite, seal) == want
    assert _structure_on(r, HOST, "recursion", suite, seal) == _structure(r, "recursion", suite, seal) == (None, 8)
    # and on tampered copies: the same verdict and message from both. (A flipped header global is
    # accepted by both: the constraints hold for any globals, and every row of this witness being
    # equal, every query index opens the same leaf.)
    rng = np.random.default_rng(31 + suite)
    for where in [1, 9, seal.size // 4, seal.size // 2, seal.size - 3] + list(rng.integers(0, seal.size, 6)):
        bad = seal.copy()
        bad[where] ^= np.uint32(1 << int(rng.integers(0, 31)))
        want = _verify(r, "recursion", suite, bad)
        assert where < seal.size // 4 or want[0] is not None
        assert _verify_on(r, HOST, "recursion", suite, bad) == want


def test_host_leg_is_verify_seal_on_garbage(r, oracle):
    """the corpus of test_native_verifier_rejects_garbage: empty, random words, a tampered po2, cuts"""
    rng = np.random.default_rng(99)
    corpus = []
    for circuit in ("rv32im", "recursion"):
        for s in (0, 1, 2):
            for n in (0, 1, 5, 64, 4096):
                junk = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
                if circuit == "rv32im" and n:
                    junk[0] = 2
                corpus.append((circuit, s, junk))
    d = oracle.load_circuit_json("recursion")
    n, gs = 1 << 8, d["group_sizes"]
    code, data, accum = (oracle.rand_elems(rng, gs[g] * n) for g in (1, 2, 0))
    seal, _mix, _ = oracle.prove_segment("recursion", 0, 8, code, data, accum, oracle.rand_elems(rng, d["output_size"]))
    for po2 in (0, 1, 9, 25, 2**31):
        bad = seal.copy()
        bad[d["output_size"]] = po2
        corpus.append(("recursion", 0, bad))
    for cut in rng.integers(1, seal.size, 20):
        corpus.append(("recursion", 0, seal[:cut]))
    for circuit, s, words in corpus:
        want = _structure(r, circuit, s, words)
        assert want[0] is not None
        assert _structure_on(r, HOST, circuit, s, words) == want
        full = _verify(r, circuit, s, words)
        assert full[0] is not None and _verify_on(r, HOST, circuit, s, words) == full
    assert _verify_on(r, HOST, "nope", 0, seal) == _verify(r, "nope", 0, seal)
    assert "unknown circuit" in _verify(r, "nope", 0, seal)[0]


def test_verify_on_refuses_bad_arguments_without_a_device(r):
    L = r.lib()
    seal = np.zeros(16, np.uint32)
    po2 = C.c_uint32(0)
    for where in (-1, 2, 7):
        m = _msg(r, L.r0hip_verify_seal_on(where, b"recursion", 0, _p(seal), seal.size, None, 0, None, C.byref(po2)))
        assert m and "where" in m and str(where) in m, m
        m = _msg(r, L.r0hip_testing_verify_seal_structure_on(where, b"recursion", 0, _p(seal), seal.size,
                                                             C.byref(po2)))
        assert m and "where" in m, m
    for where in (HOST, DEVICE):
        m = _msg(r, L.r0hip_verify_seal_on(where, b"recursion", 0, None, 5, None, 0, None, C.byref(po2)))
        assert m and "seal is NULL" in m, m
        m = _msg(r, L.r0hip_verify_seal_on(where, b"recursion", 0, _p(seal), seal.size, None, 1, None, C.byref(po2)))
        assert m and "code_roots is NULL" in m, m
        m = _msg(r, L.r0hip_verify_seal_on(where, b"recursion", 3, _p(seal), seal.size, None, 0, None, C.byref(po2)))
        assert m and "unknown hash suite" in m, m
        m = _msg(r, L.r0hip_testing_verify_seal_structure_on(where, b"nope", 0, _p(seal), seal.size, C.byref(po2)))
        assert m and "unknown circuit" in m, m
        m = _msg(r, L.r0hip_testing_verify_seal_structure_on(where, b"recursion", 0, None, 3, C.byref(po2)))
        assert m and "seal is NULL" in m, m
    # a seal that ends before its first opening never reaches the device either
    m = _msg(r, L.r0hip_testing_verify_seal_structure_on(DEVICE, b"recursion", 0, _p(seal), seal.size, C.byref(po2)))
    assert m == _structure(r, "recursion", 0, seal)[0] == "seal too short"


def _open(r, suite, words, table, n_open=None, digests=True, status=True, words_null=False, table_null=False):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n = len(table) if n_open is None else n_open
    t = (r.Opening * max(len(table), 1))()
    for dst, o in zip(t, table):
        dst.row_off, dst.path_off, dst.index, dst.cols, dst.levels = o
    dg, st = np.zeros(8 * max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    return _msg(r, r.lib().r0hip_merkle_open_digests(
        suite, None if words_null else _p(words), words.size, None if table_null else C.cast(t, C.c_void_p), n,
        _p(dg) if digests else None, _p(st) if status else None))


def test_merkle_open_digests_refuses_malformed_tables_without_a_device(r):
    words = np.zeros(300, np.uint32)
    good = (0, 16, 5, 16, 2)  # row [0, 16), path [16, 32)
    for suite in (2, 3, -1):
        m = _open(r, suite, words, [good])
        assert m and "suite" in m and str(suite) in m, m
    m = _open(r, 0, words, [good], words_null=True)
    assert m and "h_words is NULL" in m, m
    m = _open(r, 0, words, [good], table_null=True)
    assert m and "h_open is NULL" in m, m
    m = _open(r, 1, words, [good], digests=False)
    assert m and "h_digests is NULL" in m, m
    m = _open(r, 1, words, [good], status=False)
    assert m and "h_status is NULL" in m, m
    for suite in (0, 1):
        for cols in (0, 257):
            m = _open(r, suite, words, [good, (0, 16, 5, cols, 2)])
            assert m and "h_open[1].cols" in m and str(cols) in m, m
        m = _open(r, suite, words, [good, good, (0, 16, 5, 16, 41)])
        assert m and "h_open[2].levels" in m and "41" in m, m
        # a row, then a path, that ends one word past n_words
        m = _open(r, suite, words, [(300 - 16 + 1, 0, 5, 16, 2)])
        assert m and "h_open[0].row_off" in m and "n_words" in m, m
        m = _open(r, suite, words, [good, (0, 300 - 16 + 1, 5, 16, 2)])
        assert m and "h_open[1].path_off" in m and "n_words" in m, m
        # offsets that would wrap a 64-bit sum
        m = _open(r, suite, words, [(2**64 - 8, 0, 5, 16, 0)])
        assert m and "h_open[0].row_off" in m, m
        m = _open(r, suite, words, [(0, 2**64 - 8, 5, 16, 2)])
        assert m and "h_open[0].path_off" in m, m
    # Poseidon2 rows are field elements
    bad = words.copy()
    bad[7] = 15 * (1 << 27) + 1  # p
    m = _open(r, 0, bad, [good])
    assert m and "h_words[7]" in m and "canonical" in m, m


def test_verify_argument_of_the_pipelines(r):
    """"device" or 2 passes R0HIP_VERIFY_RECEIPTS_DEVICE, True still passes 1"""
    from risc0_amd import hal
    assert hal._verify_mode(True) == 1 and hal._verify_mode(False) == 0 and hal._verify_mode(None) == 0
    assert hal._verify_mode("device") == hal._verify_mode(2) == hal.VERIFY_RECEIPTS_DEVICE == 2
    assert hal._verify_mode("host") == hal._verify_mode(1) == hal._verify_mode(3) == 1
    with pytest.raises(ValueError):
        hal._verify_mode("gpu")
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    for name, val in (("R0HIP_VERIFY_HOST", 0), ("R0HIP_VERIFY_DEVICE", 1), ("R0HIP_VERIFY_RECEIPTS_DEVICE", 2)):
        assert re.search(r"#define " + name + r"\s+" + str(val) + r"\b", hdr), name


NAMES = ("r0hip_verify_seal_on", "r0hip_testing_verify_seal_structure_on", "r0hip_merkle_open_digests")


def test_the_three_symbols_are_declared_everywhere(r):
    py = open(os.path.join(ROOT, "risc0_amd", "hal.py")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    for n in NAMES:
        assert n in r.exported_symbols() and hasattr(r.lib(), n), n
        assert f'"{n}"' in py, n
        assert re.search(r"pub fn " + n + r"\(", rs), n
    for name, val in (("R0HIP_VERIFY_HOST", 0), ("R0HIP_VERIFY_DEVICE", 1), ("R0HIP_VERIFY_RECEIPTS_DEVICE", 2)):
        assert re.search(r"pub const " + name + r": c_int = " + str(val) + ";", rs), name


def test_opening_struct_layout(r):
    """r0hip_opening: gcc's sizeof and offsetof against the ctypes mirror, and the Rust struct's
    fields in the header's order (the style of test_abi_layout.py)"""
    py = r.Opening
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(r0hip_opening));']
    for f in py._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof(r0hip_opening, {f[0]}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                            capture_output=True, text=True)
        if cc.returncode:
            pytest.fail("the header does not compile as C with these field names:\n" + cc.stderr)
        got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True,
                                                       check=True).stdout.split("\n") if ln)
    assert int(got["sizeof"]) == C.sizeof(py) == 32
    for f in py._fields_:
        assert int(got[f[0]]) == getattr(py, f[0]).offset, f[0]
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    m = re.search(r"typedef struct r0hip_opening \{(.*?)\} r0hip_opening;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    cfields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert cfields == [f[0] for f in py._fields_]
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\npub struct R0HipOpening \{(.*?)\n\}", rs, flags=re.S)
    assert m, "R0HipOpening"
    assert re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("row_off", "u64"), ("path_off", "u64"), ("index", "u64"),
                                                             ("cols", "u32"), ("levels", "u32")]
