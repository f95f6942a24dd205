"""The native recursion preflight (r0hip_recursion_preflight, risc0_amd/csrc/recursion_preflight.cpp)
without a device: word for word against the restatement of Preflight::step in
tests/recursion_program.py on random and hand-encoded programs, every run-time failure with its
message and cycle, the decoder's refusals, the address cap, the size query, the tables that
depend on the program alone, and the layout of the new structs in C, ctypes and Rust."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import recursion_input_programs as IP
import recursion_program as RP
import recursion_sha_program as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32p = C.POINTER(C.c_uint32)
SEEDS = range(9100, 9120)  # 20 seeds; the coverage they give is asserted below
SIZES = (200, 1024)


def _native(prog, inp, po2=11):
    import risc0_amd as r
    return r.recursion_preflight(prog.encoded(), po2, inp)


def _compare(prog, inp, po2=11):
    """the native arrays against the restatement's, word for word"""
    pf = S.preflight(prog, inp)  # recursion_program.Preflight plus the SHA macro ops
    wom, cyc, iops = RP.trace_arrays(pf)
    n_wom, n_cyc, n_iops, n_out = _native(prog, inp, po2)
    assert n_wom.shape == wom.shape and np.array_equal(n_wom, wom), "wom"
    assert np.array_equal(n_cyc, np.array(cyc, dtype=np.uint32).reshape(-1, 2)), "cycles"
    assert n_iops.shape == iops.shape and np.array_equal(n_iops, iops), "iops"
    assert [int(x) for x in n_out] == [int(x) for x in pf.output], "output"
    return pf


@pytest.fixture(scope="module")
def random_programs():
    return [(seed, size, *RP.random_program(np.random.default_rng(seed), size)) for seed in SEEDS for size in SIZES]


def test_parity_with_the_restatement_on_random_programs(random_programs):
    """word for word on every program; and over the seeds every selector the preflight runs, every
    macro op random_program emits and every micro opcode 0..10 occurs, with an ADD that writes an
    output (the SHA macro ops have hand-encoded programs below)"""
    sels, macros, opcodes, outputs = set(), set(), set(), 0
    for seed, size, prog, inp in random_programs:
        try:
            _compare(prog, inp)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} max_rows {size}: {e}") from None
        for row in prog.rows:
            sels |= {name for name, col in RP.SEL.items() if row[col] == 1}
            if row[RP.SEL["macro"]] == 1:
                macros |= {name for name, col in RP.MACRO.items() if row[col] == 1}
            if row[RP.SEL["micro"]] == 1:
                for i in range(3):
                    opcodes.add(row[8 + 4 * i])
                    outputs += row[8 + 4 * i] == RP.ADD and row[11 + 4 * i] != 0
    assert sels == {"micro", "macro", "p2_load", "p2_full", "p2_partial", "p2_store"}
    assert macros == {"wom_init", "wom_fini", "set_global", "bit_and_elem", "bit_op_shorts"}
    assert opcodes == set(range(11))
    assert outputs > 0


@pytest.mark.parametrize("name", sorted(IP.CASES))
def test_hand_encoded_programs(name):
    prog, inp = IP.CASES[name]()
    pf = _compare(prog, inp)
    assert len(pf.cycles) == len(prog.rows)


def test_hand_encoded_programs_pin_what_they_claim():
    """the corners the programs are named for are in their traces"""
    prog, inp = IP.CASES["select_corners"]()
    wom = _native(prog, inp)[0]
    assert [RP.dec(wom[a][0]) for a in (6, 7, 8, 9, 10)] == [11, 33, 33, 22, 1]
    prog, inp = IP.CASES["inv_modes"]()
    wom = _native(prog, inp)[0]
    assert [RP.dec(wom[a][0]) for a in (6, 7, 8)] == [1, 0, 1]
    assert not wom[11].any() and wom[10].all()  # inv(0) = 0; the inverse of (3, 4) has every limb
    prog, inp = IP.CASES["outputs"]()
    assert [int(x) for x in _native(prog, inp)[3]] == [10, 30, 40]
    prog, inp = IP.CASES["iop_raw_words"]()
    iops = _native(prog, inp)[2]
    assert [int(x) for x in iops[1]] == [1, 2**31 - RP.P, 1, 5]  # the raw words mod p, no do_mont
    prog, inp = IP.CASES["full_po2_11"]()
    assert len(prog.rows) == 2**11 - 1024
    cyc = _native(prog, inp)[1]
    assert cyc.shape == (2**11 - 1024, 2) and cyc[:, 1].all() and not cyc[:, 0].any()


@pytest.mark.parametrize("form", [0, 1])
def test_both_code_forms(form):
    import risc0_amd as r
    prog, inp = RP.random_program(np.random.default_rng(77), 300)
    code = prog.encoded() if form == 0 else np.array([RP.enc(int(x)) for x in prog.encoded()], dtype=np.uint32)
    want = _native(prog, inp)
    got = r.recursion_preflight(code, 11, inp, form=form)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    if form == 0:  # Elem::from reduces every word
        shifted = (code.astype(np.uint64) + RP.P * (code < 2**32 - RP.P)).astype(np.uint32)
        for a, b in zip(r.recursion_preflight(shifted, 11, inp), want):
            assert np.array_equal(a, b)
    else:
        code[5] = RP.P
        with pytest.raises(r.R0HipError, match=r"code word 5 = 2013265921 is not a canonical Montgomery word"):
            r.recursion_preflight(code, 11, inp, form=1)


# failures the restatement shares, and what it raises there
RESTATED = dict(eq=ValueError, overwrite=ValueError, illegal_row=ValueError, selector_two=ValueError,
                unknown_opcode=ValueError, input_exhausted=IndexError, empty_body=IndexError,
                read_past_memory=IndexError)


@pytest.mark.parametrize("name", sorted(IP.ERRORS))
def test_run_time_failures(name):
    import risc0_amd as r
    prog, inp, po2, pattern = IP.ERRORS[name]()
    with pytest.raises(r.R0HipError, match=pattern):
        _native(prog, inp, po2)
    if name in RESTATED:
        with pytest.raises(RESTATED[name]):
            S.preflight(prog, inp)


def test_the_cap_moves_with_po2():
    """a write at 16 * 2^11 is refused at po2 11 and runs at po2 12"""
    import risc0_amd as r
    prog, inp, _po2, _pattern = IP.ERRORS["cap_write"]()
    with pytest.raises(r.R0HipError, match="cap of 16"):
        _native(prog, inp, 11)
    wom = _native(prog, inp, 12)[0]
    assert wom.shape == ((16 << 11) + 3, 4) and RP.dec(wom[16 << 11][0]) == 1


def test_the_decoder_refuses_what_no_witness_generator_runs():
    import risc0_amd as r
    prog, pattern = IP.refused_checked_bytes()
    with pytest.raises(r.R0HipError, match=pattern):
        _native(prog, [])


@pytest.mark.skipif(not RP.available(), reason="oracle/_ref/libref_recursion.so is not built")
@pytest.mark.parametrize("name", ["sha_shorts", "sha_montgomery"])
def test_sha_programs_satisfy_the_circuit_from_the_native_arrays(name):
    """the compiled reference witness generator accepts the native preflight's arrays of a program
    with SHA compressions (it reads the digests back, so a wrong word breaks the memory argument),
    and the circuit's constraints hold on every row"""
    prog, inp = IP.CASES[name]()
    wom, cyc, iops, _out = _native(prog, inp)

    class _Trace:  # the native arrays where recursion_program.witgen reads a Preflight's
        pass
    pf = _Trace()
    pf.wom = [tuple(RP.dec(x) for x in cell) for cell in wom]
    pf.cycles = [tuple(int(x) for x in c) for c in cyc]
    pf.iops = [tuple(RP.dec(x) for x in v) for v in iops]
    ctrl, data, glob = RP.witgen(prog, pf, 11, noise_seed=1)
    mix = np.array([RP.enc(int(x)) for x in np.random.default_rng(5).integers(1, RP.P, RP.MIX)], dtype=np.uint32)
    w = dict(ctrl=ctrl, data=data, glob=glob, work=len(prog.rows), acc0=RP.accum_init(11, noise_seed=3))
    rc = RP.row_constraints(ctrl, data, RP.accumulate(w, mix, 11), glob, mix, 11)
    assert not rc.any(), f"constraints fail on rows {np.nonzero(rc.any(axis=0))[0][:8]}"
    # every SHA macro op and both load subtypes are in the program
    macros = {n for row in prog.rows if row[RP.SEL["macro"]] == 1 for n, col in RP.MACRO.items() if row[col] == 1}
    assert {"sha_init", "sha_load", "sha_mix", "sha_fini"} <= macros
    assert {row[RP.MACRO_OPERAND + 2] for row in prog.rows if row[RP.MACRO["sha_load"]] == 1
            and row[RP.SEL["macro"]] == 1} == {0, 1}


def _call(code, po2, inp, caps, bufs=True, form=0, n_words=None):
    """r0hip_recursion_preflight with explicit capacities; returns (error or None, counts)"""
    import risc0_amd as r
    L = r.lib()
    c = np.ascontiguousarray(code, dtype=np.uint32)
    x = np.ascontiguousarray(inp, dtype=np.uint32)
    n = [C.c_size_t(12345) for _ in range(4)]
    arrs = [np.zeros(max(1, cap * w), dtype=np.uint32) for cap, w in zip(caps, (4, 2, 4, 1))]
    ptr = [a.ctypes.data_as(u32p) if bufs else None for a in arrs]
    err = L.r0hip_recursion_preflight(c.ctypes.data_as(u32p), c.size if n_words is None else n_words, form, po2,
                                      x.ctypes.data_as(u32p) if x.size else None, x.size, ptr[0], caps[0],
                                      C.byref(n[0]), ptr[1], caps[1], C.byref(n[1]), ptr[2], caps[2], C.byref(n[2]),
                                      ptr[3], caps[3], C.byref(n[3]))
    msg = None
    if err:
        msg = C.cast(err, C.c_char_p).value.decode()
        L.r0hip_free_error(err)
    return msg, [k.value for k in n]


def test_size_query_and_buffer_checks():
    prog, inp = RP.random_program(np.random.default_rng(3), 200)
    pf = RP.preflight(prog, inp)
    want = [len(pf.wom), len(prog.rows), len(pf.iops), len(pf.output)]
    msg, counts = _call(prog.encoded(), 11, [], (0, 0, 0, 0), bufs=False)  # needs no input: nothing runs
    assert msg is None and counts == want
    msg, counts = _call(prog.encoded(), 11, inp, want)
    assert msg is None and counts == want
    for i in range(4):
        if want[i] == 0:
            continue
        caps = list(want)
        caps[i] -= 1
        msg, counts = _call(prog.encoded(), 11, inp, caps)
        assert msg is not None and "too small" in msg and counts == want
    for kwargs, needle in ((dict(po2=10), "po2 10"), (dict(po2=25), "po2 25"), (dict(form=2), "form 2"),
                           (dict(n_words=22), "multiple of 23"), (dict(n_words=0), "no rows")):
        po2 = kwargs.pop("po2", 11)
        msg, _ = _call(prog.encoded(), po2, inp, want, **kwargs)
        assert msg is not None and needle in msg, (needle, msg)
    too_long = np.zeros(23 * (2**11 - 1024 + 1), dtype=np.uint32)
    msg, _ = _call(too_long, 11, [], (0, 0, 0, 0), bufs=False)
    assert msg is not None and "above 2^po2 - ZK_CYCLES = 1024" in msg


def test_cycles_and_counts_depend_on_the_program_alone():
    """two inputs of one program: the same cycles and counts, another WOM and other IOP values"""
    b = RP.Builder(np.random.default_rng(11))
    for _ in range(6):
        b.block_iop()
        b.block_arith()
    prog, inp_a = b.finish()
    inp_b = [int(x) for x in np.random.default_rng(99).integers(0, RP.P, len(inp_a))]
    a, bb = _native(prog, inp_a), _native(prog, inp_b)
    assert np.array_equal(a[1], bb[1])
    assert a[0].shape == bb[0].shape and a[2].shape == bb[2].shape and a[3].shape == bb[3].shape
    assert not np.array_equal(a[0], bb[0]) and not np.array_equal(a[2], bb[2])
    _compare(prog, inp_b)


# ---- layout ---------------------------------------------------------------------------------
def _c_layout(structs):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                            capture_output=True, text=True)
        assert cc.returncode == 0, "the header does not compile as C11:\n" + cc.stderr
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    return {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln}


def test_new_structs_match_the_c_header():
    """offsetof probe of r0hip_worker_input_job and r0hip_recursion_input_info against their
    ctypes mirrors; r0hip_worker_job keeps its size and the handle its offset"""
    from risc0_amd import hal
    structs = {"r0hip_worker_input_job": hal.WorkerInputJobStruct, "r0hip_recursion_input_info": hal.RecursionInputInfo,
               "r0hip_worker_program_job": hal.WorkerProgramJobStruct, "r0hip_worker_job": hal.WorkerJobStruct}
    got = _c_layout(structs)
    for cname, py in structs.items():
        assert got[(cname, "sizeof")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])
    assert got[("r0hip_worker_input_job", "job")] == 0
    assert got[("r0hip_worker_input_job", "program")] == got[("r0hip_worker_program_job", "program")] \
        == got[("r0hip_worker_job", "sizeof")]


def test_rust_mirrors_list_the_header_fields_in_order():
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    for rname, cname in (("R0HipWorkerInputJob", "r0hip_worker_input_job"),
                         ("R0HipRecursionInputInfo", "r0hip_recursion_input_info")):
        m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S)
        assert m, cname
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        cfields = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        m = re.search(r"pub struct " + rname + r" \{(.*?)\n\}", rs, flags=re.S)
        assert m, rname
        assert re.findall(r"pub (\w+):", m.group(1)) == cfields, rname
    assert re.search(r"pub const R0HIP_JOB_RECURSION_INPUT: u32 = 4;", rs)
    assert re.search(r"#define R0HIP_JOB_RECURSION_INPUT 4\b", hdr)


def test_every_new_symbol_is_exported_and_bound():
    import risc0_amd as r
    L = r.lib()
    for name in ("r0hip_recursion_preflight", "r0hip_recursion_program_prepare_input",
                 "r0hip_recursion_program_input_info", "r0hip_prove_recursion_program_input",
                 "r0hip_recursion_last_preflight_ms"):
        assert name in r.exported_symbols()
        assert getattr(L, name).argtypes is not None
    for method in ("preflight", "prove_input", "prepare_input", "input_info"):
        assert callable(getattr(r.RecursionProgram, method))
    assert callable(r.Worker.submit_recursion_input)
    # the from-input entry points refuse a NULL handle on the host
    for call in (lambda: L.r0hip_recursion_program_prepare_input(None),
                 lambda: L.r0hip_recursion_program_input_info(None, None)):
        err = call()
        assert err
        L.r0hip_free_error(err)
