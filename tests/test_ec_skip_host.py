"""CPU check of eval_check's kernel skipping (tools/gen_eval_check.py: gates, plan, the finishing
kernel), on the generated kernels' host translation units (`--host` for eval_check on the 4N
domain, `--host-rows` for the constraint-rows family), g++, as test_ec_host.py.

A term of poly_fp that has a selector column as a plain factor is exactly 0 where that column is
zero on the whole domain, so a kernel holding only such terms is not launched. The host entry point
<family>_host_<circuit>_skip takes the mask of dead gates and runs the launcher's own decision
function (plan). Its output must be the reference's word for word (eval_check: the numpy IR
interpreter, ec_extreme.reference; rows: the scalar restatement of the program on each row,
constraint_rows_ref.evaluate_row) and equal the run with no gate dead. Every output and scratch
buffer starts as 0xFFFFFFFF, so a kernel that was needed and did not run shows. The mask comes from
the zero scan's host restatement (ec_zero_scan.h), checked against numpy. The number of kernels
left out is checked per pattern against ec_skip_patterns.SKIPPED, which the device test
(test_ec_skip_gpu.py) checks r0hip_eval_check_launched against as well."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_rows_ref as CR
import ec_skip_patterns as S
from ec_extreme import enc, extreme_inputs, reference
from test_golden import e_mul, e_pow, rou_fwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 15 * 2**27 + 1
PO2 = 2
u32p = C.POINTER(C.c_uint32)
FAMILY = {"ec": ("--host", "ec_host_"), "rows": ("--host-rows", "rows_host_")}
CASES = [(c, f) for c in ("rv32im", "recursion") for f in ("ec", "rows")]


def ptr(a):
    return a.ctypes.data_as(u32p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(circuit, family) -> (library, entry prefix, gates as (buffer name, column), kernels)"""
    d = tmp_path_factory.mktemp("ec_skip_host")
    out = {}
    for circuit, fam in CASES:
        flag, prefix = FAMILY[fam]
        src, so = d / f"{fam}_{circuit}.cpp", d / f"{fam}_{circuit}.so"
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_eval_check.py"), flag, circuit,
                               str(src)], stdout=subprocess.DEVNULL)
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "risc0_amd", "csrc"), str(src), "-o", str(so)])
        lib = C.CDLL(str(so))
        fn = prefix + circuit
        getattr(lib, fn + "_scan").restype = C.c_uint64
        arg, col, nk = (C.c_int * 64)(), (C.c_int * 64)(), C.c_int()
        n = getattr(lib, fn + "_gates")(arg, col, C.byref(nk))
        names = json.load(open(os.path.join(ROOT, "risc0_amd", "circuits", circuit + ".taps.json")))["eval_args"]
        out[circuit, fam] = (lib, fn, [(names[arg[g]], col[g]) for g in range(n)], nk.value)
    return out


def numpy_mask(plain, gates, D):
    return sum(1 << g for g, (b, c) in enumerate(gates) if not plain[b][c * D:(c + 1) * D].any())


def tables(lib, fn, d, poly_mix):
    combos, npm = C.POINTER(C.c_int)(), C.c_int()
    ncomb = getattr(lib, fn + "_combos")(C.byref(combos), C.byref(npm))
    pows = [e_pow(poly_mix, k) for k in d["poly_mix_powers"]][:npm.value]
    k = 0
    for _ in range(ncomb):
        n = combos[k]
        prod = (1, 0, 0, 0)
        for q in range(n):
            prod = e_mul(prod, pows[combos[k + 1 + q]])
        k += 1 + n
        pows.append(prod)
    pm = enc([x for t in pows for x in t])
    pmn = enc([x * (P - 11) for t in pows for x in t])
    w = rou_fwd()[PO2 + 2]
    vinv = enc([pow((pow(3 * pow(w, q, P) % P, 1 << PO2, P) - 1) % P, P - 2, P) for q in range(4)])
    return pm, pmn, vinv


def run_skip(lib, fn, d, plain, tabs, D, dead):
    """(check planes, accumulator, kernels run, the scan's mask); dead None = the scan's mask"""
    pm, pmn, vinv = tabs
    acc = np.full(4 * D, 0xFFFFFFFF, np.uint32)
    mf = np.full(64 * D, 0xFFFFFFFF, np.uint32)
    me = np.full(64 * 4 * D, 0xFFFFFFFF, np.uint32)
    check = np.full(4 * D, 0xFFFFFFFF, np.uint32)
    arrs = [enc(plain[a]) for a in d["eval_args"]]
    argv = (u32p * len(arrs))(*[ptr(a) for a in arrs])
    scan = getattr(lib, fn + "_scan")(argv, C.c_uint32(D))
    launched = getattr(lib, fn + "_skip")(argv, ptr(pm), ptr(pmn), ptr(vinv), ptr(acc), ptr(mf), ptr(me), ptr(check),
                                          C.c_uint32(D), C.c_uint64(scan if dead is None else dead))
    return check, acc, launched, scan


def rows_reference(circuit, d, plain, poly_mix, n):
    """poly_fp on each of the n trace rows, Montgomery words, AoS"""
    w = {k: enc(v) for k, v in plain.items()}
    taps = CR.gather_taps(circuit, [w[g] for g in ("accum", "code", "data")], n.bit_length() - 1)
    out = []
    for row in range(n):
        val, _, res = CR.evaluate_row(circuit, taps[row], w["mix"], w["global"], enc(poly_mix))
        out += [CR.enc(x) for x in CR._ext(val[res])]
    return np.array(out, np.uint32)


@pytest.mark.parametrize("circuit, fam", CASES, ids=[f"{c}-{f}" for c, f in CASES])
def test_skipped_kernels_leave_the_result_unchanged(host, oracle, circuit, fam):
    lib, fn, gates, nk = host[circuit, fam]
    assert nk == S.KERNELS[circuit, fam]
    d = oracle.load_circuit_json(circuit)
    # eval_check: the 4N domain of po2 2; rows: its N = 4 trace rows (the generator draws 4 << po2 points)
    D = 4 << PO2 if fam == "ec" else 1 << PO2
    base, poly_mix = extreme_inputs(d, "edge_mix", PO2 if fam == "ec" else 0)
    assert numpy_mask(base, gates, D) == 0, "the base inputs must have no zero gate column"
    tabs = tables(lib, fn, d, poly_mix)
    skipped = {}
    for name, cols in S.patterns(circuit).items():
        plain = S.zeroed(base, cols, D)
        want_mask = numpy_mask(plain, gates, D)
        check, acc, launched, scan = run_skip(lib, fn, d, plain, tabs, D, None)
        assert scan == want_mask, (name, hex(scan), hex(want_mask))
        all_check, all_acc, all_launched, _ = run_skip(lib, fn, d, plain, tabs, D, 0)
        assert all_launched == nk, name
        if fam == "ec":
            ref = enc(reference(circuit, d, plain, poly_mix, PO2).reshape(-1))
            assert np.array_equal(all_check, ref), name
            assert np.array_equal(check, ref), name
        else:
            ref = rows_reference(circuit, d, plain, poly_mix, D)
            assert np.array_equal(all_acc, ref), name
            assert np.array_equal(acc, ref), name
        skipped[name] = nk - launched
    print(circuit, fam, skipped)
    assert any(skipped.values()), "no pattern skipped a kernel"
    assert skipped == S.SKIPPED[circuit, fam]


def test_a_dead_last_kernel_is_replaced_by_the_finishing_kernel(host, oracle):
    """rv32im's last kernel holds one term, gated by data column 12 (BigInt): with that column zero
    the kernel does not run and the check planes come from the finishing kernel"""
    lib, fn, gates, nk = host["rv32im", "ec"]
    d = oracle.load_circuit_json("rv32im")
    D = 4 << PO2
    base, poly_mix = extreme_inputs(d, "edge_mix", PO2)
    plain = S.zeroed(base, [("data", 12)], D)
    tabs = tables(lib, fn, d, poly_mix)
    check, _, launched, scan = run_skip(lib, fn, d, plain, tabs, D, None)
    assert scan == 1 << gates.index(("data", 12))
    assert launched < nk
    assert not (check == 0xFFFFFFFF).any()
    assert np.array_equal(check, enc(reference("rv32im", d, plain, poly_mix, PO2).reshape(-1)))
