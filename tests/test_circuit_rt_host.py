"""Circuits registered at run time (r0hip_circuit_register), the part that needs no GPU:
  * registration, listing, the descriptor and the unknown-circuit message;
  * a duplicate, the 65th registration and eight threads registering at once (in a process of
    their own: the registry has no way out, and a full one would starve the other tests);
  * one refusal per rule of the validation list, each made by breaking one field of the demo
    tables, each naming the field and leaving the registry as it was;
  * the host interpreter under a registered name: poly_ext on the recursion fixture, the violated
    term of a demo row, the committed demo seal verified with no GPU and no r0hip_init;
  * the ctypes struct against the header (offsetof probe);
  * the validator and the bytecode compiler as a stand-alone program under AddressSanitizer and
    UBSan: the three committed programs (slot counts within the live-value bounds measured on the
    programs, no slot read before it is written), and malformed programs refused."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import circuit_rt_util as U

ROOT = U.ROOT
GOLD = os.path.join(ROOT, "tests", "golden")
P = U.P


def enc(x):
    return np.array([(int(v) % P) * 2**32 % P for v in np.atleast_1d(x)], dtype=np.uint32)


# ---- registration and listing ----

def test_registration_listing_and_descriptor():
    from risc0_amd import hal
    before = hal.circuit_names()
    assert before[:3] == ["rv32im", "recursion", "demo"]
    for n in ("demo", "recursion", "rv32im"):
        rt = U.registered(n)
        got, want = hal.circuit_info(rt), hal.circuit_info(n)
        assert got.pop("name") == rt and want.pop("name") == n
        assert got == want
    names = hal.circuit_names()
    assert names[:3] == ["rv32im", "recursion", "demo"]
    reg = names[3:]
    assert {"rt_demo", "rt_recursion", "rt_rv32im"} <= set(reg)
    want = r"unknown circuit keccak \(compiled in: rv32im, recursion, demo; registered: " + ", ".join(reg) + r"\)$"
    z = np.zeros(64, np.uint32)
    with pytest.raises(hal.R0HipError, match=want):
        hal.circuit_info("keccak")
    with pytest.raises(hal.R0HipError, match=want):
        hal.poly_ext("keccak", z, z, z, z)
    with pytest.raises(hal.R0HipError, match=want):
        hal.verify_seal("keccak", 0, z)
    # a second registration of a name, compiled in or registered, is refused
    for taken in ("rt_demo", "demo"):
        with pytest.raises(hal.R0HipError, match=f"name: {taken} is taken"):
            hal.register_circuit(taken, U.CIRCUITS, files="demo")
    assert hal.circuit_names() == names
    # the testing chunk is the thread's, 0 until set
    assert hal.testing_set_interp_chunk(96) == 0
    assert hal.testing_set_interp_chunk(0) == 96


_FRESH = r"""
import sys, threading
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import circuit_rt_util as U
from risc0_amd import hal
z = __import__("numpy").zeros(8, "uint32")
try:
    hal.circuit_info("keccak")
except hal.R0HipError as e:
    assert str(e) == "r0hip: r0hip_circuit_info: unknown circuit keccak (compiled in: rv32im, recursion, demo)", str(e)
t = U.tables("demo")
errs = []
def reg(i):
    try:
        U.register_tables(t, f"thr_{i}")
    except Exception as e:
        errs.append(str(e))
th = [threading.Thread(target=reg, args=(i,)) for i in range(8)]
[x.start() for x in th]; [x.join() for x in th]
assert not errs, errs
names = hal.circuit_names()
assert sorted(names[3:]) == sorted(f"thr_{i}" for i in range(8)), names
for i in range(8, 64):
    U.register_tables(t, f"c{i}")
assert len(hal.circuit_names()) == 3 + 64
try:
    U.register_tables(t, "one_too_many")
    raise SystemExit("the 65th registration was accepted")
except hal.R0HipError as e:
    assert "registry is full (64 circuits)" in str(e), str(e)
assert len(hal.circuit_names()) == 3 + 64 and hal.circuit_info("c63")["n_taps"] == 16
print("ok")
"""


def test_concurrent_registration_and_the_limit_in_a_fresh_process():
    out = subprocess.run([sys.executable, "-c", _FRESH, ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- refusals ----

def _ir(t, k, field, value):
    t["ir"][6 * k + field] = value


def _tap(t, i, field, value):
    t["taps"][5 * i + field] = value


def _swap_taps(t):
    t["taps"][0:5], t["taps"][5:10] = t["taps"][5:10], t["taps"][0:5]


def _drop_arg(name):
    def f(t):
        from risc0_amd import circuit_tables
        t["eval_args"].remove(circuit_tables.ARGS[name])
    return f


# the demo program: record 0 `e`, 1 `l`, 5 `* 5 3 4`, 8 `a 8 0 7 0`, 9 `g 9 1 0`, last `r`
REFUSALS = [
    ("name_not_identifier", lambda t: t.update(name="2fast"), r"name: not a C identifier"),
    ("name_too_long", lambda t: t.update(name="x" * 32), r"name: not 1 to 31 characters"),
    ("name_taken", lambda t: t.update(name="recursion"), r"name: recursion is taken"),
    ("taps_unsorted", _swap_taps, r"taps: entry 1 is not sorted"),
    ("taps_group", lambda t: _tap(t, 15, 2, 3), r"taps: entry 15: group 3"),
    ("skip_does_not_tile", lambda t: _tap(t, 0, 4, 3), r"taps: entry \d+: skip \d+ does not tile"),
    ("combo_begin", lambda t: t.update(combo_begin=[0, 2, 3]), r"combo_begin: "),
    ("group_begin", lambda t: t.update(group_begin=[0, 7, 11, 16]), r"group_begin: entry 1 is 7"),
    ("group_sizes", lambda t: t.update(group_sizes=[4, 3, 4]), r"group_sizes: group 2 is 4"),
    ("n_groups", lambda t: t.update(n_groups=2), r"n_groups: 2 is not 3"),
    ("eval_args_value", lambda t: t["eval_args"].__setitem__(0, 5), r"eval_args: entry 0 is 5"),
    ("mix_size", lambda t: t.update(mix_size=1 << 24), r"mix_size: "),
    ("dst_not_dense", lambda t: _ir(t, 5, 1, 6), r"ir: record 5: dst 6 is not the next dense id 5"),
    ("operand_not_earlier", lambda t: _ir(t, 5, 2, 5), r"ir: record 5: operand id 5 is not below dst 5"),
    ("op_code", lambda t: _ir(t, 5, 0, 10), r"ir: record 5: op 10 is not one of"),
    ("no_r_record", lambda t: _ir(t, t["n_ir"] - 1, 0, 0), r"ir: record \d+: the last record is not the r record"),
    ("r_not_last", lambda t: _ir(t, 3, 0, 9), r"ir: record 3: the r record is not last"),
    ("r_names_nothing", lambda t: _ir(t, t["n_ir"] - 1, 1, t["n_ir"]), r"ir: record 67: r names value 68 before it is made"),
    ("l_tap_index", lambda t: _ir(t, 1, 2, 16), r"ir: record 1: l: tap index 16 is not below n_taps 16"),
    ("l_group_not_an_argument", _drop_arg("code"), r"ir: record 1: l: tap \d+ is of group 1, which eval_args does not have"),
    ("g_word_index", lambda t: _ir(t, 9, 3, 3), r"ir: record 9: g: word 3 is not below output_size 3"),
    ("g_not_an_argument", _drop_arg("global"), r"ir: record 9: g: eval_args has no global argument"),
    ("g_selector", lambda t: _ir(t, 9, 2, 2), r"ir: record 9: g: 2 is neither"),
    ("power_index", lambda t: _ir(t, 8, 4, 8), r"ir: record 8: power index 8 is not below n_poly_mix 8"),
    ("acc_is_fp", lambda t: _ir(t, 8, 2, 1), r"ir: record 8: the ACC operand 1 is an Fp value"),
    ("constant_not_canonical", lambda t: _ir(t, 0, 3, P), r"ir: record 0: e: a constant word is not below p"),
    ("n_ir_cap", lambda t: t.update(n_ir=(1 << 20) + 1), r"n_ir: 1048577 records exceed the cap of 1048576"),
    ("n_ir_zero", lambda t: t.update(n_ir=0), r"n_ir: 0 records"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_malformed_tables_are_refused_with_the_field_named(case):
    from risc0_amd import hal
    _, edit, want = case
    t = U.tables("demo")
    assert t["n_ir"] == 68 and t["n_taps"] == 16 and len(t["poly_mix_powers"]) == 8
    t["name"] = "refused"
    edit(t)
    before = hal.circuit_names()
    with pytest.raises(hal.R0HipError, match=r"r0hip_circuit_register: " + want):
        U.register_tables(t, t["name"])
    assert hal.circuit_names() == before and "refused" not in before


def test_struct_size_is_checked():
    from risc0_amd import hal
    s, keep = hal.circuit_tables_struct(U.tables("demo"), "refused")
    with pytest.raises(hal.R0HipError, match=r"t_size: \d+ is not sizeof\(r0hip_circuit_tables\)"):
        hal.check(hal.lib().r0hip_circuit_register(C.byref(s), C.sizeof(s) - 8))
    with pytest.raises(hal.R0HipError, match="t is NULL"):
        hal.check(hal.lib().r0hip_circuit_register(None, C.sizeof(s)))
    assert "refused" not in hal.circuit_names()


# ---- the host interpreter under a registered name ----

def test_poly_ext_equals_the_recursion_fixture():
    """tests/golden/poly_ext_recursion.npy on its seeded inputs, as tests/test_verifier.py reads it"""
    import oracle as O  # the input generator only: nothing is built
    import poly_ext_def as X
    from risc0_amd import hal
    rt = U.registered("recursion")
    want = np.load(os.path.join(GOLD, "poly_ext_recursion.npy"))
    info = hal.circuit_info(rt)
    pm, u, g, m = X.inputs(O, want.shape[0], info["n_taps"], info["mix_size"], info["output_size"])
    for k in range(0, want.shape[0], 20):
        a = hal.poly_ext("recursion", m[k], g[k], u[k], pm[k])
        b = hal.poly_ext(rt, m[k], g[k], u[k], pm[k])
        assert np.array_equal(a, want[k]) and np.array_equal(b, want[k]), k


def test_constraint_term_on_a_violated_demo_row():
    from risc0_amd import hal
    import demo_air as D
    rt = U.registered("demo")
    po2, n = 4, 12
    code, data, glob = D.witness(po2, n, 3, 5)
    mix = [7, P - 1, 12345, 1]
    acc = D.accumulate(po2, n, data, mix)
    x = D.enc([7, 11, 13, 17])
    rows = 1 << po2
    for broken in (False, True):
        d = np.array(data, dtype=np.uint64)
        if broken:
            d[5] = (int(d[5]) + 1) % P
        taps = D.taps_on_rows(code, d, acc, rows)
        row = D.enc([int(t[5]) for t in taps])
        want = hal.constraint_term("demo", row, D.enc(mix), D.enc(glob), x)
        got = hal.constraint_term(rt, row, D.enc(mix), D.enc(glob), x)
        assert got == want and (got is not None and got >= 0) == broken


def test_committed_demo_seal_verifies_under_the_registered_name():
    from risc0_amd import hal
    rt = U.registered("demo")
    seal = np.load(os.path.join(GOLD, "demo", "seal_demo_poseidon2_po2_8.npy"))
    assert hal.verify_seal(rt, 0, seal) == 8 == hal.verify_seal("demo", 0, seal)
    bad = seal.copy()
    bad[bad.size // 2] ^= 1
    with pytest.raises(hal.R0HipError):
        hal.verify_seal(rt, 0, bad)


# ---- the struct ----

def test_ctypes_struct_matches_the_c_header():
    from risc0_amd import hal
    cname, py = "r0hip_circuit_tables", hal.CircuitTables
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', "int main(void) {",
             f'  printf("sizeof %zu\\n", sizeof({cname}));']
    for f in py._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out if ln}
    assert got.pop("sizeof") == C.sizeof(py)
    assert got == {f[0]: getattr(py, f[0]).offset for f in py._fields_}
    # the header's fields, in its order, are the mirror's
    import re
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in py._fields_]
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    m = re.search(r"pub struct R0HipCircuitTables \{(.*?)\n\}", rs, flags=re.S)
    assert re.findall(r"pub (\w+):", m.group(1)) == fields


# ---- the validator and compiler under a sanitizer, as a program of their own ----

def _write_tables(path, t):
    with open(path, "w") as f:
        f.write(f"name 1 {t['name']}\n")
        info = t["circuit_info"].encode()
        f.write(f"info {len(info)} " + " ".join(str(b) for b in info) + "\n")
        for k in ("taps", "combo_taps", "combo_begin", "group_begin", "group_sizes", "poly_mix_powers", "eval_args", "ir"):
            f.write(f"{k} {len(t[k])} " + " ".join(str(int(v)) for v in t[k]) + "\n")
        for k in ("n_taps", "combos_count", "n_groups", "mix_size", "output_size", "n_ir"):
            f.write(f"{k} 1 {int(t[k])}\n")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("circuit_rt_check")
    exe = str(d / "circuit_rt_check")
    csrc = os.path.join(ROOT, "risc0_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-Wall", "-Wextra", "-I", csrc, os.path.join(ROOT, "tests", "circuit_rt_check.cpp"),
                         os.path.join(csrc, "circuit_rt.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe, d


# max live Fp and FpExt values of the committed programs in program order, every value counted
# (leaves included): the interpreter's slot files, which hold computed values only, stay within them
LIVE_BOUNDS = {"demo": (14, 4), "recursion": (1001, 10), "rv32im": (818, 104)}
RECORDS = {"demo": 68, "recursion": 12334, "rv32im": 20092}


@pytest.mark.parametrize("name", ["demo", "recursion", "rv32im"])
def test_compiler_under_sanitizers_on_the_committed_programs(checker, name):
    exe, d = checker
    t = U.tables(name)
    assert t["n_ir"] == RECORDS[name]
    path = str(d / f"{name}.tables")
    _write_tables(path, t)
    fp, ext = LIVE_BOUNDS[name]
    out = subprocess.run([exe, "good", path, str(fp), str(ext)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    assert out.stdout.startswith("records ")


def test_validator_under_sanitizers_refuses_malformed_programs(checker):
    exe, d = checker
    for cid, edit, want in REFUSALS:
        if cid == "name_taken":
            continue  # the registry's rule, not the validator's
        t = U.tables("demo")
        edit(t)
        path = str(d / f"bad_{cid}.tables")
        _write_tables(path, t)
        out = subprocess.run([exe, "bad", path], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (cid, out.stdout, out.stderr)
        import re
        assert re.search(want, out.stdout), (cid, out.stdout)
