"""Build-time plug-in circuits and the demo circuit, without a GPU: the generators (the circuit
list from data, refusals of malformed input), the host evaluation of the demo circuit against its
AIR written down directly (tests/demo_air.py), the committed demo seal, the new host-only entry
points and their refusals."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import demo_air as D
import ir_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCUITS = os.path.join(ROOT, "risc0_amd", "circuits")
TOOLS = os.path.join(ROOT, "tools")
GOLD = os.path.join(ROOT, "tests", "golden", "demo")
P = D.P


def _run(tool, *args, extra=None):
    env = dict(os.environ)
    env.pop("EXTRA_CIRCUIT_DIRS", None)
    if extra is not None:
        env["EXTRA_CIRCUIT_DIRS"] = extra
    return subprocess.run([sys.executable, os.path.join(TOOLS, tool), *args], env=env, capture_output=True, text=True)


def _plugin_dir(tmp, name="demo2", edit=None, ir_edit=None, file_name=None):
    """A directory holding the demo circuit under another name, optionally damaged."""
    d = os.path.join(tmp, "plug")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(CIRCUITS, "demo.taps.json")) as f:
        t = json.load(f)
    t["name"] = name
    if edit:
        edit(t)
    fn = file_name or name
    with open(os.path.join(d, fn + ".taps.json"), "w") as f:
        json.dump(t, f)
    with open(os.path.join(CIRCUITS, "demo.poly.ir")) as f:
        lines = f.read().split("\n")
    if ir_edit:
        lines = ir_edit(lines)
    with open(os.path.join(d, fn + ".poly.ir"), "w") as f:
        f.write("\n".join(lines))
    return d


# ---- generators ----

def test_demo_generator_reproduces_the_committed_files(tmp_path):
    r = _run("gen_demo_circuit.py", str(tmp_path))
    assert r.returncode == 0, r.stderr
    for fn in ("demo.poly.ir", "demo.taps.json"):
        with open(os.path.join(CIRCUITS, fn), "rb") as a, open(tmp_path / fn, "rb") as b:
            assert a.read() == b.read(), fn


def test_plugin_list_emits_the_plugged_in_circuit(tmp_path):
    d = _plugin_dir(str(tmp_path))
    out = tmp_path / "circuits.cpp"
    r = _run("gen_circuits_inc.py", str(out), extra=d)
    assert r.returncode == 0, r.stderr
    src = out.read_text()
    for n in ("rv32im", "recursion", "demo", "demo2"):
        assert f'{{"{n}", {n}_taps,' in src, n
        assert f"eval_check_{n}, eval_check_{n}_info, constraint_rows_{n}, constraint_rows_{n}_info" in src, n
    assert src.index('{"recursion",') < src.index('{"demo",') < src.index('{"demo2",')
    r = _run("circuit_files.py", "--names", extra=d)
    assert r.stdout.split() == ["rv32im", "recursion", "demo", "demo2"]
    # both kernel families of the plugged-in circuit, from its own directory, without a tuning file
    r = _run("gen_eval_check.py", "demo2", str(tmp_path / "gen"), extra=d)
    assert r.returncode == 0, r.stderr
    made = sorted(os.listdir(tmp_path / "gen"))
    assert "eval_check_demo2.hip" in made and "rows_demo2.hip" in made, made
    assert "void constraint_rows_demo2(" in (tmp_path / "gen" / "rows_demo2.hip").read_text()
    # without the variable the list is the built-in three
    assert _run("circuit_files.py", "--names").stdout.split() == ["rv32im", "recursion", "demo"]


def _swap(i, j):
    def f(t):
        t["taps"][i], t["taps"][j] = t["taps"][j], t["taps"][i]
    return f


def _set(key, value):
    def f(t):
        t[key] = value
    return f


def _tap_field(i, k, v):
    def f(t):
        t["taps"][i][k] = v
    return f


def _ir_replace(old, new):
    def f(lines):
        assert old in lines
        return [new if ln == old else ln for ln in lines]
    return f


MALFORMED = {
    # case: (plug-in arguments, file the message names, field the message names)
    "name_not_identifier": (dict(name="bad-name"), "bad-name.taps.json", "name"),
    "name_collides_shipped": (dict(name="rv32im"), "rv32im.taps.json", "name"),
    "name_collides_demo": (dict(name="demo"), "demo.taps.json", "name"),
    "name_field_differs": (dict(name="other", file_name="demo2"), "demo2.taps.json", "name"),
    "taps_not_sorted": (dict(edit=_swap(0, 1)), "demo2.taps.json", "taps"),
    "skip_does_not_tile": (dict(edit=_tap_field(15, 4, 2)), "demo2.taps.json", "skip"),
    "skip_splits_a_register": (dict(edit=lambda t: (_tap_field(0, 4, 1)(t), _tap_field(1, 4, 1)(t))),
                               "demo2.taps.json", "skip"),
    "combo_begin": (dict(edit=_set("combo_begin", [0, 2, 3])), "demo2.taps.json", "combo_begin"),
    "group_begin": (dict(edit=_set("group_begin", [0, 8, 12, 16])), "demo2.taps.json", "group_begin"),
    "group_sizes": (dict(edit=_set("group_sizes", [4, 3, 4])), "demo2.taps.json", "group_sizes"),
    "circuit_info_15_bytes": (dict(edit=_set("circuit_info", "R0HIPDEMO:rev1v")), "demo2.taps.json", "circuit_info"),
    "ir_unknown_tap": (dict(ir_edit=_ir_replace("l 2 2 2 0", "l 2 2 2 1")), "demo2.poly.ir", "l record"),
    "ir_unknown_column": (dict(ir_edit=_ir_replace("l 2 2 2 0", "l 2 2 3 0")), "demo2.poly.ir", "l record"),
    "ir_unknown_global": (dict(ir_edit=_ir_replace("g 9 1 0", "g 9 1 3")), "demo2.poly.ir", "g record"),
    "ir_unknown_argument": (dict(ir_edit=_ir_replace("g 9 1 0", "g 9 5 0")), "demo2.poly.ir", "g record"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_plugin_is_refused_with_file_and_field(case, tmp_path):
    kw, file_named, field = MALFORMED[case]
    d = _plugin_dir(str(tmp_path), **kw)
    out = tmp_path / "circuits.cpp"
    r = _run("gen_circuits_inc.py", str(out), extra=d)
    assert r.returncode != 0 and not out.exists(), (r.stdout, r.stderr)
    assert file_named in r.stderr and field in r.stderr, r.stderr
    # the list the Makefile asks for is refused the same way, so the build stops before it generates
    r = _run("circuit_files.py", "--names", extra=d)
    assert r.returncode != 0 and file_named in r.stderr and not r.stdout.strip(), (r.stdout, r.stderr)


def _make_circuits(*args):
    """what the Makefile takes as CIRCUITS (parsed only: one rule added that prints it)"""
    env = dict(os.environ)
    env.pop("EXTRA_CIRCUIT_DIRS", None)
    env.pop("MAKEFLAGS", None)
    return subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "risc0_amd", "csrc"),
                           "--eval=print-circuits: ; @echo CIRCUITS=$(CIRCUITS)", "print-circuits", *args],
                          env=env, capture_output=True, text=True)


def test_makefile_takes_the_list_from_data(tmp_path):
    mk = open(os.path.join(ROOT, "risc0_amd", "csrc", "Makefile")).read()
    assert "CIRCUITS := rv32im recursion" not in mk and "circuit_files.py --names" in mk
    assert "EXTRA_CIRCUIT_DIRS ?=\n" in mk  # empty by default
    r = _make_circuits()
    assert r.returncode == 0 and "CIRCUITS=rv32im recursion demo\n" in r.stdout, (r.stdout, r.stderr)
    d = _plugin_dir(str(tmp_path))
    r = _make_circuits(f"EXTRA_CIRCUIT_DIRS={d}")  # a variable given on the command line reaches the list
    assert r.returncode == 0 and "CIRCUITS=rv32im recursion demo demo2\n" in r.stdout, (r.stdout, r.stderr)
    bad = _plugin_dir(str(tmp_path / "bad"), edit=_set("group_sizes", [4, 3, 4]))
    r = _make_circuits(f"EXTRA_CIRCUIT_DIRS={bad}")
    assert r.returncode != 0 and "group_sizes" in r.stderr and "refused" in r.stderr, (r.stdout, r.stderr)


# ---- the library's view ----

def test_circuit_info_and_names():
    from risc0_amd import hal
    assert hal.circuit_names()[:3] == ["rv32im", "recursion", "demo"]
    assert hal.circuit_info("demo") == {"name": "demo", "group_sizes": [4, 3, 3], "mix_size": 4, "output_size": 3,
                                        "n_taps": 16, "info": b"R0HIPDEMO:rev1v1"}
    for n in ("rv32im", "recursion"):
        with open(os.path.join(CIRCUITS, n + ".taps.json")) as f:
            t = json.load(f)
        i = hal.circuit_info(n)
        assert (i["group_sizes"], i["mix_size"], i["output_size"], i["n_taps"], i["info"]) == \
            (t["group_sizes"], t["mix_size"], t["output_size"], len(t["taps"]), t["circuit_info"].encode())
    d = hal.CircuitDesc()
    L = hal.lib()
    for args, word in (((b"demo", C.byref(d), C.sizeof(d) - 4, None, 0), "out_size"),
                       ((b"demo", None, C.sizeof(d), None, 0), "out is NULL"),
                       ((None, None, 0, None, 0), "names is NULL"),
                       ((None, None, 0, C.create_string_buffer(4), 4), "names_cap")):
        with pytest.raises(hal.R0HipError, match=word):
            hal.check(L.r0hip_circuit_info(*args))


def test_unknown_circuit_lists_the_compiled_in_names():
    from risc0_amd import hal
    z = np.zeros(64, np.uint32)
    want = r"unknown circuit keccak \(compiled in: rv32im, recursion, demo"
    with pytest.raises(hal.R0HipError, match=want):
        hal.circuit_info("keccak")
    with pytest.raises(hal.R0HipError, match=want):
        hal.poly_ext("keccak", z, z, z, z)
    with pytest.raises(hal.R0HipError, match=want):
        hal.constraint_term("keccak", z, z, z, z)
    with pytest.raises(hal.R0HipError, match=want):
        hal.verify_seal("keccak", 0, z)
    with pytest.raises(hal.R0HipError, match=want):
        hal.verify_seal("keccak", 0, z, check_validity=False)


def test_new_structs_match_the_c_header():
    from risc0_amd import hal
    mirrors = {"r0hip_circuit_desc": hal.CircuitDesc, "r0hip_selftest_suite": hal.SelftestSuite,
               "r0hip_selftest_report": hal.SelftestReport}
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
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln}
    for cname, py in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(py), cname
        for f in py._fields_:
            assert got[(cname, f[0])] == getattr(py, f[0]).offset, (cname, f[0])


def test_selftest_and_callback_refusals_need_no_device():
    from risc0_amd import hal
    L = hal.lib()
    rep = hal.SelftestReport()
    for args, word in (((0, 10, C.byref(rep), C.sizeof(rep)), "suites_mask 0"),
                       ((8, 10, C.byref(rep), C.sizeof(rep)), "suites_mask 8"),
                       ((7, 10, C.byref(rep), C.sizeof(rep) - 8), "out_size"),
                       ((7, 10, None, C.sizeof(rep)), "out is NULL"),
                       ((7, 7, C.byref(rep), C.sizeof(rep)), "po2 7"),
                       ((7, 25, C.byref(rep), C.sizeof(rep)), "po2 25")):
        with pytest.raises(hal.R0HipError, match=word):
            hal.check(L.r0hip_selftest(*args))
    with pytest.raises(hal.R0HipError, match="suites_mask 0"):
        hal.selftest(0)
    with pytest.raises(hal.R0HipError, match="out_size"):
        hal.selftest(7, out_size=8)
    with pytest.raises(hal.R0HipError, match="unknown circuit keccak"):
        hal.check(L.r0hip_prove_segment_cb(b"keccak", 0, 8, None, None, None, None, None, 0, 0, None, 0, None, None))
    with pytest.raises(hal.R0HipError, match="accum is NULL"):
        hal.check(L.r0hip_prove_segment_cb(b"demo", 0, 8, None, None, None, None, None, 0, 0, None, 0, None, None))


# ---- host evaluation against the AIR ----

def _ints(rng, n):
    return [int(x) for x in rng.integers(0, P, n)]


def _poly_ext(t, g, m, x):
    from risc0_amd import hal
    return tuple(int(v) for v in D.dec(hal.poly_ext("demo", D.enc(m), D.enc(g), D.enc(np.array(t).reshape(-1)),
                                                     D.enc(x))))


def test_poly_ext_equals_the_air_at_random_points():
    rng = np.random.default_rng(0xD3)
    for _ in range(20):
        t = [tuple(_ints(rng, 4)) for _ in range(16)]
        g, m, x = _ints(rng, 3), _ints(rng, 4), tuple(_ints(rng, 4))
        assert _poly_ext(t, g, m, x) == D.poly(t, g, m, x)


def test_poly_ext_equals_the_air_at_worst_case_values():
    """0, 1 and p - 1 in every position: every operand everywhere, then each tap, global, mix word
    and the poly_mix in turn against the others at p - 1 (every product of the AIR sees each of the
    three in either position)."""
    vals = (0, 1, P - 1)
    cases = []
    for v in vals:
        cases.append(([(v,) * 4] * 16, [v] * 3, [v] * 4, (v,) * 4))
    hi = P - 1
    for v in vals:
        for i in range(16):
            t = [(hi,) * 4] * 16
            t[i] = (v,) * 4
            cases.append((t, [hi] * 3, [hi] * 4, (hi,) * 4))
        for i in range(3):
            cases.append(([(hi,) * 4] * 16, [v if j == i else hi for j in range(3)], [hi] * 4, (hi,) * 4))
        for i in range(4):
            cases.append(([(hi,) * 4] * 16, [hi] * 3, [v if j == i else hi for j in range(4)], (hi,) * 4))
            cases.append(([(hi,) * 4] * 16, [hi] * 3, [hi] * 4, tuple(v if j == i else hi for j in range(4))))
    for t, g, m, x in cases:
        assert _poly_ext(t, g, m, x) == D.poly(t, g, m, x), (t, g, m, x)


def test_ir_eval_of_the_demo_program_equals_the_air():
    po2, n = 4, 13
    rows = 1 << po2
    rng = np.random.default_rng(0xD4)
    prog = ir_eval.load_ir("demo")
    x = tuple(_ints(rng, 4))
    pm = [D.epow(x, p) for p in D.POWERS]
    for groups in ("random", "all p - 1", "witness"):
        if groups == "witness":
            m = _ints(rng, 4)
            code, data, glob = D.witness(po2, n, 3, 5, noise=rng)
            acc = D.accumulate(po2, n, data, m)
        else:
            draw = (lambda k: rng.integers(0, P, k).astype(np.uint64)) if groups == "random" else \
                (lambda k: np.full(k, P - 1, np.uint64))
            code, data, acc, glob, m = draw(3 * rows), draw(3 * rows), draw(4 * rows), draw(3), [int(v) for v in draw(4)]
        args = [code, glob, data, np.array(m, np.uint64), acc]  # demo.taps.json eval_args
        got = ir_eval.evaluate(prog, args, rows, pm, inv_rate=1)
        want = D.poly(D.taps_on_rows(code, data, acc, rows), [int(v) for v in glob], m, x)
        for k in range(4):
            assert np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)), (groups, k)
        if groups == "witness":
            assert not any(np.asarray(want[k]).any() for k in range(4)), "the witness violates its own AIR"
        else:
            assert any(np.asarray(want[k]).any() for k in range(4))


def _term_ids():
    """ids of the 14 constraints in chain order: the `a` records of demo.poly.ir in file order (the
    generator writes each guarded block's inner chain before the block's `b` record)"""
    prog = ir_eval.load_ir("demo")
    ids = [ins[1] for ins in prog if ins[0] == "a"]
    assert len(ids) == 14 and sum(1 for ins in prog if ins[0] == "b") == 2
    return ids


def test_constraint_term_names_the_innermost_violated_record():
    from risc0_amd import hal
    po2, n = 4, 13
    rows = 1 << po2
    rng = np.random.default_rng(0xD5)
    m, x = _ints(rng, 4), tuple(_ints(rng, 4))
    code, data, glob = D.witness(po2, n, 3, 5, noise=rng)
    acc = D.accumulate(po2, n, data, m)
    ids = _term_ids()

    def term(code, data, acc, row):
        taps = [int(c[row]) for c in D.taps_on_rows(code, data, acc, rows)]
        got = hal.constraint_term("demo", D.enc(taps), D.enc(m), D.enc(glob), D.enc(x))
        cs = D.constraints(taps, [int(v) for v in glob], m)
        bad = [j for j, c in enumerate(cs) if any(c)]
        return got, (ids[bad[0]] if bad else None)

    for row in range(rows):  # active, padding and noise rows all satisfy the constraints
        assert term(code, data, acc, row) == (None, None), row
    # (group, column, row changed, row looked at) -> the constraint index that must be named
    cases = [("data", 2, 5, 5, 0),    # s: the product, outside any block
             ("data", 0, 0, 0, 0),    # a on the first row: the product first
             ("data", 1, 0, 1, 7),    # b[0] seen from row 1: a = b', inside the second block
             ("accum", 2, 0, 0, 5),   # z2 on the first row: inside the first block
             ("accum", 1, 6, 6, 10),  # z1 in the middle: inside the second block
             ("accum", 3, 6, 7, 12),  # z3 seen from the next row
             ("data", 0, 4, 5, 8),    # a[4] seen from row 5: b = a' + b'
             ("code", 2, 4, 4, 13)]   # `last` raised on a row whose b is not g2
    for grp, col, at, look, want in cases:
        g = {"code": code.copy(), "data": data.copy(), "accum": acc.copy()}
        g[grp][col * rows + at] = (g[grp][col * rows + at] + 1) % P
        got, expect = term(g["code"], g["data"], g["accum"], look)
        assert got == expect == ids[want], (grp, col, at, look, got, expect, ids[want])
    # a row of worst-case words names the first constraint
    taps = [P - 1] * 16
    assert hal.constraint_term("demo", D.enc(taps), D.enc([P - 1] * 4), D.enc([P - 1] * 3), D.enc((P - 1,) * 4)) == ids[0]


# ---- the committed seal ----

def test_golden_demo_seal_verifies_and_a_flipped_word_does_not():
    from risc0_amd import hal
    with open(os.path.join(GOLD, "index.json")) as f:
        idx = json.load(f)
    assert idx["seals"], "no demo seal recorded"
    for e in idx["seals"]:
        seal = np.load(os.path.join(GOLD, e["file"]))
        assert seal.dtype == np.uint32 and seal.nbytes < 256 << 10
        assert hal.verify_seal("demo", e["suite"], seal) == e["po2"]
        for at in (0, seal.size // 2, seal.size - 1):
            bad = seal.copy()
            bad[at] ^= 1
            with pytest.raises(hal.R0HipError):
                hal.verify_seal("demo", e["suite"], bad)
