"""Circuit modules (r0hip_circuit_load, include/r0hip_module.h), the part that needs no GPU:
  * the modules of the default build load, r0hip_circuit_backend tells compiled in (0), registered
    (1) and module (2) apart, the descriptor of mod_demo is the demo's;
  * a module exports its entry function and nothing else, and needs no symbol of libr0hip.so;
  * the host poly_ext under mod_recursion on the committed recursion fixture;
  * one refusal per rule of the load path, each naming the path and what disagrees and leaving
    the name list as it was; the malformed modules are stubs: plain C++ with no kernels, compiled
    here with g++ -shared;
  * the 64-entry limit and eight threads loading one file at once, in a process of their own (the
    registry has no way out);
  * the load path's host logic (descriptor checks, table validation, kernel-view checks) as a
    stand-alone program under AddressSanitizer and UBSan (tests/circuit_module_check.cpp)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import circuit_module_util as M
import circuit_rt_util as U

ROOT = U.ROOT
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- loading and telling the kinds apart ----

def test_load_backend_and_descriptor():
    from risc0_amd import hal
    assert M.loaded("mod_demo") == "mod_demo"
    rt = U.registered("demo")
    assert [hal.circuit_backend(n) for n in ("demo", rt, "mod_demo")] == [0, 1, 2]
    assert [hal.circuit_backend(n) for n in ("rv32im", "recursion")] == [0, 0]
    got, want = hal.circuit_info("mod_demo"), hal.circuit_info("demo")
    assert got.pop("name") == "mod_demo" and want.pop("name") == "demo"
    assert got == want
    names = hal.circuit_names()
    assert names[:3] == ["rv32im", "recursion", "demo"] and "mod_demo" in names[3:]
    # loaded names stand among the registered ones, in arrival order, under the word "registered"
    want = r"unknown circuit keccak \(compiled in: rv32im, recursion, demo; registered: " + ", ".join(names[3:]) + r"\)$"
    with pytest.raises(hal.R0HipError, match=r"r0hip_circuit_backend: " + want):
        hal.circuit_backend("keccak")
    with pytest.raises(hal.R0HipError, match=want):
        hal.circuit_info("keccak")
    for n in ("mod_recursion", "mod_variant"):
        assert M.loaded(n) == n and hal.circuit_backend(n) == 2
    got, want = hal.circuit_info("mod_recursion"), hal.circuit_info("recursion")
    got.pop("name"), want.pop("name")
    assert got == want
    with pytest.raises(hal.R0HipError, match="r0hip_circuit_backend: kind is NULL"):
        hal.check(hal.lib().r0hip_circuit_backend(b"demo", None))


@pytest.mark.parametrize("name", sorted(M.MODULES))
def test_a_module_exports_one_symbol_and_needs_none_of_the_library(name):
    path = M.module_path(name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    assert [ln.split()[-1] for ln in out.splitlines() if ln.strip()] == ["r0hip_circuit_module"]
    undefined = subprocess.check_output(["nm", "-D", "-u", path]).decode()
    assert "r0hip" not in undefined and "_ZN2r0" not in undefined, undefined
    needed = subprocess.check_output(["readelf", "-d", path]).decode()
    assert "libr0hip" not in needed and "libamdhip64" in needed
    data = open(path, "rb").read()
    assert set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", data)) == {b"gfx950"}


def test_poly_ext_under_the_loaded_name_equals_the_recursion_fixture():
    import oracle as O  # the input generator only: nothing is built
    import poly_ext_def as X
    from risc0_amd import hal
    mod = M.loaded("mod_recursion")
    want = np.load(os.path.join(GOLD, "poly_ext_recursion.npy"))
    info = hal.circuit_info(mod)
    pm, u, g, m = X.inputs(O, want.shape[0], info["n_taps"], info["mix_size"], info["output_size"])
    for k in range(0, want.shape[0], 20):
        a = hal.poly_ext("recursion", m[k], g[k], u[k], pm[k])
        b = hal.poly_ext(mod, m[k], g[k], u[k], pm[k])
        assert np.array_equal(a, want[k]) and np.array_equal(b, want[k]), k


def test_committed_demo_seal_verifies_under_the_loaded_name():
    from risc0_amd import hal
    mod = M.loaded("mod_demo")
    seal = np.load(os.path.join(GOLD, "demo", "seal_demo_poseidon2_po2_8.npy"))
    assert hal.verify_seal(mod, 0, seal) == 8
    bad = seal.copy()
    bad[bad.size // 2] ^= 1
    with pytest.raises(hal.R0HipError):
        hal.verify_seal(mod, 0, bad)
    with pytest.raises(hal.R0HipError):
        hal.verify_seal(M.loaded("mod_variant"), 0, seal)  # another circuit's seal


# ---- the build: a module's name becomes a directory the build clears ----

@pytest.mark.parametrize("name", ["", "..", "../x", "a/b", "2fast", "x" * 32])
def test_make_module_refuses_a_name_that_is_no_identifier(name, tmp_path):
    """refused before anything is generated or removed, through `make module` and when
    Makefile.module is entered directly"""
    args = [f"NAME={name}", f"DIR={tmp_path}", f"OUT={tmp_path}/x.r0mod.so"]
    for cmd in (["make", "-C", M.CSRC, "module"] + args,
                ["make", "-C", M.CSRC, "-f", "Makefile.module", "generate", f"ROOT={ROOT}"] + args):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0, cmd
        assert "is not a C identifier of at most 31 characters" in out.stderr or "usage: make module" in out.stderr, out.stderr
    assert os.listdir(tmp_path) == []


# ---- refusals ----

def _refused(path, want):
    """the load of `path` is refused with the path and `want` in the message, and the name list
    stays as it was"""
    from risc0_amd import hal
    before = hal.circuit_names()
    with pytest.raises(hal.R0HipError, match=r"^r0hip: r0hip_circuit_load: " + re.escape(str(path)) + ": " + want):
        hal.load_circuit_module(str(path))
    assert hal.circuit_names() == before


def test_a_missing_file_and_a_file_that_is_no_shared_object(tmp_path):
    _refused(tmp_path / "nowhere.r0mod.so", r".*cannot open shared object file")
    text = tmp_path / "text.r0mod.so"
    text.write_text("not a shared object, only as long as an ELF header would be: " + "x" * 64 + "\n")
    _refused(text, r".*(invalid ELF header|file too short)")


def test_a_name_that_is_taken(tmp_path):
    M.loaded("mod_demo")
    _refused(M.module_path("mod_demo"), "name: mod_demo is taken")  # the same file twice
    t = U.tables("demo")
    for taken in ("demo", U.registered("demo")):  # compiled in, registered
        _refused(M.build_stub(tmp_path, "taken_" + taken, M.stub_source(t, taken)), f"name: {taken} is taken")


def _swapped_taps(t):
    t = dict(t, taps=list(t["taps"]))
    t["taps"][0:5], t["taps"][5:10] = t["taps"][5:10], t["taps"][0:5]
    return t


# the demo's eval_args are code, global, data, mix, accum: argument 0 is code, of 3 columns
STUBS = [
    ("no_entry_symbol", dict(entry="some_other_function"), None, r"no entry symbol r0hip_circuit_module$"),
    ("abi", dict(abi="R0HIP_MODULE_ABI + 1"), None, r"abi: the module has 2 for R0HIP_MODULE_ABI, the library 1$"),
    ("struct_size", dict(args_size="sizeof(EvalCheckArgs) + 8"), None,
     r"args_size: the module has (\d+) for sizeof\(EvalCheckArgs\), the library (\d+)$"),
    ("architecture", dict(arch="gfx942"), None, r"arch: the module was compiled for gfx942, the library for gfx950$"),
    ("taps_out_of_order", {}, _swapped_taps, r"taps: entry 1 is not sorted"),
    ("col_idx_outside_its_group", dict(col=(0, 3)), None, r"info\(\): col_idx: column 0 is column 3 of code, which has 3$"),
    ("nargs", dict(nargs=4), None, r"info\(\): nargs: the kernels take 4 arguments, eval_args has 5$"),
]


@pytest.mark.parametrize("case", STUBS, ids=[c[0] for c in STUBS])
def test_a_malformed_module_is_refused_with_what_disagrees(case, tmp_path):
    cid, kw, edit, want = case
    t = U.tables("demo")
    assert t["eval_args"] == [1, -2, 2, -1, 0] and t["group_sizes"] == [4, 3, 3]
    if edit:
        t = edit(t)
    _refused(M.build_stub(tmp_path, cid, M.stub_source(t, "refused", **kw)), want)
    if cid == "struct_size":
        from risc0_amd import hal
        with pytest.raises(hal.R0HipError) as e:
            hal.load_circuit_module(os.path.join(str(tmp_path), cid + ".r0mod.so"))
        a, b = (int(x) for x in re.search(want, str(e.value)).groups())
        assert a == b + 8  # both values are printed


def test_a_sound_stub_loads_and_a_short_name_buffer_is_refused_first(tmp_path):
    """the control of the refusals above: the same stub with nothing changed is accepted (its
    empty kernels are never launched: the name is used on the host only)"""
    import ctypes as C
    from risc0_amd import hal
    path = M.build_stub(tmp_path, "stub_ok", M.stub_source(U.tables("demo"), "stub_ok"))
    before = hal.circuit_names()
    buf = C.create_string_buffer(16)
    with pytest.raises(hal.R0HipError, match="r0hip_circuit_load: name_cap 16 is below 32"):
        hal.check(hal.lib().r0hip_circuit_load(path.encode(), buf, 16))
    with pytest.raises(hal.R0HipError, match="r0hip_circuit_load: path is NULL"):
        hal.check(hal.lib().r0hip_circuit_load(None, None, 0))
    assert hal.circuit_names() == before
    if "stub_ok" not in before:  # (a second run in one process finds it loaded)
        hal.check(hal.lib().r0hip_circuit_load(path.encode(), None, 0))  # the name is optional
        assert hal.circuit_names() == before + ["stub_ok"]
    assert hal.circuit_backend("stub_ok") == 2
    seal = np.load(os.path.join(GOLD, "demo", "seal_demo_poseidon2_po2_8.npy"))
    assert hal.verify_seal("stub_ok", 0, seal) == 8  # its tables and ir serve the host verifier


_FRESH = r"""
import sys, threading
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import circuit_rt_util as U
import circuit_module_util as M
from risc0_amd import hal
# eight threads load one file at once: one wins, seven find the name taken
res = []
def load():
    try:
        res.append(hal.load_circuit_module(M.module_path("mod_variant")))
    except hal.R0HipError as e:
        res.append(str(e))
th = [threading.Thread(target=load) for _ in range(8)]
[x.start() for x in th]; [x.join() for x in th]
assert sorted(res)[0] == "mod_variant" and all(r.endswith("name: mod_variant is taken") for r in sorted(res)[1:]), res
assert hal.circuit_names()[3:] == ["mod_variant"]
# the registry's 64 entries are shared with registration
t = U.tables("demo")
for i in range(62):
    U.register_tables(t, f"c{i}")
assert hal.load_circuit_module(M.module_path("mod_demo")) == "mod_demo"
names = hal.circuit_names()
assert len(names) == 3 + 64 and names[-1] == "mod_demo"
try:
    hal.load_circuit_module(M.module_path("mod_recursion"))
    raise SystemExit("the 65th entry was accepted")
except hal.R0HipError as e:
    assert str(e) == "r0hip: r0hip_circuit_load: " + M.module_path("mod_recursion") + ": the registry is full (64 circuits)", str(e)
assert hal.circuit_names() == names
assert [hal.circuit_backend(n) for n in ("mod_variant", "c0", "mod_demo")] == [2, 1, 2]
print("ok")
"""


def test_concurrent_loads_and_the_limit_in_a_fresh_process():
    out = subprocess.run([sys.executable, "-c", _FRESH, ROOT], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- the load path's host logic under a sanitizer, as a program of its own ----

def test_load_checks_under_sanitizers(tmp_path):
    from test_circuit_rt_host import _write_tables
    exe = str(tmp_path / "circuit_module_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-Wall", "-Wextra", "-I", M.CSRC, os.path.join(ROOT, "tests", "circuit_module_check.cpp"),
                         os.path.join(M.CSRC, "circuit_module.cpp"), os.path.join(M.CSRC, "circuit_rt.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    path = str(tmp_path / "demo.tables")
    _write_tables(path, U.tables("demo"))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    lines = dict(ln.split(": ", 1) for ln in out.stdout.splitlines())
    assert lines["good"] == "ok" and lines["no_columns_no_combos"] == "ok"
    assert len(lines) >= 25 and sum(v == "ok" for v in lines.values()) == 2
    assert lines["taps_unsorted"].startswith("taps: entry 1 is not sorted")  # registration's words
    assert lines["col_idx"] == "info(): col_idx: column 0 is column 3 of data, which has 3"
