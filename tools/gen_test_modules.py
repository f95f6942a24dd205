#!/usr/bin/env python3
"""The circuit files of the modules the tests load (tests/test_circuit_module_*.py), made at
build time from what is committed, one directory per module under the directory given:

  mod_demo        risc0_amd/circuits/demo.* under another name
  mod_recursion   risc0_amd/circuits/recursion.* under another name, its tuning file included
  mod_variant     the demo with the step (a, b) -> (b, a + 2b), which no build compiles in
                  (tests/circuit_rt_util.py write_variant)

A module's name must differ from every compiled-in circuit's, so each taps.json gets the new
name; the programs are copied as they are. A file is rewritten only when its content changes, so
`make` rebuilds a module only when its circuit did.

  gen_test_modules.py OUTDIR            all three
  gen_test_modules.py OUTDIR rv32im     mod_<circuit> of one committed circuit (the benchmark's)
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CIRCUITS = os.path.join(ROOT, "risc0_amd", "circuits")


def put(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if os.path.exists(path):
        with open(path) as f:
            if f.read() == text:
                return
    with open(path, "w") as f:
        f.write(text)


def renamed(outdir, new, src_dir, old):
    """<outdir>/<new>/<new>.*: the files of circuit `old` in src_dir under the name `new`"""
    with open(os.path.join(src_dir, old + ".taps.json")) as f:
        d = json.load(f)
    d["name"] = new
    put(os.path.join(outdir, new, new + ".taps.json"), json.dumps(d))
    for suffix in ("poly.ir", "ectune.json"):
        src = os.path.join(src_dir, f"{old}.{suffix}")
        if os.path.exists(src):
            with open(src) as f:
                put(os.path.join(outdir, new, f"{new}.{suffix}"), f.read())


def main():
    outdir = os.path.abspath(sys.argv[1])
    if len(sys.argv) > 2:
        for c in sys.argv[2:]:
            renamed(outdir, "mod_" + c, CIRCUITS, c)
        return
    renamed(outdir, "mod_demo", CIRCUITS, "demo")
    renamed(outdir, "mod_recursion", CIRCUITS, "recursion")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuit_rt_util as U
    with tempfile.TemporaryDirectory() as tmp:
        U.write_variant(tmp)
        renamed(outdir, "mod_variant", tmp, U.VARIANT)


if __name__ == "__main__":
    main()
