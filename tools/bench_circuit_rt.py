#!/usr/bin/env python3
"""A/B of the generated eval_check / constraint-rows kernels against the interpreter that a
circuit registered at run time gets (risc0_amd/csrc/eval_interp.hip), on the same committed
program: `rv32im` against `rt_rv32im`, `recursion` against `rt_recursion`.

One process, the legs alternated, 2 warm-up rounds and 7 repeats, device time from
r0hip_set_kernel_timing (the KScope families eval_check, eval_check_interp, constraint_rows,
constraint_rows_interp); median and min-max per leg. The interpreter runs with its own chunk (the
library's slot-file budget, leg "interp") and, for comparison, with the chunks other budgets would
give (legs "interp_<MiB>MiB", set through r0hip_testing_set_interp_chunk).

  tools/bench_circuit_rt.py [--out profiles/circuit_rt_ab.json] [--cases rv32im:20:846,recursion:18:470]
                            [--budgets 32]

With --modules the second leg is a circuit module instead (r0hip_circuit_load): the same program's
generated kernels compiled into a shared object of their own (mod_rv32im, mod_recursion, built
from the committed files into --module-dir when they are not there yet; the seconds each build
took on this machine are kept beside the module and reported). The kernels are the same source
under the same tuning, so the module leg's median is expected inside the compiled leg's min-max.

  tools/bench_circuit_rt.py --modules [--out profiles/circuit_module_ab.json] [--build-only]

A case is circuit:po2:slot words per point (Fp slots + 4 x FpExt slots of the compiled program, as
tests/circuit_rt_check.cpp prints them), from which a budget's chunk follows.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
P = 15 * 2**27 + 1
WARMUP, REPEATS = 2, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None,
                    help="default profiles/circuit_rt_ab.json, with --modules profiles/circuit_module_ab.json")
    ap.add_argument("--cases", default="rv32im:20:846,recursion:18:470")
    ap.add_argument("--budgets", default="32", help="other slot-file budgets to compare, MiB")
    ap.add_argument("--modules", action="store_true", help="A/B the compiled-in kernels against circuit modules")
    ap.add_argument("--module-dir", default=os.path.join(ROOT, "risc0_amd", "modules", "bench"))
    ap.add_argument("--build-only", action="store_true", help="with --modules: build the modules and stop (no GPU)")
    ap.add_argument("--module-first", action="store_true",
                    help="with --modules: the module leg first in every round (a difference that follows the "
                         "position in the round is the order's, not the module's)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "circuit_module_ab.json" if a.modules else "circuit_rt_ab.json")
    if a.modules:
        return module_ab(a)
    budgets = [int(b) for b in a.budgets.split(",") if b]
    import risc0_amd as r
    from risc0_amd import hal as H
    hal = r.HipHal("poseidon2")
    circuits = os.path.join(ROOT, "risc0_amd", "circuits")
    result = {"warmup": WARMUP, "repeats": REPEATS, "cases": []}
    for case in a.cases.split(","):
        name, po2, slot_words = case.split(":")
        po2, slot_words = int(po2), int(slot_words)
        rt = "rt_" + name
        if rt not in H.circuit_names():
            H.register_circuit(rt, circuits, files=name)
        info = H.circuit_info(name)
        rng = np.random.default_rng(0xAB00 + po2)
        pm = rng.integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
        dmix = hal.copy_from_elem("mix", rng.integers(0, P, info["mix_size"], dtype=np.uint64).astype(np.uint32))
        dglob = hal.copy_from_elem("glob", rng.integers(0, P, info["output_size"], dtype=np.uint64).astype(np.uint32))
        for family, n in (("eval_check", 4 << po2), ("constraint_rows", 1 << po2)):
            groups = []
            for g in info["group_sizes"]:
                b = hal.alloc_elem("g", g * n)
                H.check(H.lib().r0hip_fill_uniform(b.ptr, g * n, int(rng.integers(1, 1 << 62))))
                groups.append(b)
            out = hal.alloc_elem("out", 4 * n)

            def run(circuit):
                if family == "eval_check":
                    hal.eval_check(circuit, out, groups, dmix, dglob, pm, po2)
                else:
                    H.constraint_rows(circuit, po2, groups[1], groups[2], groups[0], dmix, dglob, pm, out)

            def timed(circuit, key):
                before = H.kernel_times().get(key, (0.0, 0))
                run(circuit)
                after = H.kernel_times()[key]
                assert after[1] == before[1] + 1, (key, before, after)
                return after[0] - before[0]

            # the interpreter with its own chunk (0: the library's budget) and with other budgets'
            H.set_kernel_timing(True)
            legs = {"compiled": (name, family, 0), "interp": (rt, family + "_interp", 0)}
            for b in budgets:
                legs[f"interp_{b}MiB"] = (rt, family + "_interp", chunk_points(b, slot_words, n))
            ms = {k: [] for k in legs}
            for rnd in range(WARMUP + REPEATS):
                for k, (circuit, key, chunk) in legs.items():
                    was = H.testing_set_interp_chunk(chunk)
                    try:
                        t = timed(circuit, key)
                    finally:
                        H.testing_set_interp_chunk(was)
                    if rnd >= WARMUP:
                        ms[k].append(t)
            H.set_kernel_timing(False)
            entry = {"circuit": name, "po2": po2, "family": family, "points": n,
                     "chunk_points": {f"{b}MiB": chunk_points(b, slot_words, n) for b in budgets}}
            for k, v in ms.items():
                entry[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            entry["interp_over_compiled"] = entry["interp"]["median_ms"] / entry["compiled"]["median_ms"]
            print(json.dumps(entry), flush=True)
            result["cases"].append(entry)
            del groups, out
            H.trim()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def build_module(circuit, module_dir):
    """module_dir/mod_<circuit>.r0mod.so from the committed files, built if absent; (path, the
    seconds its build took and the jobs it ran with, as recorded when it was built)"""
    import subprocess
    import time
    from risc0_amd import hal as H
    name = "mod_" + circuit
    out = os.path.join(module_dir, name + ".r0mod.so")
    note = os.path.join(module_dir, name + ".build.json")
    if not os.path.exists(out):
        src = os.path.join(module_dir, "src")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_test_modules.py"), src, circuit])
        jobs = min(16, os.cpu_count() or 8)
        t0 = time.time()
        H.build_circuit_module(name, os.path.join(src, name), out, jobs=jobs)
        with open(note, "w") as f:
            json.dump({"build_s": round(time.time() - t0, 1), "jobs": jobs}, f)
    with open(note) as f:
        return out, json.load(f)


def module_ab(a):
    from risc0_amd import hal as H
    cases = [c.split(":")[:2] for c in a.cases.split(",")]
    built = {name: build_module(name, a.module_dir) for name, _ in cases}
    for name, (path, note) in built.items():
        print(json.dumps({"module": "mod_" + name, "bytes": os.path.getsize(path), **note}), flush=True)
    if a.build_only:
        return
    import risc0_amd as r
    hal = r.HipHal("poseidon2")
    result = {"warmup": WARMUP, "repeats": REPEATS, "cases": [],
              "modules": {"mod_" + n: dict(note, bytes=os.path.getsize(p)) for n, (p, note) in built.items()}}
    for name, po2 in cases:
        po2 = int(po2)
        mod = H.load_circuit_module(built[name][0])
        assert H.circuit_backend(mod) == 2 and H.circuit_backend(name) == 0
        info = H.circuit_info(name)
        rng = np.random.default_rng(0xAB00 + po2)
        pm = rng.integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
        dmix = hal.copy_from_elem("mix", rng.integers(0, P, info["mix_size"], dtype=np.uint64).astype(np.uint32))
        dglob = hal.copy_from_elem("glob", rng.integers(0, P, info["output_size"], dtype=np.uint64).astype(np.uint32))
        for family, n in (("eval_check", 4 << po2), ("constraint_rows", 1 << po2)):
            groups = []
            for g in info["group_sizes"]:
                b = hal.alloc_elem("g", g * n)
                H.check(H.lib().r0hip_fill_uniform(b.ptr, g * n, int(rng.integers(1, 1 << 62))))
                groups.append(b)
            out = hal.alloc_elem("out", 4 * n)

            def timed(circuit):
                before = H.kernel_times().get(family, (0.0, 0))
                if family == "eval_check":
                    hal.eval_check(circuit, out, groups, dmix, dglob, pm, po2)
                else:
                    H.constraint_rows(circuit, po2, groups[1], groups[2], groups[0], dmix, dglob, pm, out)
                after = H.kernel_times()[family]
                assert after[1] == before[1] + 1, (family, before, after)
                return after[0] - before[0]

            # the two legs must also agree word for word
            words = []
            for circuit in (name, mod):
                if family == "eval_check":
                    hal.eval_check(circuit, out, groups, dmix, dglob, pm, po2)
                else:
                    H.constraint_rows(circuit, po2, groups[1], groups[2], groups[0], dmix, dglob, pm, out)
                words.append(out.to_numpy())  # 4n words in both families
            assert np.array_equal(words[0], words[1]), (name, family, "the module's words differ")
            del words
            H.set_kernel_timing(True)
            legs = {"module": mod, "compiled": name} if a.module_first else {"compiled": name, "module": mod}
            ms = {k: [] for k in legs}
            for rnd in range(WARMUP + REPEATS):
                for k, circuit in legs.items():
                    t = timed(circuit)
                    if rnd >= WARMUP:
                        ms[k].append(t)
            H.set_kernel_timing(False)
            entry = {"circuit": name, "po2": po2, "family": family, "points": n, "order": list(legs)}
            for k, v in ms.items():
                entry[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            entry["module_over_compiled"] = entry["module"]["median_ms"] / entry["compiled"]["median_ms"]
            entry["module_median_inside_compiled_spread"] = \
                entry["compiled"]["min_ms"] <= entry["module"]["median_ms"] <= entry["compiled"]["max_ms"]
            print(json.dumps(entry), flush=True)
            result["cases"].append(entry)
            del groups, out
            H.trim()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def chunk_points(budget_mib, slot_words, n):
    """points per launch a slot file of budget_mib holds (a multiple of the workgroup, as the
    library sizes its own chunk from its budget)"""
    return max(256, min(n, (budget_mib << 20) // (4 * max(1, slot_words)) // 256 * 256))


if __name__ == "__main__":
    main()
