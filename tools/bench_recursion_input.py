#!/usr/bin/env python3
"""Recursion proofs from a resident program and its input words (r0hip_prove_recursion_program_input,
worker kind 4) against the proofs from the preflight's arrays as they stand
(r0hip_prove_recursion_program, worker kind 3).

Needs an MI355X. ONE process. The program and input are those of
tests/recursion_program.satisfying_witness(seed, --po2): random_program with that seed, filling the
segment. The arrays of leg A come from r0hip_recursion_preflight, which tests/
test_recursion_preflight_host.py pins word for word to the Python restatement (the restatement takes
a minute at po2 18). Legs are alternated (A, B, A, ...) after --warmups untimed rounds of each,
--repeats timed rounds; a repeat is one proof between two r0hip_synchronize calls on the host clock.

  A  program        r0hip_prove_recursion_program with wom, cycles and iops prepared outside the
                    timed region: the parent's path, which leaves the preflight to the caller
  B  program_input  r0hip_prove_recursion_program_input: preflight on the host, planned witness
                    generation, the same proof; the handle's plan is made before the timed region
     preflight      B's preflight alone, as the call itself measured it (r0hip_recursion_last_preflight_ms)
     b_less_preflight  B minus its own preflight, per repeat: what planned witness generation and
                    the page-locked staging change against A
  worker_kind3 / worker_kind4   --jobs jobs at --inflight in flight through a worker made before the
                    timed region (a fresh one per repeat, so tickets and the ZK noise agree): submit
                    all, wait for all; ms per job. Kind 4 runs the preflight on the uploader thread.

The witness generator's kernels are timed in a separate, untimed pass per leg with
r0hip_set_kernel_timing (recursion_witgen_exec covers the run keys, the run sort and the host
round trip in A, only the exec launches in B). r0hip_last_profile starts after witness generation
and has no such phase.

DESIGN.md section 7 item 9's rule on b_less_preflight against A: planned witness generation is
kept when it is not slower than A by more than A's spread (max - min), and called faster only
when the median gain exceeds that spread. All seals of a round must be equal. One JSON file
(default profiles/recursion_input_ab.json) and the same line on stdout.

    python3 tools/bench_recursion_input.py [--po2 18] [--repeats 7] [--warmups 2] [--jobs 12] [--inflight 3]

--pool-ab: the worker's preflight pool (r0hip_worker_set_preflight_threads) instead of the legs above,
into profiles/worker_preflight_pool_ab.json. Per repeat, alternated: kind 3 (the floor: arrays prepared
outside) and kind 4 with n = 0, 1, 2 and 3 pool threads, --jobs jobs at --inflight in flight, ms per job,
with the worker's own counters (r0hip_worker_get_stats) per leg; then a mixed queue that alternates kind-4
jobs with the rv32im jobs of tests/rv32im_trace.ecall_trace(--ecall-po2, reps=--ecall-reps) that
tools/bench_backs.py uses, at n = 0 and at every n > 0. With --parent-lib PATH (a libr0hip.so built from
the parent commit, under the git-ignored risc0_amd/lib_variants/) the kind-4 leg is first run on that
library in a child process of the same session (R0HIP_LIB; one process holds one library), with the same
program, warm-ups and repeats; the n = 0 leg must lie within that leg's spread. Item 9's rule per pool
size: faster only when the median gain over the compared leg exceeds that leg's spread.

--p2-share: no GPU. Builds tools/micro/preflight_p2_share.cpp with g++ -O3 and runs it on the same
program: the preflight alone (rpf::run), the program's Poseidon2 permutations alone (poseidon2_mix on a
chained state, as many as the program has p2_partial rows), and r0hip_recursion_preflight from Python
for the same program; prints one JSON line (and writes --out if given).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 0x5249534330
KEY = bytes(range(32))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=18)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--jobs", type=int, default=12)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--suite", default="poseidon2")
    ap.add_argument("--wait-s", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pool-ab", action="store_true")
    ap.add_argument("--p2-share", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ecall-po2", type=int, default=16)
    ap.add_argument("--ecall-reps", type=int, default=30)
    ap.add_argument("--pool-child", default=None, help=argparse.SUPPRESS)  # the parent-library leg: an .npz
    args = ap.parse_args()
    if args.out is None and not args.p2_share:
        args.out = os.path.join(ROOT, "profiles",
                                "worker_preflight_pool_ab.json" if args.pool_ab else "recursion_input_ab.json")
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    return args


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3)}


def compare(out, base, leg):
    spread = round(out[base]["max"] - out[base]["min"], 3)
    gain = round(out[base]["median"] - out[leg]["median"], 3)
    return {"compared": base, "spread_ms": spread, "gain_ms": gain, "gain_exceeds_spread": bool(gain > spread),
            "slower_by_more_than_spread": bool(-gain > spread)}


def witgen_kernels(r, hal, fn):
    """GPU milliseconds of the witness generator's launchers over one call of fn"""
    fn()
    r.set_kernel_timing(True)
    try:
        fn()
        hal.synchronize()
        times = r.kernel_times()
    finally:
        r.set_kernel_timing(False)
    return {k: round(v[0], 3) for k, v in times.items() if k.startswith("recursion_witgen")}


def build_program(np, po2):
    import recursion_program as RP
    t0 = time.perf_counter()
    prog_rows, inp = RP.random_program(np.random.default_rng(SEED), (1 << po2) - RP.ZK_CYCLES - 1)
    code = np.ascontiguousarray(prog_rows.encoded(), dtype=np.uint32).reshape(-1)
    print(f"one po2={po2} program of {len(prog_rows.rows)} rows built in {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    return code, np.array(inp, dtype=np.uint32), len(prog_rows.rows)


def worker_run(r, hal, args, po2, n, submit, jobs):
    """one fresh worker with n pool threads: submit(w, i) for i < jobs, wait for all; returns ms per
    job, the seals by ticket and the worker's counters (None on a library without them)"""
    with r.Worker(hal, max_po2=po2, in_flight=args.inflight, verify=True, noise_key=KEY) as w:
        if n:
            w.set_preflight_threads(n)
        hal.synchronize()
        t = time.perf_counter()
        for i in range(jobs):
            submit(w, i)
        seals = {}
        for _ in range(jobs):
            res = w.wait(args.wait_s)
            if res is None:
                raise SystemExit("bench_recursion_input: a worker job did not come back")
            if res[3] is not None:
                raise SystemExit(f"bench_recursion_input: job {res[0]}: {res[3]}")
            seals[res[0]] = res[1]
        per_job = 1000.0 * (time.perf_counter() - t) / jobs
        st = None
        if hasattr(r.lib(), "r0hip_worker_get_stats"):
            s = w.stats()
            st = {"pool_jobs": int(s.pool_jobs), "inline_jobs": int(s.inline_jobs),
                  "peak_slots_in_use": int(s.peak_slots_in_use), "preflight_slots": int(s.preflight_slots),
                  "slot_bytes": int(s.slot_bytes), "pool_busy_ms": round(s.pool_busy_ms, 3),
                  "uploader_preflight_ms": round(s.uploader_preflight_ms, 3),
                  "uploader_wait_preflight_ms": round(s.uploader_wait_preflight_ms, 3)}
    return per_job, seals, st


def pool_child(args):
    """the kind-4 leg on whatever library R0HIP_LIB names (the parent's): one JSON line"""
    import numpy as np
    import risc0_amd as r
    z = np.load(args.pool_child)
    code, inp, po2 = z["code"], z["inp"], args.po2
    hal = r.HipHal(args.suite)
    prog = r.RecursionProgram.create(hal, po2, code)
    prog.prepare_input()
    ms = []
    for rep in range(args.warmups + args.repeats):
        m, _seals, _st = worker_run(r, hal, args, po2, 0, lambda w, i: w.submit_recursion_input(prog, inp), args.jobs)
        if rep >= args.warmups:
            ms.append(m)
    prog.close()
    print(json.dumps({"library": os.environ.get("R0HIP_LIB"), "has_pool": hasattr(r.lib(), "r0hip_worker_get_stats"),
                      **summary(ms)}))


def median_stats(stats):
    """the per-repeat counters of one leg as their medians"""
    return {k: round(statistics.median(s[k] for s in stats), 3) for k in stats[0]} if stats and stats[0] else None


def pool_ab(args):
    import subprocess
    import tempfile

    import numpy as np
    import risc0_amd as r
    import rv32im_trace as T

    po2 = args.po2
    code, inp, code_rows = build_program(np, po2)
    wom, cyc, iops, _output = r.recursion_preflight(code, po2, inp)
    out = {}
    if args.parent_lib:
        # before this process opens the GPU: one process, one library
        with tempfile.TemporaryDirectory() as d:
            npz = os.path.join(d, "program.npz")
            np.savez(npz, code=code, inp=inp)
            cmd = [sys.executable, os.path.abspath(__file__), "--pool-child", npz, "--po2", str(po2), "--repeats",
                   str(args.repeats), "--warmups", str(args.warmups), "--jobs", str(args.jobs), "--inflight",
                   str(args.inflight), "--suite", args.suite, "--wait-s", str(args.wait_s)]
            env = dict(os.environ, R0HIP_LIB=os.path.abspath(args.parent_lib))
            child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200)
            if child.returncode:
                raise SystemExit("bench_recursion_input: the parent-library leg failed:\n" + child.stderr[-3000:])
            out["parent_kind4"] = json.loads(child.stdout.strip().split("\n")[-1])
            if out["parent_kind4"].pop("has_pool"):
                raise SystemExit("bench_recursion_input: --parent-lib has the pool's entry points: not the parent")
        print(f"parent kind 4: {out['parent_kind4']['ms']} ms per job", file=sys.stderr, flush=True)

    hal = r.HipHal(args.suite)
    prog = r.RecursionProgram.create(hal, po2, code)
    prog.prepare_input()
    te = T.ecall_trace(args.ecall_po2, seed=3, bigint=True, reps=args.ecall_reps)
    tcyc, ttx = te.arrays()
    ecall = r.TraceJob(*(r.pinned_copy(a) for a in (te.global_words(), *te.injector_arrays(), tcyc, ttx)),
                       te.table_split_cycle, bigint=te.bigint_array(), bigint_records=te.bigint_records())
    sizes = [0, 1, 2, 3]

    def kind3(w, i):
        w.submit_recursion_program(prog, wom, cyc, iops)

    def kind4(w, i):
        w.submit_recursion_input(prog, inp)

    def mixed(w, i):
        if i % 2:
            w.submit_trace(ecall, args.ecall_po2)
        else:
            w.submit_recursion_input(prog, inp)

    max_po2 = max(po2, args.ecall_po2)
    legs = [("kind3", 0, kind3)] + [(f"kind4_n{n}", n, kind4) for n in sizes] + [(f"mixed_n{n}", n, mixed) for n in sizes]
    ms, stats = {name: [] for name, _, _ in legs}, {name: [] for name, _, _ in legs}
    equal = True
    for rep in range(args.warmups + args.repeats):
        seals = {}
        for name, n, submit in legs:
            m, seals[name], st = worker_run(r, hal, args, max_po2 if name.startswith("mixed") else po2, n, submit,
                                            args.jobs)
            if rep >= args.warmups:
                ms[name].append(m)
                stats[name].append(st)
        for n in sizes:  # a seal depends on the job and its ticket alone
            equal = equal and all(np.array_equal(seals["kind3"][k], seals[f"kind4_n{n}"][k]) for k in seals["kind3"])
            equal = equal and all(np.array_equal(seals["mixed_n0"][k], seals[f"mixed_n{n}"][k]) for k in seals["mixed_n0"])
    prog.close()
    for name, _, _ in legs:
        out[name] = summary(ms[name])
        if name != "kind3":
            out[name]["stats_median"] = median_stats(stats[name])
        print(f"{name}: {out[name]['ms']} ms per job", file=sys.stderr, flush=True)
    if args.parent_lib:
        out["n0_vs_parent"] = compare(out, "parent_kind4", "kind4_n0")
        out["n0_within_parent_spread"] = bool(abs(out["n0_vs_parent"]["gain_ms"]) <= out["n0_vs_parent"]["spread_ms"])
    for n in sizes[1:]:
        out[f"kind4_n{n}_vs_n0"] = compare(out, "kind4_n0", f"kind4_n{n}")
        out[f"mixed_n{n}_vs_n0"] = compare(out, "mixed_n0", f"mixed_n{n}")
        out[f"kind4_n{n}_vs_kind3"] = compare(out, "kind3", f"kind4_n{n}")
    best = min(sizes[1:], key=lambda n: out[f"mixed_n{n}"]["median"])
    out["mixed_best_n"] = best

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "the worker's kind-4 jobs (a resident program and its input words) with the preflight on the "
                "uploader thread (n0) and on a pool of n host threads (r0hip_worker_set_preflight_threads), kind 3 "
                "(arrays prepared outside) as the floor; mixed_*: kind-4 jobs alternating with rv32im ecall_trace "
                "jobs in one queue. ms per job = host clock from the first submit to the last wait / jobs, a fresh "
                "worker per run, made before the timed region. Legs alternated in one process after warm-up rounds; "
                "parent_kind4: the kind-4 leg on a library built from the parent commit, in a child process of the "
                "same session before the other legs. stats_median: r0hip_worker_get_stats after the last job, median "
                "over the repeats. Not measured: a real lift or join program, other suites, other in_flight, a "
                "loaded host",
        "device": buf.value.decode(), "suite": args.suite, "po2": po2, "repeats": args.repeats,
        "warmup_rounds": args.warmups, "worker_jobs": args.jobs, "worker_in_flight": args.inflight,
        "code_rows": code_rows, "input_words": int(inp.size), "ecall_po2": args.ecall_po2,
        "ecall_reps": args.ecall_reps, "host_cpus": len(os.sched_getaffinity(0)), **out, "seals_equal": bool(equal),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    if not equal:
        print("bench_recursion_input: the legs' seals differ", file=sys.stderr)
        sys.exit(1)


def p2_share(args):
    import platform
    import subprocess
    import tempfile

    import numpy as np
    import risc0_amd as r

    po2 = args.po2
    code, inp, code_rows = build_program(np, po2)
    py_ms = []
    for _ in range(args.warmups + args.repeats):
        t = time.perf_counter()
        r.recursion_preflight(code, po2, inp)
        py_ms.append(1000.0 * (time.perf_counter() - t))
    with tempfile.TemporaryDirectory() as d:
        exe, case = os.path.join(d, "preflight_p2_share"), os.path.join(d, "case.bin")
        csrc = os.path.join(ROOT, "risc0_amd", "csrc")
        subprocess.run(["g++", "-O3", "-std=c++17", "-I", csrc, "-o", exe,
                        os.path.join(ROOT, "tools", "micro", "preflight_p2_share.cpp"),
                        os.path.join(csrc, "recursion_preflight.cpp")], check=True)
        np.concatenate([np.array([po2, code.size, inp.size], np.uint32), code, inp]).tofile(case)
        native = json.loads(subprocess.run([exe, case, str(args.warmups), str(args.repeats)], capture_output=True,
                                           text=True, check=True).stdout)
    cpu = ""
    try:
        cpu = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")][0]
    except (OSError, IndexError):
        cpu = platform.processor()
    result = {"what": "the host preflight of one program and the share of its Poseidon2 permutations, one thread, "
                      "no GPU: preflight = rpf::run alone (decoded program), permutations = as many poseidon2_mix "
                      "calls on a chained 24-word state as the program has p2_partial rows, c_abi = "
                      "r0hip_recursion_preflight from Python (decode, run, the copies out)",
              "cpu": cpu, "po2": po2, "code_rows": code_rows, "repeats": args.repeats, "warmup_rounds": args.warmups,
              **native, "c_abi": summary(py_ms[args.warmups:])}
    result["p2_share_of_preflight"] = round(result["permutations"]["median"] / result["preflight"]["median"], 4)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


def main():
    args = parse()
    if args.pool_child:
        return pool_child(args)
    if args.pool_ab:
        return pool_ab(args)
    if args.p2_share:
        return p2_share(args)
    import numpy as np
    import recursion_program as RP
    import risc0_amd as r

    po2 = args.po2
    t0 = time.perf_counter()
    prog_rows, inp = RP.random_program(np.random.default_rng(SEED), (1 << po2) - RP.ZK_CYCLES - 1)
    code = prog_rows.encoded()
    inp = np.array(inp, dtype=np.uint32)
    wom, cyc, iops, output = r.recursion_preflight(code, po2, inp)
    print(f"one po2={po2} program of {len(prog_rows.rows)} rows built in {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)

    hal = r.HipHal(args.suite)
    prog = r.RecursionProgram.create(hal, po2, code)
    hal.synchronize()
    t = time.perf_counter()
    prog.prepare_input()
    prepare_ms = 1000.0 * (time.perf_counter() - t)
    info = prog.input_info()
    sid = [0]
    last_out = [None]

    def leg_a():
        return prog.prove(wom, cyc, iops, KEY, sid[0])[0]

    def leg_b():
        seal, _mix, out = prog.prove_input(inp, KEY, sid[0])
        last_out[0] = out
        return seal

    ms = {"program": [], "program_input": [], "preflight": [], "b_less_preflight": []}
    equal = True
    for _ in range(args.warmups):
        leg_a()
        leg_b()
    for rep in range(args.repeats):
        sid[0] = 1 + rep
        hal.synchronize()
        t = time.perf_counter()
        sa = leg_a()
        hal.synchronize()
        ms["program"].append(1000.0 * (time.perf_counter() - t))
        t = time.perf_counter()
        sb = leg_b()
        hal.synchronize()
        b = 1000.0 * (time.perf_counter() - t)
        pre = r.recursion_last_preflight_ms()
        ms["program_input"].append(b)
        ms["preflight"].append(pre)
        ms["b_less_preflight"].append(b - pre)
        equal = equal and bool(np.array_equal(sa, sb)) and bool(np.array_equal(last_out[0], output))
    print("  ".join(f"{leg}: {[round(x, 2) for x in v]}" for leg, v in ms.items()) + " ms", file=sys.stderr, flush=True)
    out = {leg: summary(v) for leg, v in ms.items()}
    out["planned_vs_program"] = compare(out, "program", "b_less_preflight")
    out["input_vs_program"] = compare(out, "program", "program_input")
    out["witgen_kernels_ms"] = {"program": witgen_kernels(r, hal, leg_a), "program_input": witgen_kernels(r, hal, leg_b)}

    def run(kind):
        with r.Worker(hal, max_po2=po2, in_flight=args.inflight, verify=True, noise_key=KEY) as w:
            hal.synchronize()
            t = time.perf_counter()
            for _ in range(args.jobs):
                if kind == 3:
                    w.submit_recursion_program(prog, wom, cyc, iops)
                else:
                    w.submit_recursion_input(prog, inp)
            seals = {}
            for _ in range(args.jobs):
                res = w.wait(args.wait_s)
                if res is None:
                    raise SystemExit("bench_recursion_input: a worker job did not come back")
                if res[3] is not None:
                    raise SystemExit(f"bench_recursion_input: job {res[0]}: {res[3]}")
                seals[res[0]] = res[1]
            per_job = 1000.0 * (time.perf_counter() - t) / args.jobs
        return per_job, seals

    wms = {3: [], 4: []}
    for _ in range(args.warmups):
        run(3)
        run(4)
    for _ in range(args.repeats):
        m3, s3 = run(3)
        m4, s4 = run(4)
        wms[3].append(m3)
        wms[4].append(m4)
        equal = equal and all(np.array_equal(s3[k], s4[k]) for k in s3)
    print(f"worker kind 3: {[round(x, 2) for x in wms[3]]}  kind 4: {[round(x, 2) for x in wms[4]]} ms per job",
          file=sys.stderr, flush=True)
    out["worker_kind3"], out["worker_kind4"] = summary(wms[3]), summary(wms[4])
    out["worker_kind4_vs_kind3"] = compare(out, "worker_kind3", "worker_kind4")
    prog.close()

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "recursion proofs of one program filling a po2 segment from a resident handle: "
                "r0hip_prove_recursion_program with the preflight's arrays prepared outside the timed region "
                "(program), r0hip_prove_recursion_program_input with the native preflight inside it (program_input), "
                "that call's own preflight (preflight) and the difference per repeat (b_less_preflight); the worker at "
                "in_flight with kind-3 jobs (arrays) and kind-4 jobs (input words, preflight on the uploader thread), "
                "ms per job. Legs alternated in one process after warm-up rounds; ms = host clock between two "
                "r0hip_synchronize calls. witgen_kernels_ms: GPU time of the witness generator's launchers in an "
                "untimed pass. Not measured: a real lift or join program, other suites, a caller's own preflight",
        "device": buf.value.decode(), "suite": args.suite, "po2": po2, "repeats": args.repeats,
        "warmup_rounds": args.warmups, "worker_jobs": args.jobs, "worker_in_flight": args.inflight,
        "code_rows": len(prog_rows.rows), "input_words": int(inp.size), "wom_bytes": int(wom.nbytes),
        "n_runs": int(info.n_runs), "bucket_runs": [int(x) for x in info.bucket_runs],
        "plan_device_bytes": int(info.plan_device_bytes), "plan_host_bytes": int(info.plan_host_bytes),
        "prepare_input_ms": round(prepare_ms, 3), **out, "seals_equal": bool(equal),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    if not equal:
        print("bench_recursion_input: the legs' seals or outputs differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
