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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recursion_input_ab.json"))
    args = ap.parse_args()
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


def main():
    args = parse()
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
