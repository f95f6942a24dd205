#!/usr/bin/env python3
"""One proof at a time: r0hip_set_proof_streams(2) and (3) against the single-stream default.

Needs an MI355X. A caller that proves one task at a time (an r0vm GPU worker) sees one proof's
latency, and alone a proof leaves parts of the chip idle; with n >= 2 the code group's commitment
runs on a side stream, beside the witness generation (r0hip_prove_recursion) or the data group's
commitment. This measures what that gives, in ONE process, on:

  trace      one po2=20 segment of the bench's loop.s session (bench.session_jobs) through the
             fused r0hip_prove_segment_trace
  per_op     the same segment through the native per-op driver (integration/hal_prover.cpp), whose
             calls are single ops: the setting changes nothing there, the leg shows the noise
  rec_sha    a recursion program filling --rec-po2 (18) through r0hip_prove_recursion, SHA-256
  rec_p2     the same with Poseidon2

Each workload runs at n = 1, 2 and 3. After --warmups untimed rounds of every leg, the timed
repeats alternate the legs of a workload, so drift of the machine falls on all alike; a repeat
is one proof between two r0hip_synchronize calls on the host clock. Reported per leg: every
repeat, median, min and max, and the eval_check phase of the proof (the prover's stream events,
or the driver's host phase). Per workload: the n = 1 leg's spread (max - min), each n's median
minus the n = 1 median, and whether that gain is larger than the spread (the rule by which the
overlap is kept). n = 1 is the launch sequence of the library before the mode existed. All seals
of a workload must be equal. One JSON file (default profiles/proof_streams_ab.json) and the same
line on stdout.

    python3 tools/bench_proof_streams.py [--po2 20] [--rec-po2 18] [--repeats 7] [--warmups 2]
                                         [--only trace,per_op,rec_sha,rec_p2] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "integration"))
WORKLOADS = ("trace", "per_op", "rec_sha", "rec_p2")
STREAMS = (1, 2, 3)


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rec-po2", type=int, default=18)
    ap.add_argument("--segments", type=int, default=2, help="segments of the session the first is taken from")
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats of each leg (at least 5)")
    ap.add_argument("--warmups", type=int, default=2, help="untimed rounds of each leg before the timed ones")
    ap.add_argument("--only", default=",".join(WORKLOADS), help="comma-separated workloads")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proof_streams_ab.json"))
    args = ap.parse_args()
    args.only = [w for w in args.only.split(",") if w]
    if args.repeats < 5 or any(w not in WORKLOADS for w in args.only):
        ap.error("--repeats must be at least 5, --only a list of " + ", ".join(WORKLOADS))
    return args


def leg_summary(ms, ec):
    return {"ms": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3), "eval_check_ms": round(statistics.median(ec), 3) if ec else None}


def measure(args, np, r, hal, prove, ec_phase):
    """the legs n = 1, 2, 3 of one workload: prove() returns the seal, ec_phase() the last proof's
    eval_check phase in ms"""
    ms, ec, seals = ({n: [] for n in STREAMS} for _ in range(3))
    for _ in range(args.warmups):
        for n in STREAMS:
            r.set_proof_streams(n)
            prove()
    for _ in range(args.repeats):
        for n in STREAMS:
            r.set_proof_streams(n)
            hal.synchronize()
            t = time.perf_counter()
            seal = prove()
            hal.synchronize()
            ms[n].append(1000.0 * (time.perf_counter() - t))
            ec[n].append(ec_phase())
            seals[n].append(seal)
    r.set_proof_streams(1)
    print("  ".join(f"n={n}: {[round(x, 2) for x in ms[n]]}" for n in STREAMS) + " ms", file=sys.stderr, flush=True)
    out = {f"n{n}": leg_summary(ms[n], ec[n]) for n in STREAMS}
    base = out["n1"]
    out["n1_spread_ms"] = round(base["max"] - base["min"], 3)
    for n in STREAMS[1:]:
        gain = round(base["median"] - out[f"n{n}"]["median"], 3)
        out[f"n{n}_gain_ms"] = gain
        out[f"n{n}_gain_exceeds_n1_spread"] = bool(gain > out["n1_spread_ms"])
    out["seals_equal"] = bool(all(np.array_equal(s, seals[1][0]) for n in STREAMS for s in seals[n]))
    return out


def main():
    args = parse()
    import numpy as np
    import bench
    import halprover
    import risc0_amd as r

    hal = r.HipHal("poseidon2")
    result = {}
    if "trace" in args.only or "per_op" in args.only:
        t0 = time.perf_counter()
        jobs, tr0 = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments), [0])
        job = jobs[0]
        print(f"one po2={args.po2} session segment built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

        def fused():
            return r.prove_segment_trace(hal, args.po2, job.glob, job.index, job.offsets, job.values, job.cycles,
                                         job.txns, tr0.table_split_cycle, bigint=tr0.bigint_array(),
                                         bigint_records=tr0.bigint_records())[0]
        if "trace" in args.only:
            result["trace"] = measure(args, np, r, hal, fused, lambda: r.last_profile().get("eval_check", 0.0))
        if "per_op" in args.only:
            result["per_op"] = measure(args, np, r, hal, lambda: halprover.prove_trace(hal, args.po2, job)[0],
                                       lambda: halprover.last_profile().get("eval_check", 0.0))
        del jobs, job
    if "rec_sha" in args.only or "rec_p2" in args.only:
        import recursion_program as RP
        t0 = time.perf_counter()
        po2 = args.rec_po2
        prog, inp = RP.random_program(np.random.default_rng(0x5249534330), (1 << po2) - RP.ZK_CYCLES - 1)
        wom, cyc, iops = (np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
                          for a in RP.trace_arrays(RP.preflight(prog, inp)))
        ctrl_words = RP.ctrl_group(prog, po2)
        print(f"one po2={po2} recursion program built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for name, suite in (("rec_sha", "sha-256"), ("rec_p2", "poseidon2")):
            if name not in args.only:
                continue
            h = r.HipHal(suite)
            ctrl = h.copy_from_elem("ctrl", ctrl_words)
            result[name] = measure(args, np, r, h, lambda: r.prove_recursion(h, po2, ctrl, wom, cyc, iops, 0x5EED)[0],
                                   lambda: r.last_profile().get("eval_check", 0.0))
            ctrl.free()

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    out = {
        "what": "one proof at a time under r0hip_set_proof_streams(n), n = 1 (the single-stream launch sequence), 2 "
                "and 3: the code group's commitment on a side stream for n >= 2. Legs of a workload alternated "
                "in one process after warm-up rounds of each; ms = host clock around one proof between two "
                "r0hip_synchronize calls; eval_check_ms = median of the proof's eval_check phase",
        "device": buf.value.decode(), "po2": args.po2, "rec_po2": args.rec_po2, "repeats": args.repeats,
        "warmup_rounds": args.warmups, **result,
        "seals_equal": bool(all(w["seals_equal"] for w in result.values())),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not out["seals_equal"]:
        print("bench_proof_streams: the legs' seals differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
