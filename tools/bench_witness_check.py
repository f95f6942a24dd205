#!/usr/bin/env python3
"""What r0hip_set_witness_check costs one proof, and that the mode off costs nothing.

Needs an MI355X. With the mode on, the provers evaluate the constraint polynomial on the 2^po2
trace rows before the accum commit (the rows family of tools/gen_eval_check.py, a quarter of
eval_check's points, then a one-pass report and a 19-word read-back). Measured in ONE process:

  trace   one po2=20 segment of the bench's loop.s session (bench.session_jobs) through the fused
          r0hip_prove_segment_trace, mode off and on
  rec     a recursion program filling --rec-po2 (18) through r0hip_prove_recursion (Poseidon2),
          mode off and on

After --warmups untimed rounds of both legs, the timed repeats alternate off and on, so drift of
the machine falls on both alike; a repeat is one proof between two r0hip_synchronize calls on the
host clock. Reported per leg: every repeat, median, min and max; for the on leg also the
check_witness phase of the proof (the prover's stream events). Per workload: the on leg's median
minus the off leg's, and whether the seals are equal (they must be).

  --parent-lib FILE   the library of the parent commit: the off leg of both workloads is also
          measured against the same calls on that library, by the rule of DESIGN.md §7 item 9 (the
          off path adds no launch, so it may not be slower than the parent by more than the parent
          leg's own spread, max - min). A library holds its own runtime state, so each side runs
          in a child process of its own (this script with --child), parent and new alternating
          twice, before this process opens the device; never two at once.

One JSON file (default profiles/witness_check_ab.json) and the same line on stdout.

    python3 tools/bench_witness_check.py [--po2 20] [--rec-po2 18] [--repeats 7] [--warmups 2]
                                         [--only trace,rec] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = ("trace", "rec")


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rec-po2", type=int, default=18)
    ap.add_argument("--segments", type=int, default=2, help="segments of the session the first is taken from")
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats of each leg (at least 5)")
    ap.add_argument("--warmups", type=int, default=2, help="untimed rounds of each leg before the timed ones")
    ap.add_argument("--only", default=",".join(WORKLOADS), help="comma-separated workloads")
    ap.add_argument("--parent-lib", default=None, help="libr0hip.so of the parent commit (leg c)")
    ap.add_argument("--child", action="store_true", help="(internal) off legs only, JSON on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_check_ab.json"))
    args = ap.parse_args()
    args.only = [w for w in args.only.split(",") if w]
    if args.repeats < 5 or any(w not in WORKLOADS for w in args.only):
        ap.error("--repeats must be at least 5, --only a list of " + ", ".join(WORKLOADS))
    return args


def summary(ms, phase=None):
    out = {"ms": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
           "max": round(max(ms), 3)}
    if phase:
        out["check_witness_ms"] = round(statistics.median(phase), 3)
    return out


def timed(hal, prove):
    hal.synchronize()
    t = time.perf_counter()
    seal = prove()
    hal.synchronize()
    return 1000.0 * (time.perf_counter() - t), seal


def measure(args, np, r, hal, prove):
    """the legs off and on of one workload, alternated"""
    ms, seals, phase = {0: [], 1: []}, {0: [], 1: []}, []
    for _ in range(args.warmups):
        for on in (0, 1):
            r.set_witness_check(on)
            prove()
    for _ in range(args.repeats):
        for on in (0, 1):
            r.set_witness_check(on)
            t, seal = timed(hal, prove)
            ms[on].append(t)
            seals[on].append(seal)
            if on:
                phase.append(r.last_profile().get("check_witness", 0.0))
    r.set_witness_check(0)
    print("  ".join(f"{'on' if on else 'off'}: {[round(x, 2) for x in ms[on]]}" for on in (0, 1)) + " ms",
          file=sys.stderr, flush=True)
    out = {"off": summary(ms[0]), "on": summary(ms[1], phase)}
    out["on_minus_off_ms"] = round(out["on"]["median"] - out["off"]["median"], 3)
    out["off_spread_ms"] = round(out["off"]["max"] - out["off"]["min"], 3)
    out["seals_equal"] = bool(all(np.array_equal(s, seals[0][0]) for on in (0, 1) for s in seals[on]))
    return out


def measure_off(args, hal, prove):
    for _ in range(args.warmups):
        prove()
    return summary([timed(hal, prove)[0] for _ in range(args.repeats)])


def workloads(args, np, r):
    """name -> (hal, prove) for the workloads asked for"""
    out = {}
    if "trace" in args.only:
        import bench
        t0 = time.perf_counter()
        hal = r.HipHal("poseidon2")
        jobs, tr0 = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments), [0])
        job = jobs[0]
        print(f"one po2={args.po2} session segment built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        out["trace"] = (hal, lambda: r.prove_segment_trace(hal, args.po2, job.glob, job.index, job.offsets, job.values,
                                                           job.cycles, job.txns, tr0.table_split_cycle,
                                                           bigint=tr0.bigint_array(),
                                                           bigint_records=tr0.bigint_records())[0])
    if "rec" in args.only:
        import recursion_program as RP
        t0 = time.perf_counter()
        po2 = args.rec_po2
        h = r.HipHal("poseidon2")
        prog, inp = RP.random_program(np.random.default_rng(0x5249534330), (1 << po2) - RP.ZK_CYCLES - 1)
        wom, cyc, iops = (np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
                          for a in RP.trace_arrays(RP.preflight(prog, inp)))
        ctrl = h.copy_from_elem("ctrl", RP.ctrl_group(prog, po2))
        print(f"one po2={po2} recursion program built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        out["rec"] = (h, lambda: r.prove_recursion(h, po2, ctrl, wom, cyc, iops, 0x5EED)[0])
    return out


def child(args):
    import numpy as np
    import risc0_amd as r
    print(json.dumps({name: measure_off(args, hal, prove) for name, (hal, prove) in workloads(args, np, r).items()}))


def against_parent(args):
    """leg c: the off legs on the parent's library and on this one, a child process each, ABAB"""
    runs = {"parent": [], "new": []}
    base = [sys.executable, os.path.abspath(__file__), "--child", "--po2", str(args.po2), "--rec-po2", str(args.rec_po2),
            "--segments", str(args.segments), "--repeats", str(args.repeats), "--warmups", str(args.warmups),
            "--only", ",".join(args.only)]
    for side in ("parent", "new", "parent", "new"):
        env = dict(os.environ)
        env.pop("R0HIP_LIB", None)
        if side == "parent":
            env["R0HIP_LIB"] = os.path.abspath(args.parent_lib)
        out = subprocess.run(base, env=env, stdout=subprocess.PIPE, check=True, timeout=900).stdout.decode()
        runs[side].append(json.loads(out.strip().splitlines()[-1]))
    res = {}
    for name in args.only:
        legs = {}
        for side in runs:
            ms = [x for run in runs[side] for x in run[name]["ms"]]
            legs[side] = summary(ms)
            legs[side]["process_medians"] = [run[name]["median"] for run in runs[side]]
        spread = round(legs["parent"]["max"] - legs["parent"]["min"], 3)
        slower = round(legs["new"]["median"] - legs["parent"]["median"], 3)
        res[name] = {**legs, "parent_spread_ms": spread, "new_minus_parent_ms": slower,
                     "off_path_within_parent_spread": bool(slower <= spread)}
    return res


def main():
    args = parse()
    if args.child:
        return child(args)
    result = {}
    if args.parent_lib:
        result["off_against_parent"] = against_parent(args)
    import numpy as np
    import risc0_amd as r
    for name, (hal, prove) in workloads(args, np, r).items():
        result[name] = measure(args, np, r, hal, prove)
    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    out = {
        "what": "one proof with r0hip_set_witness_check off and on (the constraint polynomial on the trace rows "
                "before the accum commit). Legs alternated in one process after warm-up rounds of each; ms = host "
                "clock around one proof between two r0hip_synchronize calls; check_witness_ms = median of the "
                "proof's check_witness phase. off_against_parent: the off leg on the parent commit's library and "
                "on this one, a child process each, parent and new alternating twice",
        "device": buf.value.decode(), "po2": args.po2, "rec_po2": args.rec_po2, "repeats": args.repeats,
        "warmup_rounds": args.warmups, **result,
        "seals_equal": bool(all(result[w]["seals_equal"] for w in args.only)),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not out["seals_equal"]:
        print("bench_witness_check: the legs' seals differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
