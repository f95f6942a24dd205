#!/usr/bin/env python3
"""The per-op path in deferred completion mode against the same path in the default mode.

Needs an MI355X. Builds one segment of the bench's loop.s session (bench.session_jobs: the first
of --segments consecutive po2=20 segments, in page-locked memory) and proves it through the
native per-op driver (integration/hal_prover.cpp, what a Rust HipHal delivers) three ways in ONE
process:

  sync      halp_prove_trace, every r0hip_* call complete on return (the default mode)
  deferred  the same call sequence under r0hip_set_deferred(1): the device-only calls return
            with their work queued; the host waits where the Prover reads
  fused     r0hip_prove_segment_trace on the same trace: the floor, no per-op boundary at all

After --warmups untimed rounds of each leg, the timed repeats alternate sync/deferred/fused, so
drift of the machine falls on all alike. Each repeat is one proof between two r0hip_synchronize
calls, timed on the host clock. Reported: ms of every repeat, mean, min and max of each leg, the
sync leg's spread (max - min), deferred minus sync, and whether the deferred mean lies below,
inside or above the sync leg's min..max; the per-proof call counters (calls, drained, queued) of
both per-op legs; the driver's host phases. The three seals must be equal. The result is one JSON
file (default profiles/per_op_deferred_ab.json) and the same line on stdout.

    python3 tools/bench_per_op.py [--po2 20] [--repeats 7] [--warmups 2] [--out FILE]

With --mirror-budget BYTES the legs are instead the node-heap mirror budget's (halp_set_mirror_budget;
all in the default completion mode, same alternation, same clock):

  default   the default budget (4 GiB): at po2 <= 21 every tree's node heap is mirrored
  budget    the given budget; 0 = no mirror, one r0hip_merkle_paths_host call per opening
  parent    with --parent-driver FILE: a libr0hip_halprover.so built from another commit's
            integration/hal_prover.cpp against this libr0hip.so, loaded beside this one

Reported besides each leg's ms: halp_mirror_stats of one proof of the first two legs, each leg's
mean against the parent's min..max (or the default's without a parent), the call counters and the
host phases. Default output profiles/per_op_mirror_budget_ab.json.

    python3 tools/bench_per_op.py --mirror-budget 0 [--parent-driver FILE] [--po2 20] [--repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "integration"))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--segments", type=int, default=2, help="segments of the session the first is taken from")
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats of each leg (at least 5)")
    ap.add_argument("--warmups", type=int, default=2, help="untimed rounds of each leg before the timed ones")
    ap.add_argument("--mirror-budget", type=int, default=None, metavar="BYTES",
                    help="run the mirror-budget legs (default budget, this budget, --parent-driver) instead")
    ap.add_argument("--parent-driver", default=None, metavar="FILE",
                    help="with --mirror-budget: another commit's libr0hip_halprover.so as a third leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_driver and args.mirror_budget is None:
        ap.error("--parent-driver needs --mirror-budget")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "per_op_deferred_ab.json" if args.mirror_budget is None
                                else "per_op_mirror_budget_ab.json")
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    return args


def leg_summary(v):
    return {"ms": [round(x, 3) for x in v], "mean": round(sum(v) / len(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def mirror_budget_ab(args, np, r, hal, halprover, job):
    """the --mirror-budget legs; returns the result dict"""
    def with_budget(nbytes):
        def run():
            halprover.set_mirror_budget(nbytes)
            return halprover.prove_trace(hal, args.po2, job)[0]
        return run

    run = {"default": with_budget(halprover.DEFAULT_MIRROR_BUDGET), "budget": with_budget(args.mirror_budget)}
    if args.parent_driver:
        this = halprover.lib()
        other = C.CDLL(os.path.abspath(args.parent_driver))
        other.halp_prove_trace.restype = other.halp_set_deferred.restype = other.halp_last_profile.restype = C.c_void_p
        other.halp_prove_trace.argtypes = this.halp_prove_trace.argtypes
        other.halp_set_deferred.argtypes = this.halp_set_deferred.argtypes
        other.halp_last_profile.argtypes = this.halp_last_profile.argtypes

        def parent():
            halprover._lib = other
            try:
                return halprover.prove_trace(hal, args.po2, job)[0], halprover.last_profile()
            finally:
                halprover._lib = this
        run["parent"] = lambda: parent()[0]
    order = tuple(run)
    legs, calls, phases, stats, seals = ({name: [] for name in order}, {}, {name: {} for name in order}, {}, {})
    for _ in range(args.warmups):
        for name in order:
            run[name]()
    for _ in range(args.repeats):
        for name in order:
            hal.synchronize()
            halprover.mirror_stats(reset=True)
            s0 = r.call_stats()
            t = time.perf_counter()
            seals[name] = run[name]()
            hal.synchronize()
            legs[name].append(1000.0 * (time.perf_counter() - t))
            s1 = r.call_stats()
            calls[name] = {k: s1[k] - s0[k] for k in s1}
            if name != "parent":
                stats[name] = halprover.mirror_stats()
                for k, v in halprover.last_profile().items():
                    phases[name][k] = phases[name].get(k, 0.0) + v / args.repeats
    halprover.set_mirror_budget(halprover.DEFAULT_MIRROR_BUDGET)
    print("  ".join(f"{name}: {[round(x, 2) for x in legs[name]]}" for name in order) + " ms", file=sys.stderr, flush=True)
    out = {name: leg_summary(legs[name]) for name in order}
    base = "parent" if "parent" in out else "default"
    lo, hi = out[base]["min"], out[base]["max"]
    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "one po2=%d loop.s session segment through the native per-op driver (halp_prove_trace, default "
                "completion mode) under the default node-heap mirror budget, under --mirror-budget%s; legs alternated "
                "in one process after warm-up rounds of each; ms = host clock around one proof between two "
                "r0hip_synchronize calls" % (args.po2, ", and through the parent commit's driver library"
                                             if "parent" in out else ""),
        "device": buf.value.decode(), "po2": args.po2, "repeats": args.repeats, "warmup_rounds": args.warmups,
        "mirror_budget_bytes": {"default": halprover.DEFAULT_MIRROR_BUDGET, "budget": args.mirror_budget},
        **out,
        base + "_spread_ms": round(hi - lo, 3),
        "mean_vs_%s_range" % base: {name: "below" if out[name]["mean"] < lo else "above" if out[name]["mean"] > hi
                                    else "inside" for name in order if name != base},
        "budget_minus_default_ms": round(out["budget"]["mean"] - out["default"]["mean"], 3),
        "mirror_stats_per_proof": stats,
        "calls_per_proof": calls,
        "host_phases_ms": {name: {k: round(v, 2) for k, v in phases[name].items()} for name in stats},
        "seals_equal": bool(all(np.array_equal(seals[order[0]], seals[name]) for name in order)),
    }
    return result


def main():
    args = parse()
    import numpy as np
    import bench
    import halprover
    import risc0_amd as r

    hal = r.HipHal("poseidon2")
    t0 = time.perf_counter()
    jobs, tr0 = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments), [0])
    job = jobs[0]
    print(f"one po2={args.po2} session segment built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    if args.mirror_budget is not None:
        result = mirror_budget_ab(args, np, r, hal, halprover, job)
        return finish(args, result)

    def fused():
        seal, _ = r.prove_segment_trace(hal, args.po2, job.glob, job.index, job.offsets, job.values, job.cycles,
                                        job.txns, tr0.table_split_cycle, bigint=tr0.bigint_array(),
                                        bigint_records=tr0.bigint_records())
        return seal

    run = {
        "sync": lambda: halprover.prove_trace(hal, args.po2, job)[0],
        "deferred": lambda: halprover.prove_trace(hal, args.po2, job, deferred=True)[0],
        "fused": fused,
    }
    order = ("sync", "deferred", "fused")
    legs = {name: [] for name in order}
    calls = {name: None for name in order}
    phases = {name: {} for name in order}
    seals = {}
    for _ in range(args.warmups):  # the thread's pool, scratch and arena; the driver's host mirrors
        for name in order:
            run[name]()
    for _ in range(args.repeats):
        for name in order:
            hal.synchronize()
            s0 = r.call_stats()
            t = time.perf_counter()
            seals[name] = run[name]()
            hal.synchronize()
            legs[name].append(1000.0 * (time.perf_counter() - t))
            s1 = r.call_stats()
            calls[name] = {k: s1[k] - s0[k] for k in s1}
            if name != "fused":
                for k, v in halprover.last_profile().items():
                    phases[name][k] = phases[name].get(k, 0.0) + v / args.repeats
    print("  ".join(f"{name}: {[round(x, 2) for x in legs[name]]}" for name in order) + " ms", file=sys.stderr, flush=True)

    ls, ld, lf = (leg_summary(legs[name]) for name in order)
    spread = round(ls["max"] - ls["min"], 3)
    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "one po2=%d loop.s session segment through the native per-op driver (halp_prove_trace), in the "
                "default mode and under r0hip_set_deferred(1), and through the fused r0hip_prove_segment_trace; legs "
                "alternated in one process after warm-up rounds of each; ms = host clock around one proof between "
                "two r0hip_synchronize calls" % args.po2,
        "device": buf.value.decode(), "po2": args.po2, "repeats": args.repeats, "warmup_rounds": args.warmups,
        "sync": ls, "deferred": ld, "fused": lf,
        "sync_spread_ms": spread,
        "deferred_minus_sync_ms": round(ld["mean"] - ls["mean"], 3),
        "deferred_mean_vs_sync_spread": "below" if ld["mean"] < ls["min"] else "above" if ld["mean"] > ls["max"] else "inside",
        "deferred_not_slower_than_sync_by_more_than_its_spread": bool(ld["mean"] <= ls["mean"] + spread),
        "calls_per_proof": {"sync": calls["sync"], "deferred": calls["deferred"]},
        "host_phases_ms": {name: {k: round(v, 2) for k, v in phases[name].items()} for name in ("sync", "deferred")},
        "seals_equal": bool(np.array_equal(seals["sync"], seals["deferred"]) and
                            np.array_equal(seals["sync"], seals["fused"])),
    }
    finish(args, result)


def finish(args, result):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    if not result["seals_equal"]:
        print("bench_per_op: the legs' seals differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
