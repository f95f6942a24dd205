#!/usr/bin/env python3
"""The GPU worker against the batch call it is built from, on the bench's own workload.

Needs an MI355X. Builds the bench's loop.s session (bench.session_jobs: --segments consecutive
po2=20 segments of one run, in page-locked memory) and proves it three ways in ONE process:

  a   r0hip_prove_trace_segments(in_flight)   every job handed over up front; the calling
                                              thread is one of the provers
  b   one persistent r0hip_worker             the same jobs submitted at once, then waited
                                              for; in_flight prover threads, the caller idle
  mixed size: segments - 1 of the po2=20 segments and a final segment of --final-po2 (a
      terminating loop.s guest of that size), as
  a2  two r0hip_prove_trace_segments calls    one per po2, the pipeline drained between them
  b2  the same worker                          all of them in one queue

After --warmups untimed rounds of each pair, alternated like the timed ones (two by default:
with one, the first batch call after the worker's first run was 15 ms per segment slower, most
likely because the worker's threads had taken the pooled device blocks the batch call's exited
threads left), the legs alternate
a/b/a/b/a/b (then a2/b2/...), so drift of the machine falls on both alike. Reported: ms per segment of every repeat, the mean of each leg, the
spread (min..max) of the three `a` repeats, and whether `b`'s mean lies below, inside or above it. Every receipt
is verified in every leg, and the legs' seals are compared. The result is one JSON file
(default profiles/worker_ab.json) and the same line on stdout.

    python3 tools/bench_worker.py [--segments 24] [--inflight 3] [--repeats 3] [--out FILE]
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--segments", type=int, default=24)
    ap.add_argument("--final-po2", type=int, default=17)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmups", type=int, default=2, help="untimed a/b rounds before the timed ones")
    ap.add_argument("--wait-s", type=float, default=300.0, help="longest wait for one job of the worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "worker_ab.json"))
    return ap.parse_args()


def main():
    args = parse()
    import numpy as np
    import bench
    import risc0_amd as r
    import rv32im_trace as T

    hal = r.HipHal("poseidon2")
    k = args.inflight
    t0 = time.perf_counter()
    jobs, _ = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments),
                                 list(range(args.segments)))
    tf = T.loop_s_trace(args.final_po2, seed=0x5249534330 + 99)
    cyc, tx = tf.arrays()
    final = r.TraceJob(*(r.pinned_copy(a) for a in (tf.global_words(), *tf.injector_arrays(), cyc, tx)),
                       tf.table_split_cycle, bigint=tf.bigint_array(), bigint_records=tf.bigint_records())
    print(f"{len(jobs)} po2={args.po2} session segments and one po2={args.final_po2} segment built in "
          f"{time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def batch(po2, js):
        res = r.prove_trace_segments(hal, po2, js, in_flight=min(k, len(js)), per_job=True, verify=True)
        bad = [e for _, _, e, _, _ in res if e]
        if bad:
            raise RuntimeError(f"{len(bad)} of {len(res)} segments failed: {bad[0]}")
        return [s for s, _, _, _, _ in res]

    def queue(w, items):
        """submit every (job, po2) at once, wait for all; seals in submission order"""
        tickets = [w.submit_trace(j, p) for j, p in items]
        got = {}
        for _ in items:
            res = w.wait(args.wait_s)
            if res is None:
                raise RuntimeError(f"the worker returned nothing for {args.wait_s} s")
            if res[3]:
                raise RuntimeError(f"job {res[0]} failed: {res[3]}")
            got[res[0]] = res[1]
        return [got[t] for t in tickets]

    def timed(f):
        hal.synchronize()
        t = time.perf_counter()
        out = f()
        hal.synchronize()
        return time.perf_counter() - t, out

    same = [(j, args.po2) for j in jobs]
    mixed = same[:-1] + [(final, args.final_po2)]
    legs = {name: [] for name in ("a", "b", "a2", "b2")}
    seals = {}
    t0 = time.perf_counter()
    w = r.Worker(hal, max_po2=args.po2, in_flight=k, verify=True)
    create_ms = 1000.0 * (time.perf_counter() - t0)
    try:
        run = {
            "a": lambda: batch(args.po2, jobs),
            "b": lambda: queue(w, same),
            "a2": lambda: batch(args.po2, jobs[:-1]) + batch(args.final_po2, [final]),
            "b2": lambda: queue(w, mixed),
        }
        for pair in (("a", "b"), ("a2", "b2")):
            for _ in range(args.warmups):  # every thread's stream, pool and scratch; the sets' growth
                for name in pair:
                    run[name]()
            for _ in range(args.repeats):
                for name in pair:
                    dt, out = timed(run[name])
                    legs[name].append(1000.0 * dt / len(jobs))
                    seals[name] = out
            print(f"{pair[0]}: {[round(x, 3) for x in legs[pair[0]]]}  {pair[1]}: "
                  f"{[round(x, 3) for x in legs[pair[1]]]} ms per segment", file=sys.stderr, flush=True)
    finally:
        t0 = time.perf_counter()
        w.close()
        destroy_ms = 1000.0 * (time.perf_counter() - t0)

    def equal(x, y):
        return len(seals[x]) == len(seals[y]) and all(np.array_equal(p, q) for p, q in zip(seals[x], seals[y]))

    def leg(name):
        v = legs[name]
        return {"ms_per_segment": [round(x, 3) for x in v], "mean": round(sum(v) / len(v), 3),
                "min": round(min(v), 3), "max": round(max(v), 3)}

    def compare(a, b):
        la, lb = leg(a), leg(b)
        return {a: la, b: lb, "worker_minus_batch_ms": round(lb["mean"] - la["mean"], 3),
                "batch_spread_ms": round(la["max"] - la["min"], 3),
                "worker_mean_vs_batch_spread": "below" if lb["mean"] < la["min"] else
                "above" if lb["mean"] > la["max"] else "inside",
                "seals_equal": equal(a, b)}

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "the GPU worker (r0hip_worker_*) against r0hip_prove_trace_segments on the bench's loop.s session, "
                "legs alternated in one process after warm-up rounds of each; ms per segment = wall time of the leg / segments",
        "device": buf.value.decode(), "po2": args.po2, "segments": len(jobs), "final_po2": args.final_po2, "in_flight": k,
        "repeats": args.repeats, "warmup_rounds": args.warmups, "receipts_verified": True,
        "same_size": compare("a", "b"),
        "mixed_size": compare("a2", "b2"),
        "worker_create_ms": round(create_ms, 1), "worker_destroy_ms": round(destroy_ms, 1),
        "legs": {"a": "r0hip_prove_trace_segments, all segments in one call (the caller is one of the provers)",
                 "b": "one persistent worker, the same jobs submitted at once (the caller proves nothing)",
                 "a2": f"two r0hip_prove_trace_segments calls: {len(jobs) - 1} po2={args.po2} segments, then one "
                       f"po2={args.final_po2} segment",
                 "b2": "the same worker, the same segments in one queue"},
    }
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
