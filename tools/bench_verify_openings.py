#!/usr/bin/env python3
"""The receipt check with its Merkle openings on the device (r0hip_verify_seal_on, verify = 2)
against the host check it is an option beside.

Needs an MI355X. ONE process; after --warmups untimed rounds of every leg the timed repeats
alternate the legs, so drift of the machine falls on all alike. The host leg is the library's
behaviour without the option and the baseline of each comparison.

  (a) seals      r0hip_verify_seal_on(HOST) against (DEVICE) on one seal each of: an rv32im po2-20
                 segment of the bench's loop.s session with Poseidon2 and with SHA-256, and a
                 recursion program filling --rec-po2 (18) with Poseidon2. A third leg runs the
                 Poseidon2 openings one per lane instead of one per lane quad (R0_MERKLE_OPEN_QUAD=0).
                 ms = host clock around the call; kernel_ms = the opening kernel's own time from
                 r0hip_kernel_times (three more calls with kernel timing on).
  (b) pipeline   r0hip_prove_trace_segments over the session's --segments (12) po2-20 segments at
                 3 in flight with verify = 1 against 2: ms per segment and the mean verify_ms.
  (c) latency    one segment at 1 in flight, verify = 1 against 2: prove_ms + verify_ms.
  (d) p254       Poseidon254, whose device openings sit behind r0hip_set_verify_device_poseidon254
                 (the device legs turn it on for their call and off again): one recursion seal at
                 --rec-po2 from the GPU prover, host against device and against device with the trees'
                 top layers hashed level by level on the verifier's threads (R0_VERIFY_P254_TOPS=1,
                 hash_tops; the default is the serial loop), with the kernel's own time; and
                 --p254-jobs (12) Poseidon254 recursion jobs of that size through a worker at 3 in
                 flight, verify = 1 against 2: wall ms per job and the mean verify_ms. This part alone
                 (--only p254) writes profiles/verify_device_p254_ab.json.

Per comparison: each leg's repeats, median, min and max, the host leg's spread (max - min), the
device leg's gain (host median - device median) and whether the gain exceeds the spread (the rule
by which a change counts as a gain). One JSON file (default profiles/verify_device_ab.json) and the
same line on stdout.

    python3 tools/bench_verify_openings.py [--po2 20] [--rec-po2 18] [--segments 12] [--repeats 7]
                                           [--warmups 2] [--only seals,pipeline,latency,p254] [--out FILE]
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
PARTS = ("seals", "pipeline", "latency", "p254")


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rec-po2", type=int, default=18)
    ap.add_argument("--segments", type=int, default=12, help="segments of the session (b) proves")
    ap.add_argument("--repeats", type=int, default=7, help="timed repeats of each leg (at least 5)")
    ap.add_argument("--warmups", type=int, default=2, help="untimed rounds of each leg before the timed ones")
    ap.add_argument("--only", default=",".join(PARTS), help="comma-separated parts")
    ap.add_argument("--p254-jobs", type=int, default=12, help="recursion jobs the worker of (d) proves per repeat")
    ap.add_argument("--out", default=None, help="default profiles/verify_device_ab.json, or "
                                                "profiles/verify_device_p254_ab.json with --only p254")
    args = ap.parse_args()
    args.only = [w for w in args.only.split(",") if w]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles",
                                "verify_device_p254_ab.json" if args.only == ["p254"] else "verify_device_ab.json")
    if args.repeats < 5 or any(w not in PARTS for w in args.only):
        ap.error("--repeats must be at least 5, --only a list of " + ", ".join(PARTS))
    return args


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3)}


def compare(out, base, legs):
    """the rule: a leg is a gain when its median beats the base leg's by more than the base leg's spread"""
    out[base + "_spread_ms"] = round(out[base]["max"] - out[base]["min"], 3)
    for leg in legs:
        gain = round(out[base]["median"] - out[leg]["median"], 3)
        out[leg + "_gain_ms"] = gain
        out[leg + "_gain_exceeds_" + base + "_spread"] = bool(gain > out[base + "_spread_ms"])
    return out


def alternate(args, legs):
    """legs: name -> callable returning the leg's figure(s) for one repeat"""
    got = {name: [] for name in legs}
    for _ in range(args.warmups):
        for fn in legs.values():
            fn()
    for _ in range(args.repeats):
        for name, fn in legs.items():
            got[name].append(fn())
    return got


def seal_legs(args, r, circuit, suite, seal, po2):
    def timed(where, quad, tops=False):
        def run():
            os.environ["R0_MERKLE_OPEN_QUAD"] = "1" if quad else "0"
            os.environ["R0_VERIFY_P254_TOPS"] = "1" if tops else "0"
            r.set_verify_device_poseidon254(suite == 2 and where == "device")
            try:
                t = time.perf_counter()
                assert r.verify_seal(circuit, suite, seal, where=where) == po2
                return 1000.0 * (time.perf_counter() - t)
            finally:
                r.set_verify_device_poseidon254(0)
        return run
    legs = {"host": timed("host", True), "device": timed("device", True)}
    if suite == 0:
        legs["device_lane"] = timed("device", False)
    if suite == 2:  # the trees' top layers on the verifier's threads (hash_tops) instead of the serial loop
        legs["device_hash_tops"] = timed("device", True, tops=True)
    got = alternate(args, legs)
    out = {name: summary(ms) for name, ms in got.items()}
    for name in [n for n in legs if n != "host"]:  # the kernel's own time
        r.set_kernel_timing(True)
        for _ in range(3):
            legs[name]()
        kt = {k: v for k, v in r.kernel_times().items() if k.startswith("merkle_open")}
        r.set_kernel_timing(False)
        (kname, (ms, calls, _, _)), = kt.items()
        out[name]["kernel"] = kname
        out[name]["kernel_ms"] = round(ms / calls, 4)
    os.environ["R0_MERKLE_OPEN_QUAD"] = "1"
    os.environ.pop("R0_VERIFY_P254_TOPS", None)
    out["seal_words"] = int(seal.size)
    print(f"  {circuit} po2={po2} suite={suite}: " + "  ".join(
        f"{n}: {out[n]['median']} ms" + (f" (kernel {out[n]['kernel_ms']})" if "kernel_ms" in out[n] else "")
        for n in legs), file=sys.stderr, flush=True)
    return compare(out, "host", [n for n in legs if n != "host"])


def main():
    args = parse()
    import numpy as np
    import bench
    import risc0_amd as r

    hal = r.HipHal("poseidon2")
    result = {}
    t0 = time.perf_counter()
    jobs = []
    if set(args.only) & {"seals", "pipeline", "latency"}:
        mine = list(range(args.segments if "pipeline" in args.only else 1))
        jobs, tr0 = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments), mine)
        print(f"{len(jobs)} po2={args.po2} session segment(s) built in {time.perf_counter() - t0:.1f} s",
              file=sys.stderr, flush=True)
        job = jobs[0]

    if "seals" in args.only:
        seals = {}
        for name, suite in (("rv32im_poseidon2", "poseidon2"), ("rv32im_sha256", "sha-256")):
            h = hal if suite == "poseidon2" else r.HipHal(suite)
            seal = r.prove_segment_trace(h, args.po2, job.glob, job.index, job.offsets, job.values, job.cycles, job.txns,
                                         tr0.table_split_cycle, bigint=tr0.bigint_array(),
                                         bigint_records=tr0.bigint_records())[0]
            seals[name] = seal_legs(args, r, "rv32im", h.suite, seal, args.po2)
        import recursion_program as RP
        po2 = args.rec_po2
        prog, inp = RP.random_program(np.random.default_rng(0x5249534330), (1 << po2) - RP.ZK_CYCLES - 1)
        wom, cyc, iops = (np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
                          for a in RP.trace_arrays(RP.preflight(prog, inp)))
        ctrl = hal.copy_from_elem("ctrl", RP.ctrl_group(prog, po2))
        seal = r.prove_recursion(hal, po2, ctrl, wom, cyc, iops, 0x5EED)[0]
        ctrl.free()
        seals["recursion_poseidon2"] = seal_legs(args, r, "recursion", 0, seal, po2)
        result["seals"] = seals

    def pipeline(jobs_, in_flight, verify):
        def run():
            t = time.perf_counter()
            res = r.prove_trace_segments(hal, args.po2, jobs_, in_flight=in_flight, verify=verify, per_job=True)
            wall = 1000.0 * (time.perf_counter() - t)
            assert all(e is None for _, _, e, _, _ in res), [e for _, _, e, _, _ in res]
            return (wall / len(jobs_), statistics.mean(v for _, _, _, v, _ in res),
                    statistics.mean(p + v for _, _, _, v, p in res))
        return run

    if "pipeline" in args.only:
        got = alternate(args, {"host": pipeline(jobs, 3, 1), "device": pipeline(jobs, 3, 2)})
        out = {leg: dict(summary([x[0] for x in v]), verify_ms_mean=round(statistics.mean(x[1] for x in v), 3))
               for leg, v in got.items()}
        out["what"] = f"ms per segment, {len(jobs)} segments at 3 in flight"
        result["pipeline"] = compare(out, "host", ["device"])
        print(f"  pipeline: host {out['host']['median']} device {out['device']['median']} ms/segment", file=sys.stderr,
              flush=True)
    if "latency" in args.only:
        got = alternate(args, {"host": pipeline(jobs[:1], 1, 1), "device": pipeline(jobs[:1], 1, 2)})
        out = {leg: dict(summary([x[2] for x in v]), verify_ms=summary([x[1] for x in v])) for leg, v in got.items()}
        out["what"] = "prove_ms + verify_ms of one segment at 1 in flight"
        result["latency"] = compare(out, "host", ["device"])
        print(f"  latency: host {out['host']['median']} device {out['device']['median']} ms", file=sys.stderr, flush=True)

    if "p254" in args.only:
        import recursion_program as RP
        po2 = args.rec_po2
        prog, inp = RP.random_program(np.random.default_rng(0x5249534330), (1 << po2) - RP.ZK_CYCLES - 1)
        wom, cyc, iops = (np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
                          for a in RP.trace_arrays(RP.preflight(prog, inp)))
        ctrl_words = RP.ctrl_group(prog, po2)
        h254 = r.HipHal("poseidon254")
        ctrl = h254.copy_from_elem("ctrl", ctrl_words)
        seal = r.prove_recursion(h254, po2, ctrl, wom, cyc, iops, 0x5EED)[0]
        ctrl.free()
        out = {"recursion_poseidon254": seal_legs(args, r, "recursion", 2, seal, po2)}

        def worker(verify):
            def run():
                r.set_verify_device_poseidon254(verify == 2)
                try:
                    t = time.perf_counter()
                    with r.Worker(hal, max_po2=po2, in_flight=3, verify=verify) as w:
                        for _ in range(args.p254_jobs):
                            w.submit_recursion(po2, ctrl_words, wom, cyc, iops, suite="poseidon254")
                        res = [w.wait(600.0) for _ in range(args.p254_jobs)]
                    wall = 1000.0 * (time.perf_counter() - t)
                finally:
                    r.set_verify_device_poseidon254(0)
                assert all(x is not None and x[3] is None for x in res), [x and x[3] for x in res]
                return wall / args.p254_jobs, statistics.mean(x[4] for x in res)
            return run

        got = alternate(args, {"host": worker(1), "device": worker(2)})
        wk = {leg: dict(summary([x[0] for x in v]), verify_ms_mean=round(statistics.mean(x[1] for x in v), 3))
              for leg, v in got.items()}
        wk["what"] = (f"wall ms per job (worker created and destroyed inside the timed span), {args.p254_jobs} "
                      f"Poseidon254 recursion jobs of po2 {po2} at 3 in flight")
        out["worker"] = compare(wk, "host", ["device"])
        print(f"  p254 worker: host {wk['host']['median']} device {wk['device']['median']} ms/job, verify_ms "
              f"{wk['host']['verify_ms_mean']} -> {wk['device']['verify_ms_mean']}", file=sys.stderr, flush=True)
        result["p254"] = out

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    out = {
        "what": "the receipt check with the seal's Merkle openings on host threads (host: r0hip_verify_seal, "
                "verify = 1) against one device launch (device: r0hip_verify_seal_on(DEVICE), verify = 2; "
                "device_lane: the Poseidon2 kernel with one opening per lane instead of one per lane quad; p254: "
                "Poseidon254, the device legs under r0hip_set_verify_device_poseidon254(1)). "
                "Legs alternated in one process after warm-up rounds of each",
        "device": buf.value.decode(), "po2": args.po2, "rec_po2": args.rec_po2, "repeats": args.repeats,
        "warmup_rounds": args.warmups, "verify_threads": os.environ.get("R0HIP_VERIFY_THREADS", "default (up to 8)"),
        "unmeasured": [p for p in PARTS if p not in args.only], **result,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
