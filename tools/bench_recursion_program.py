#!/usr/bin/env python3
"""Recursion proofs from a resident program (r0hip_recursion_program_*) against the keyed call
and the worker's kind-1 jobs as they stand.

Needs an MI355X. ONE process. The program is tests/recursion_program.satisfying_witness(seed,
--po2): a random program filling the segment, its preflight, its control group. Per suite
(SHA-256 and Poseidon2: every leg; Poseidon254: one pair, `keyed` against `program`) the legs
are alternated (keyed, keyed_upload, program, keyed, ...) after --warmups untimed rounds of
each, --repeats timed rounds; a repeat is one proof between two r0hip_synchronize calls on the
host clock. Reported per leg: every repeat, median, min and max.

  keyed          r0hip_prove_recursion_keyed with d_ctrl already on the device
  keyed_upload   the same with the 23 x 2^po2 word h_ctrl upload (pageable host memory, as a
                 caller holds it) and the buffer's free inside the timed region: what a caller
                 pays per proof today. The host transposition of WitnessGenerator::new that such
                 a caller also runs per proof is NOT in it (here it is Python and would swamp
                 the figure).
  program        r0hip_prove_recursion_program from a handle made before the timed region
  worker_kind1   --jobs recursion jobs at --inflight in flight through a worker made before the
  worker_kind3   timed region (a fresh one per repeat, so tickets and with them the ZK noise agree
                 between the legs): submit all, wait for all; ms per job. Kind 1 stages h_ctrl
                 per job, kind 3 names the handle.

Also: the one-off cost of r0hip_recursion_program_create (median of --repeats creates, each
destroyed again), and the number of proofs after which a handle has paid for itself against
keyed_upload: create / (keyed_upload - program), when that difference is positive.

Per pair the compared leg's spread (max - min) is reported beside the gain of `program`
(compared median - program median) and whether the gain exceeds the spread, the rule of DESIGN.md
section 7 item 9. All seals of a suite's single-call legs must be equal, and every worker job's
seal must equal its twin's of the other kind. One JSON file (default
profiles/recursion_program_ab.json) and the same line on stdout.

    python3 tools/bench_recursion_program.py [--po2 18] [--repeats 7] [--warmups 2] [--jobs 12]
                                             [--inflight 3] [--cache FILE] [--build-only] [--out FILE]

--cache FILE keeps the built program (an .npz of its code words, control group and trace) so a
later run skips the minute of Python that builds it; --build-only writes the cache and stops (no
GPU needed).
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = 0x5249534330
KEY = bytes(range(32))
SUITES = (("sha256", "sha-256", True), ("poseidon2", "poseidon2", True), ("poseidon254", "poseidon254", False))


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=18)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--jobs", type=int, default=12)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--wait-s", type=float, default=300.0)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recursion_program_ab.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    return args


def build_program(np, po2, cache):
    """code words (row-major, plain), the control group, WOM, cycles and IOP values"""
    if cache and os.path.exists(cache):
        z = np.load(cache)
        if int(z["po2"]) == po2 and int(z["seed"]) == SEED:
            return {k: z[k] for k in ("code", "ctrl", "wom", "cyc", "iops")}
    import recursion_program as RP
    t0 = time.perf_counter()
    if RP.available():
        w = RP.satisfying_witness(SEED, po2)
        prog, pf, ctrl = w["program"], w["preflight"], w["ctrl"]
    else:  # the same program and trace without the compiled reference's witness generator
        prog, inp = RP.random_program(np.random.default_rng(SEED), (1 << po2) - RP.ZK_CYCLES - 1)
        pf, ctrl = RP.preflight(prog, inp), RP.ctrl_group(prog, po2)
    wom, cyc, iops = (np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1)) for a in RP.trace_arrays(pf))
    out = dict(code=prog.encoded(), ctrl=np.ascontiguousarray(ctrl, dtype=np.uint32), wom=wom, cyc=cyc, iops=iops)
    print(f"one po2={po2} recursion program of {len(prog.rows)} rows built in {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    if cache:
        np.savez(cache, po2=po2, seed=SEED, **out)
    return out


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3)}


def compare(out, base, leg):
    """the gain of `leg` over `base` beside base's own spread"""
    spread = round(out[base]["max"] - out[base]["min"], 3)
    gain = round(out[base]["median"] - out[leg]["median"], 3)
    return {"compared": base, "spread_ms": spread, "gain_ms": gain, "gain_exceeds_spread": bool(gain > spread)}


def single_legs(args, np, r, hal, p, legs):
    """the single-call legs of one suite, alternated; returns their summaries and whether every
    seal equals the first"""
    po2 = args.po2
    d_ctrl = hal.copy_from_elem("ctrl", p["ctrl"])
    prog = r.RecursionProgram.create(hal, po2, p["code"])
    sid = [0]

    def keyed():
        return r.prove_recursion_keyed(hal, po2, d_ctrl, p["wom"], p["cyc"], p["iops"], KEY, sid[0])[0]

    def keyed_upload():
        d = hal.copy_from_elem("ctrl", p["ctrl"])
        seal = r.prove_recursion_keyed(hal, po2, d, p["wom"], p["cyc"], p["iops"], KEY, sid[0])[0]
        d.free()
        return seal

    def program():
        return prog.prove(p["wom"], p["cyc"], p["iops"], KEY, sid[0])[0]

    fns = {"keyed": keyed, "keyed_upload": keyed_upload, "program": program}
    ms = {leg: [] for leg in legs}
    equal = True
    for _ in range(args.warmups):
        for leg in legs:
            fns[leg]()
    for rep in range(args.repeats):
        sid[0] = 1 + rep  # one stream_id per round: the legs of a round make one seal
        first = None
        for leg in legs:
            hal.synchronize()
            t = time.perf_counter()
            seal = fns[leg]()
            hal.synchronize()
            ms[leg].append(1000.0 * (time.perf_counter() - t))
            if first is None:
                first = seal
            equal = equal and bool(np.array_equal(seal, first))
    print("  ".join(f"{leg}: {[round(x, 2) for x in ms[leg]]}" for leg in legs) + " ms", file=sys.stderr, flush=True)
    out = {leg: summary(ms[leg]) for leg in legs}
    # the one-off cost of a handle
    create_ms = []
    for _ in range(args.repeats):
        hal.synchronize()
        t = time.perf_counter()
        h = r.RecursionProgram.create(hal, po2, p["code"])
        create_ms.append(1000.0 * (time.perf_counter() - t))
        h.close()
    out["create"] = summary(create_ms)
    info = prog.info()
    out["device_bytes"] = int(info[4])
    out["control_id"] = [int(x) for x in info[3]]
    prog.close()
    d_ctrl.free()
    return out, equal, info[3]


def worker_legs(args, np, r, hal, p, cid):
    """--jobs recursion jobs at --inflight in flight, kind 1 against kind 3, ms per job"""
    po2 = args.po2
    prog = r.RecursionProgram.create(hal, po2, p["code"])
    ctrl = r.pinned_copy(p["ctrl"])  # the worker's h_ctrl at full PCIe rate, as INTEGRATION.md asks

    def run(kind):
        with r.Worker(hal, max_po2=po2, in_flight=args.inflight, verify=True, noise_key=KEY) as w:
            hal.synchronize()
            t = time.perf_counter()
            for _ in range(args.jobs):
                if kind == 1:
                    w.submit_recursion(po2, ctrl, p["wom"], p["cyc"], p["iops"], code_roots=cid)
                else:
                    w.submit_recursion_program(prog, p["wom"], p["cyc"], p["iops"])
            seals = {}
            for _ in range(args.jobs):
                res = w.wait(args.wait_s)
                if res is None:
                    raise SystemExit("bench_recursion_program: a worker job did not come back")
                if res[3] is not None:
                    raise SystemExit(f"bench_recursion_program: job {res[0]}: {res[3]}")
                seals[res[0]] = res[1]
            ms = 1000.0 * (time.perf_counter() - t) / args.jobs
        return ms, seals

    ms = {1: [], 3: []}
    equal = True
    for _ in range(args.warmups):
        run(1)
        run(3)
    for _ in range(args.repeats):
        m1, s1 = run(1)
        m3, s3 = run(3)
        ms[1].append(m1)
        ms[3].append(m3)
        equal = equal and all(np.array_equal(s1[k], s3[k]) for k in s1)
    print(f"worker kind 1: {[round(x, 2) for x in ms[1]]}  kind 3: {[round(x, 2) for x in ms[3]]} ms per job",
          file=sys.stderr, flush=True)
    prog.close()
    return {"worker_kind1": summary(ms[1]), "worker_kind3": summary(ms[3])}, equal


def main():
    args = parse()
    import numpy as np
    p = build_program(np, args.po2, args.cache)
    if args.build_only:
        return
    import risc0_amd as r

    result, seals_equal = {}, True
    for name, suite, full in SUITES:
        hal = r.HipHal(suite)
        legs = ("keyed", "keyed_upload", "program") if full else ("keyed", "program")
        out, eq, cid = single_legs(args, np, r, hal, p, legs)
        out["program_vs_keyed"] = compare(out, "keyed", "program")
        if full:
            out["program_vs_keyed_upload"] = compare(out, "keyed_upload", "program")
            saved = out["keyed_upload"]["median"] - out["program"]["median"]
            out["proofs_to_pay_for_create"] = round(out["create"]["median"] / saved, 2) if saved > 0 else None
            wout, weq = worker_legs(args, np, r, hal, p, cid)
            out.update(wout)
            out["worker_kind3_vs_kind1"] = compare(out, "worker_kind1", "worker_kind3")
            eq = eq and weq
        out["seals_equal"] = bool(eq)
        seals_equal = seals_equal and eq
        result[name] = out
        r.trim()

    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    out = {
        "what": "recursion proofs of one program filling a po2 segment: r0hip_prove_recursion_keyed with the control "
                "group on the device (keyed), with its upload from pageable host memory in the timed region "
                "(keyed_upload; the caller's host transposition is not included), and "
                "r0hip_prove_recursion_program from a handle (program); the worker at in_flight with kind-1 jobs "
                "(h_ctrl staged per job, from page-locked memory) and kind-3 jobs (the handle), ms per job. Legs "
                "alternated in one process after warm-up rounds of each; ms = host clock between two "
                "r0hip_synchronize calls. create = one r0hip_recursion_program_create. Not measured: a real "
                "lift or join program, Poseidon254 in the worker, more than two handles resident",
        "device": buf.value.decode(), "po2": args.po2, "repeats": args.repeats, "warmup_rounds": args.warmups,
        "worker_jobs": args.jobs, "worker_in_flight": args.inflight, "h_ctrl_bytes": int(p["ctrl"].nbytes),
        "code_rows": int(p["code"].size // 23), **result, "seals_equal": bool(seals_equal),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not seals_equal:
        print("bench_recursion_program: the legs' seals differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
