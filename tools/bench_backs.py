#!/usr/bin/env python3
"""The worker's kind-2 jobs (the injector as the preflight's Back records, expanded on the
device) against its CSR jobs (the injector expanded by the caller), on two workloads.

Needs an MI355X. ONE process, one persistent worker; per workload the two legs are alternated
(csr, backs, csr, backs, ...) after --warmups untimed rounds of each, --repeats timed rounds;
median and min..max of every figure. Workloads:

  loop    the bench's loop.s session (bench.session_jobs): one po2 segment as a job alone, and
          the --segments-job session at --inflight in flight; its injector is set_cycle's five
          entries per row and a few paging rows
  ecall   tests/rv32im_trace.ecall_trace(--ecall-po2, reps=--ecall-reps, bigint=True): rows of
          Poseidon2, SHA-256 and BigInt ecalls; one job alone and --ecall-jobs copies pipelined

The Back records of a leg are recovered from the job's CSR injector (unpack(): the inverse of
build_injector, checked here by expanding them again), so both legs prove the same segment.
Per leg: bytes staged per job, host ms inside r0hip_worker_submit per job, prove_ms of a job
alone, ms per segment pipelined. The expansion's device time comes from r0hip_kernel_times over
single calls on the calling thread: `rv32im_backs_inject` for the records; the CSR inject kernel
shares the name `rv32im_groups_init` with the groups' fill, which both legs run, so it is
reported as the difference of that name between the legs. Seals must be identical between the
legs. The result is one JSON file (default profiles/backs_ab.json) and the same line on stdout.

    python3 tools/bench_backs.py [--segments 24] [--inflight 3] [--repeats 7] [--out FILE]
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

P = 15 * 2**27 + 1
RINV = pow(1 << 32, -1, P)
WORDS = {3: 1, 39: 2, 103: 3, 22: 4}  # a row's entries beside set_cycle's five -> the record kind


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--segments", type=int, default=24)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--ecall-po2", type=int, default=16)
    ap.add_argument("--ecall-reps", type=int, default=30)
    ap.add_argument("--ecall-jobs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--wait-s", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backs_ab.json"))
    return ap.parse_args()


def unpack(np, index, offsets, values, rows):
    """the Back records of a CSR injector built by build_injector: per row, the entries before
    set_cycle's five are the row's Back, whose kind follows from their count; values go back from
    Montgomery words to plain integers, a SHA-2 row's 96 bit cells to its three words"""
    index = np.asarray(index, np.int64)
    count = np.diff(index) - 5
    assert count.min() >= 0
    plain = ((np.asarray(values, np.uint64) * np.uint64(RINV)) % np.uint64(P)).astype(np.uint32)
    recs, words, at = [], [], 0
    sh = np.arange(32, dtype=np.uint64)
    for row in np.flatnonzero(count):
        n, v = int(count[row]), plain[index[row]:index[row] + int(count[row])]
        recs.append((row, WORDS[n], at))
        if n == 103:
            w = [int(x) for x in v[:7]] + [int((v[7 + 32 * k:39 + 32 * k].astype(np.uint64) << sh).sum()) for k in range(3)]
        else:
            w = v.tolist()
        words += w
        at += len(w)
    return np.array(recs, np.uint32).reshape(-1, 3), np.array(words, np.uint32)


def main():
    args = parse()
    import numpy as np
    import bench
    import risc0_amd as r
    import rv32im_backs as B
    import rv32im_trace as T

    hal = r.HipHal("poseidon2")
    k = args.inflight
    t0 = time.perf_counter()
    loop_csr, _ = bench.session_jobs(r, argparse.Namespace(po2=args.po2, session=args.segments),
                                     list(range(args.segments)))
    te = T.ecall_trace(args.ecall_po2, seed=3, bigint=True, reps=args.ecall_reps)
    cyc, tx = te.arrays()
    ecall_csr = r.TraceJob(*(r.pinned_copy(a) for a in (te.global_words(), *te.injector_arrays(), cyc, tx)),
                           te.table_split_cycle, bigint=te.bigint_array(), bigint_records=te.bigint_records())
    majors = np.bincount(cyc["major"], minlength=13)
    print(f"inputs built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def backs_job(j, po2, check):
        recs, words = unpack(np, j.index, j.offsets, j.values, 1 << po2)
        if check:  # the records expand to the job's own injector
            again = B.expand(recs, words, j.index.size - 1, j.cycles.view(T.CYCLE_DTYPE).reshape(-1), 1 << po2)
            assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(again, (j.index, j.offsets, j.values)))
        backs = r.Backs(r.pinned_copy(recs), r.pinned_copy(words), j.index.size - 1)
        return r.BacksJob(j.glob, backs, j.cycles, j.txns, j.table_split, bigint=j.bigint, mode=0), recs

    loop_backs = [backs_job(j, args.po2, False)[0] for j in loop_csr]
    ecall_backs, ecall_recs = backs_job(ecall_csr, args.ecall_po2, True)
    kinds = np.bincount(ecall_recs[:, 1], minlength=5)

    def run(w, items, po2, backs):
        """submit every job, wait for all: (wall s, submit s, [prove_ms], seals in submission order)"""
        hal.synchronize()
        t0 = time.perf_counter()
        tickets = [(w.submit_backs if backs else w.submit_trace)(j, po2) for j in items]
        t1 = time.perf_counter()
        got = {}
        for _ in items:
            res = w.wait(args.wait_s)
            if res is None:
                raise RuntimeError(f"the worker returned nothing for {args.wait_s} s")
            if res[3]:
                raise RuntimeError(f"job {res[0]} failed: {res[3]}")
            got[res[0]] = res
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, [got[t][5] for t in tickets], [got[t][1] for t in tickets]

    def stat(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    def workload(w, csr, backs, po2):
        """one job alone and the whole list pipelined, csr and backs alternated"""
        out = {}
        for shape, pick in (("alone", lambda js: js[:1]), ("pipelined", lambda js: js)):
            legs = {"csr": pick(csr), "backs": pick(backs)}
            fig = {n: {"wall": [], "submit": [], "prove": []} for n in legs}
            seals = {}
            for rnd in range(args.warmups + args.repeats):
                for n, items in legs.items():
                    wall, sub, prove, s = run(w, items, po2, n == "backs")
                    seals[n] = s
                    if rnd >= args.warmups:
                        fig[n]["wall"].append(1000.0 * wall / len(items))
                        fig[n]["submit"].append(1000.0 * sub / len(items))
                        fig[n]["prove"].append(statistics.median(prove))
            res = {"jobs": len(legs["csr"]),
                   "seals_equal": all(np.array_equal(a, b) for a, b in zip(seals["csr"], seals["backs"]))}
            for n, items in legs.items():
                res[n] = {"staged_bytes_per_job": int(sum(j.h2d_bytes() for j in items) // len(items)),
                          "submit_ms_per_job": stat(fig[n]["submit"]), "prove_ms": stat(fig[n]["prove"]),
                          "ms_per_segment": stat(fig[n]["wall"])}
            c, b = res["csr"]["ms_per_segment"], res["backs"]["ms_per_segment"]
            res["backs_minus_csr_median_ms"] = round(b["median"] - c["median"], 3)
            res["csr_spread_ms"] = round(c["max"] - c["min"], 3)
            res["backs_within_csr_spread"] = bool(b["median"] - c["median"] <= c["max"] - c["min"])
            out[shape] = res
            print(f"{shape}: csr {c} backs {b} ms per segment", file=sys.stderr, flush=True)
        return out

    def kernel_ms(f):
        r.kernel_times()
        f()
        t = r.kernel_times()
        return {n: round(t[n][0], 4) for n in ("rv32im_groups_init", "rv32im_backs_inject") if n in t}

    def expansion(j, jb, po2):
        """device ms of the injector's kernels over single calls on this thread (timing on)"""
        csr = lambda: r.prove_segment_trace(hal, po2, j.glob, j.index, j.offsets, j.values, j.cycles, j.txns,
                                            j.table_split, bigint=j.bigint, bigint_records=j.records)
        bks = lambda: r.prove_segment_trace_backs(hal, po2, jb.glob, jb.backs, jb.cycles, jb.txns, j.table_split,
                                                  bigint=jb.bigint)
        csr(), bks()
        r.set_kernel_timing(True)
        try:
            a, b = [kernel_ms(csr) for _ in range(3)], [kernel_ms(bks) for _ in range(3)]
        finally:
            r.set_kernel_timing(False)
        fill = statistics.median(x["rv32im_groups_init"] for x in b)
        return {"csr_fill_and_inject_ms": statistics.median(x["rv32im_groups_init"] for x in a),
                "backs_fill_ms": fill, "backs_inject_ms": statistics.median(x["rv32im_backs_inject"] for x in b),
                "csr_inject_ms_by_difference": round(statistics.median(x["rv32im_groups_init"] for x in a) - fill, 4)}

    w = r.Worker(hal, max_po2=max(args.po2, args.ecall_po2), in_flight=k, verify=True)
    try:
        loop = workload(w, loop_csr, loop_backs, args.po2)
        ecall = workload(w, [ecall_csr] * args.ecall_jobs, [ecall_backs] * args.ecall_jobs, args.ecall_po2)
    finally:
        w.close()
    loop["expansion_kernels"] = expansion(loop_csr[0], loop_backs[0], args.po2)
    ecall["expansion_kernels"] = expansion(ecall_csr, ecall_backs, args.ecall_po2)
    rows = 1 << args.ecall_po2
    ecall["trace"] = {"po2": args.ecall_po2, "reps": args.ecall_reps, "rows": rows,
                      "records": {"ecall": int(kinds[1]), "poseidon2": int(kinds[2]), "sha2": int(kinds[3]),
                                  "bigint": int(kinds[4])},
                      "sha_row_share": round(float(kinds[3]) / rows, 4),
                      "poseidon2_row_share": round(float(kinds[2]) / rows, 4),
                      "csr_entries": int(ecall_csr.index[-1]), "sha_arm_rows": int(majors[11])}
    buf, total = C.create_string_buffer(256), C.c_uint64(0)
    r.check(r.lib().r0hip_device_info(buf, 256, C.byref(total)))
    result = {
        "what": "worker jobs with the injector as Back records (kind 2) against CSR jobs (kind 0), legs alternated in "
                "one process on one worker after warm-up rounds of each; medians and min..max over the repeats",
        "device": buf.value.decode(), "in_flight": k, "repeats": args.repeats, "warmup_rounds": args.warmups,
        "receipts_verified": True, "loop_session": dict(loop, po2=args.po2, segments=len(loop_csr)),
        "ecall_trace": ecall,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
