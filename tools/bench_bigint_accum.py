#!/usr/bin/env python3
"""rv32im BigInt accumulator states: the serial host loop against the device scans.

For n in 2^8 .. 2^20 records of a segment of 2^21 rows, in one process, the two legs
alternating:

  host    r0hip_rv32im_bigint_accum_states (the serial loop), then the upload of its states
          (48 n bytes) and of the row list (4 n bytes), then the scatter into the accum group:
          what rv32im_bigint_inject did before the device path existed;
  device  r0hip_rv32im_bigint_accum_states_device (upload of the records, 28 n bytes, the
          scans, the readback of the failing-EqZero word), then the same scatter.

Both legs scatter with r0hip_scatter over a CSR index kept on the device (the library's own
scatter kernel is reachable only through the injection); `inject` times
r0hip_rv32im_bigint_accum_inject as a whole, on whichever path the library takes at that n.
Every call ends in a device synchronise, so the host clock around it is the time. The accum
groups the two legs leave are compared once per n.

The crossover for rv32im_bigint_inject (bigint.cpp, kDeviceMinRecords) is the smallest
measured n at which `device` is not slower than `host`.

  python tools/bench_bigint_accum.py [--out profiles/r7_bigint_accum.json] [--reps 15]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ROWS = 1 << 21
SIZES = [1 << k for k in range(8, 21, 2)]
INVALID = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7_bigint_accum.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import bigint_records as G
    import risc0_amd as r
    from risc0_amd.hal import check, u32p
    hal = r.HipHal("poseidon2")
    L = r.lib()
    name = C.create_string_buffer(256)
    mem = C.c_uint64()
    check(L.r0hip_device_info(name, 256, C.byref(mem)))

    rng = np.random.default_rng(0xB16ACC)
    mix = rng.integers(0, 2013265921, 36, dtype=np.uint64).astype(np.uint32)
    mp = mix.ctypes.data_as(u32p)
    accum = [hal.alloc_elem_init("accum", 12 * ROWS, INVALID) for _ in range(2)]
    result = {"device": name.value.decode(), "rows": ROWS, "reps": args.reps, "warmup": args.warmup, "unit": "ms",
              "sizes": []}
    for n in SIZES:
        recs = G.valid_stream(rng, n, ROWS)
        backs = r.bigint_backs(recs)
        bp = C.cast(backs, C.c_void_p)
        h_rows = np.ascontiguousarray(recs["row"])
        h_states = np.zeros(n * 12, np.uint32)
        d_states, d_rows = hal.alloc_u32("states", n * 12), hal.alloc_u32("rows", n)
        # record k's word c goes to accum[c * ROWS + row_k]
        d_index = hal.copy_from_u32("index", np.arange(n + 1, dtype=np.uint32) * 12)
        d_offsets = hal.copy_from_u32("offsets", (np.arange(12, dtype=np.uint32)[None, :] * ROWS
                                                  + h_rows[:, None]).reshape(-1))

        def host(acc):
            check(L.r0hip_rv32im_bigint_accum_states(mp, bp, n, ROWS, h_states.ctypes.data_as(u32p)))
            check(L.r0hip_memcpy_h2d(d_states.ptr, h_states.ctypes.data, n * 48))
            check(L.r0hip_memcpy_h2d(d_rows.ptr, h_rows.ctypes.data, n * 4))
            check(L.r0hip_scatter(acc.ptr, d_index.ptr, d_offsets.ptr, d_states.ptr, n))

        def device(acc):
            check(L.r0hip_rv32im_bigint_accum_states_device(d_states.ptr, mp, bp, n, ROWS))
            check(L.r0hip_scatter(acc.ptr, d_index.ptr, d_offsets.ptr, d_states.ptr, n))

        def inject(acc):
            check(L.r0hip_rv32im_bigint_accum_inject(acc.ptr, ROWS, mp, bp, n))

        legs = {"host": host, "device": device, "inject": inject}
        times = {k: [] for k in legs}
        for it in range(args.warmup + args.reps):
            for k, fn in legs.items():  # alternating, so drift hits every leg alike
                t0 = time.perf_counter()
                fn(accum[0])
                dt = (time.perf_counter() - t0) * 1e3
                if it >= args.warmup:
                    times[k].append(dt)
        # the same words from both legs (and from the injection)
        groups = []
        for fn in (host, device, inject):
            check(L.r0hip_memset32(accum[1].ptr, INVALID, 12 * ROWS))
            fn(accum[1])
            groups.append(accum[1].to_numpy())
        assert np.array_equal(groups[0], groups[1]) and np.array_equal(groups[0], groups[2]), n
        row = {"n": n}
        for k, v in times.items():
            row[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        row["host_over_device"] = round(row["host"]["median"] / row["device"]["median"], 2)
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
        for b in (d_states, d_rows, d_index, d_offsets):
            b.free()
    wins = [row["n"] for row in result["sizes"] if row["device"]["median"] <= row["host"]["median"]]
    result["crossover_n"] = min(wins) if wins else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"crossover_n = {result['crossover_n']}; written to {args.out}")


if __name__ == "__main__":
    main()
