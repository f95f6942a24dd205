"""The injector in its compact form (include/r0hip.h, r0hip_backs), restated for the tests:
pack() turns a restated trace's Back records (tests/rv32im_trace.py, Trace.backs) into the
records and payload words the C ABI takes, and expand() is build_injector (circuit/rv32im/src/
prove/witgen/mod.rs:226-270, Injector :329-378) over them in numpy, giving the CSR arrays
hal.scatter takes. tests/test_rv32im_backs.py pins expand(pack(t)) to Trace.injector_arrays()."""
import numpy as np

import rv32im_trace as T

ECALL, POSEIDON2, SHA2, BIGINT = 1, 2, 3, 4
WORDS = {ECALL: 3, POSEIDON2: 39, SHA2: 10, BIGINT: 22}
KIND = {"ecall": ECALL, "p2": POSEIDON2, "sha2": SHA2, "bigint": BIGINT}
SHA_FP = ("state_in_addr", "state_out_addr", "data_addr", "count", "k_addr", "round", "next_state")


def payload(back):
    """a Trace back's payload as the reference's array holds it (plain integers)"""
    tag, st = back
    if tag == "ecall":
        return [int(v) for v in st]
    if tag == "p2":  # Poseidon2State::as_array
        return [int(v) for v in st.as_array()]
    if tag == "sha2":  # Sha2State::fp_array, then u32_array (a, e, w)
        return [int(st[k]) for k in SHA_FP] + [int(st["a"]), int(st["e"]), int(st["w"])]
    if tag == "bigint":  # BigIntState::as_array
        return [int(st["is_ecall"]), int(st["mode"]), int(st["pc"]), int(st["poly_op"]), int(st["coeff"])] + \
            [int(b) for b in st["bytes"]] + [int(st["next_state"])]
    raise ValueError(tag)


def pack(trace):
    """(recs, words, inj_rows): recs (n, 3) uint32 rows of (row, kind, index of the payload's
    first word) in row order, words the payloads back to back, inj_rows the trace's cycle count"""
    recs, words = [], []
    for row, back in trace.backs.items():
        p = payload(back)
        assert len(p) == WORDS[KIND[back[0]]]
        recs.append((row, KIND[back[0]], len(words)))
        words += p
    return (np.array(recs, np.uint32).reshape(-1, 3), np.array(words, np.uint32), len(trace.cyc))


def kind_columns(lay, kind):
    """(columns of the plain words, first columns of the bit words) of a record kind"""
    return {ECALL: (lay["ecall_s"], []), POSEIDON2: (lay["poseidon2_state"], []),
            SHA2: (lay["sha2_fp"], lay["sha2_u32"]), BIGINT: (lay["bigint_state"], [])}[kind]


def expand(recs, words, inj_rows, cycles, rows, lay=None):
    """build_injector over the records: (index, offsets, values) as hal.scatter takes them, in
    the reference's push order (per row its Back's entries, then set_cycle's five); index has
    inj_rows + 1 entries, offsets are col * rows + row, values Montgomery words of value % P"""
    lay = lay or T.layout()
    recs = np.asarray(recs, np.uint32).reshape(-1, 3)
    words = np.asarray(words, np.uint32)
    by_row = {int(r): (int(k), int(w)) for r, k, w in recs}
    index, offs, vals = [0], [], []
    for r in range(inj_rows):
        if r in by_row:
            kind, w = by_row[r]
            plain, bits = kind_columns(lay, kind)
            for i, col in enumerate(plain):
                offs.append(col * rows + r)
                vals.append(int(words[w + i]))
            for i, col in enumerate(bits):
                v = int(words[w + len(plain) + i])
                for b in range(32):
                    offs.append((col + b) * rows + r)
                    vals.append((v >> b) & 1)
        pc = int(cycles["pc"][r])
        for col, v in ((lay["cycle"], r), (lay["next_pc_low"], pc & 0xFFFF), (lay["next_pc_high"], pc >> 16),
                       (lay["next_state_0"], int(cycles["state"][r])),
                       (lay["next_machine_mode"], int(cycles["machineMode"][r]))):
            offs.append(col * rows + r)
            vals.append(v)
        index.append(len(offs))
    return (np.array(index, np.uint32), np.array(offs, np.uint32),
            T.encode(np.array(vals, np.uint64)) if vals else np.zeros(0, np.uint32))


def scattered(index, offsets, values, rows, cols=211):
    """hal.scatter of the CSR arrays into an all-INVALID group (column-major words)"""
    data = np.full(cols * rows, T.INVALID, np.uint32)
    data[np.asarray(offsets, np.int64)] = values
    return data


def bigint_records(recs, words):
    """the accumulation's (row, poly_op, coeff, bytes) records of the BigInt payloads"""
    out = []
    for r, k, w in np.asarray(recs, np.uint32).reshape(-1, 3):
        if int(k) == BIGINT:
            p = [int(x) for x in words[int(w):int(w) + 22]]
            out.append((int(r), p[3], p[4], [b & 0xFF for b in p[5:21]]))
    return out
