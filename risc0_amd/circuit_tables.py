"""A circuit's two files, <name>.taps.json and <name>.poly.ir, as the flat tables the library reads.

Both ways of giving the library a circuit go through here: tools/gen_circuits_inc.py writes the
tables into risc0_amd/csrc/gen/circuits.cpp at build time, and risc0_amd.register_circuit hands
them to r0hip_circuit_register while the process runs. No dependency beyond the standard library
(the build imports this file on its own, without the package).
"""
import json

P = 15 * 2**27 + 1
OPS = "celg+-*abr"
ARGS = {"accum": 0, "code": 1, "data": 2, "mix": -1, "global": -2}
GROUPS = {"accum": 0, "code": 1, "data": 2}


def enc(x):
    """The Montgomery word of x mod p (R = 2^32)."""
    return (x % P) * 2**32 % P


def ir_records(d, poly_ir_path):
    """The flattened constraint program as 6-word records {op, dst, a, b, c, d} for the host
    poly_ext (risc0_amd/csrc/verify.cpp) and the device interpreter: constants pre-encoded to
    Montgomery, an `l` as its tap's index, a `g` as {0 mix | 1 global, word}. d: the taps.json."""
    tap_index = {(t[2], t[0], t[1]): i for i, t in enumerate(d["taps"])}
    recs = []
    for line in open(poly_ir_path):
        if line.startswith("#") or not line.strip():
            continue
        t = line.split()
        op, a = t[0], [int(x) for x in t[1:]]
        if op == "c":
            a = [a[0], enc(a[1])]
        elif op == "e":
            a = [a[0]] + [enc(x) for x in a[1:5]]
        elif op == "l":
            a = [a[0], tap_index[(GROUPS[d["eval_args"][a[1]]], a[2], a[3])]]
        elif op == "g":
            a = [a[0], {"mix": 0, "global": 1}[d["eval_args"][a[1]]], a[2]]
        recs.append([OPS.index(op)] + a + [0] * (5 - len(a)))
    return recs


def load(taps_json_path, poly_ir_path):
    """{"name", "taps" (flat), "n_taps", "combo_taps", "combo_begin", "combos_count", "group_begin",
    "n_groups", "group_sizes", "poly_mix_powers", "circuit_info", "mix_size", "output_size",
    "eval_args" (ints), "ir" (flat), "n_ir"} of one circuit."""
    d = json.load(open(taps_json_path))
    recs = ir_records(d, poly_ir_path)
    return {
        "name": d["name"],
        "taps": [x for t in d["taps"] for x in t],
        "n_taps": len(d["taps"]),
        "combo_taps": list(d["combo_taps"]),
        "combo_begin": list(d["combo_begin"]),
        "combos_count": d["combos_count"],
        "group_begin": list(d["group_begin"]),
        "n_groups": len(d["group_names"]),
        "group_sizes": list(d["group_sizes"]),
        "poly_mix_powers": list(d["poly_mix_powers"]),
        "circuit_info": d["circuit_info"],
        "mix_size": d["mix_size"],
        "output_size": d["output_size"],
        "eval_args": [ARGS[a] for a in d["eval_args"]],
        "ir": [x for r in recs for x in r],
        "n_ir": len(recs),
    }
