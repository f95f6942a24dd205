"""Extreme eval_check inputs and their reference, shared by the host twin's test
(test_ec_host.py) and the device test (test_gpu_op_edges.py): every buffer word p - 1, or a
mix of 0, 1, 2, p - 2, p - 1, with the numpy IR interpreter (ir_eval.py) times the
1/((3 w^c)^N - 1) factor as the expected check polynomial. Needs no compiled reference."""
import numpy as np

import ir_eval
from test_golden import e_pow, rou_fwd

P = 15 * 2**27 + 1
MODES = ("all_pm1", "edge_mix")


def enc(x):
    """plain integers -> Montgomery words"""
    return np.array([(int(v) % P) * 2**32 % P for v in x], dtype=np.uint32)


def extreme_inputs(d, mode, po2):
    """(plain, poly_mix): plain values per buffer name ("accum", "code", "data", "mix", "global")
    for the circuit description d on the 4 * 2^po2 evaluation domain, and the plain FpExt
    poly_mix that goes with them"""
    D = 4 << po2
    rng = np.random.default_rng(7)
    gs = d["group_sizes"]
    sizes = {"accum": gs[0] * D, "code": gs[1] * D, "data": gs[2] * D, "mix": d["mix_size"],
             "global": d["output_size"]}
    edge = np.array([0, 1, 2, P - 2, P - 1], dtype=np.uint64)
    plain = {}
    for k, n in sizes.items():
        plain[k] = np.full(n, P - 1, np.uint64) if mode == "all_pm1" else rng.choice(edge, size=n)
    poly_mix = (P - 1, P - 1, P - 1, P - 1) if mode == "all_pm1" else (P - 2, 1, P - 1, 2)
    return plain, poly_mix


def reference(circuit, d, plain, poly_mix, po2):
    """the check polynomial on the evaluation domain as plain values, shape (4, 4 * 2^po2):
    poly_fp(cycle) / ((3 w^cycle)^(2^po2) - 1)"""
    D = 4 << po2
    args_plain = [plain[a] for a in d["eval_args"]]
    pows = [e_pow(poly_mix, k) for k in d["poly_mix_powers"]]
    fp = ir_eval.evaluate(ir_eval.load_ir(circuit), args_plain, D, pows)
    w = rou_fwd()[po2 + 2]
    ref = np.zeros((4, D), np.uint64)
    for c in range(D):
        x = 3 * pow(w, c, P) % P
        inv = pow((pow(x, 1 << po2, P) - 1) % P, P - 2, P)
        for k in range(4):
            ref[k, c] = int(fp[k][c]) * inv % P
    return ref
