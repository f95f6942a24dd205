"""Helpers of the constraint-rows tests (test_constraint_rows_host.py, test_constraint_rows_gpu.py):
the taps of a trace row gathered from the witness groups, the reference's compiled poly_fp on
them (oracle.poly_fp_at_taps without its per-call set-up), and a Python restatement of
r0hip_constraint_term's walk as scalar evaluation of the committed <circuit>.poly.ir."""
import ctypes as C
import functools
import json
import os

import numpy as np

import ir_eval

P = 15 * 2**27 + 1
R = 2**32 % P
R_INV = pow(2**32, P - 2, P)
NB = P - 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = {"accum": 0, "code": 1, "data": 2}


@functools.lru_cache(maxsize=None)
def circuit(name):
    with open(os.path.join(ROOT, "risc0_amd", "circuits", name + ".taps.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def program(name):
    return ir_eval.load_ir(name)


def max_back(name):
    return max(t[1] for t in circuit(name)["taps"])


def dec(w):
    return int(w) * R_INV % P


def enc(x):
    return int(x) % P * R % P


# ---- a row's taps -----------------------------------------------------------------------------
def gather_taps(name, groups, po2, rows=None):
    """groups: (accum, code, data) as flat column-major arrays of 2^po2 rows. Returns the tap
    values of every row in `rows` (all rows by default), shape (len(rows), n_taps), tap order:
    tap (offset, back, group) of row r reads groups[group][offset * n + ((r - back) mod n)]"""
    n = 1 << po2
    taps = np.array(circuit(name)["taps"], dtype=np.int64)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    out = np.zeros((rows.size, taps.shape[0]), np.uint32)
    for g in range(3):
        sel = np.nonzero(taps[:, 2] == g)[0]
        idx = taps[sel, 0][None, :] * n + ((rows[:, None] - taps[sel, 1][None, :]) & (n - 1))
        out[:, sel] = np.asarray(groups[g], dtype=np.uint32)[idx]
    return out


def rows_near(name, po2, cells):
    """the rows whose taps can read one of `cells` (row numbers of changed cells): every row
    within the circuit's largest `back` after a cell, wrapping"""
    n = 1 << po2
    out = set()
    for r in cells:
        out.update((r + k) & (n - 1) for k in range(max_back(name) + 1))
    return sorted(out)


# ---- the reference's compiled poly_fp -----------------------------------------------------------
class PolyFp:
    """oracle.poly_fp_at_taps with the circuit description made once: value(taps, mix, glob,
    poly_mix) -> 4 Montgomery words. rows(...) evaluates many rows and reuses the value of a row
    whose taps it has already seen under the same mix, global and poly_mix (poly_fp is a pure
    function of those), so a one-cell change costs only the rows that read the cell."""

    def __init__(self, oracle, name):
        self.o, self.name = oracle, name
        self.c, self.keep, _ = oracle.make_circuit(name)
        self.memo = {}

    def value(self, taps, mix, glob, poly_mix):
        o = self.o
        out = np.zeros(4, np.uint32)
        o._check(o.lib().oracle_poly_fp_at_taps(C.byref(self.c), o.ptr(np.ascontiguousarray(taps, np.uint32)),
                                               o.ptr(np.ascontiguousarray(mix, np.uint32)),
                                               o.ptr(np.ascontiguousarray(glob, np.uint32)),
                                               o.ptr(np.ascontiguousarray(poly_mix, np.uint32)), o.ptr(out)))
        return out

    def rows(self, taps, mix, glob, poly_mix):
        mix, glob, poly_mix = (np.ascontiguousarray(a, np.uint32) for a in (mix, glob, poly_mix))
        key = (mix.tobytes(), glob.tobytes(), poly_mix.tobytes())
        memo = self.memo.setdefault(key, {})
        out = np.zeros((taps.shape[0], 4), np.uint32)
        for i in range(taps.shape[0]):
            k = taps[i].tobytes()
            if k not in memo:
                memo[k] = self.value(taps[i], mix, glob, poly_mix)
            out[i] = memo[k]
        return out


def report_of(values):
    """what r0hip_constraint_rows reports for per-row values of shape (n, 4)"""
    bad = np.nonzero(values.any(axis=1))[0]
    return {"bad_rows": int(bad.size), "first_row": int(bad[0]) if bad.size else None,
            "rows": [int(x) for x in bad[:16]]}


# ---- the term walk, restated ------------------------------------------------------------------
def _emul(a, b):
    a0, a1, a2, a3 = a
    b0, b1, b2, b3 = b
    return ((a0 * b0 + NB * (a1 * b3 + a2 * b2 + a3 * b1)) % P, (a0 * b1 + a1 * b0 + NB * (a2 * b3 + a3 * b2)) % P,
            (a0 * b2 + a1 * b1 + a2 * b0 + NB * a3 * b3) % P, (a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0) % P)


def _ext(v):
    return v if isinstance(v, tuple) else (v, 0, 0, 0)


def _add(a, b):
    if isinstance(a, tuple) or isinstance(b, tuple):
        return tuple((x + y) % P for x, y in zip(_ext(a), _ext(b)))
    return (a + b) % P


def _sub(a, b):
    if isinstance(a, tuple) or isinstance(b, tuple):
        return tuple((x - y) % P for x, y in zip(_ext(a), _ext(b)))
    return (a - b) % P


def _mul(a, b):
    if isinstance(a, tuple) and isinstance(b, tuple):
        return _emul(a, b)
    if isinstance(a, tuple):
        return tuple(x * b % P for x in a)
    if isinstance(b, tuple):
        return tuple(a * y % P for y in b)
    return a * b % P


def _nonzero(v):
    return any(_ext(v))


@functools.lru_cache(maxsize=8)
def _powers(name, poly_mix):
    out = []
    for k in circuit(name)["poly_mix_powers"]:
        v, b, e = (1, 0, 0, 0), poly_mix, k
        while e:
            if e & 1:
                v = _emul(v, b)
            b, e = _emul(b, b), e >> 1
        out.append(v)
    return out


def evaluate_row(name, taps, mix, glob, poly_mix):
    """every value of <name>.poly.ir on one row, as plain integers (Fp) or 4-tuples (FpExt), by
    id, from the row's tap values, mix, global and poly_mix given as Montgomery words; also the
    poly_mix powers and the id the `r` record names"""
    d = circuit(name)
    tap_index = {(t[2], t[0], t[1]): i for i, t in enumerate(d["taps"])}
    args = d["eval_args"]
    pm = _powers(name, tuple(dec(w) for w in poly_mix))
    val = {}
    for ins in program(name):
        op, i = ins[0], ins[1]
        if op == "c":
            val[i] = ins[2] % P
        elif op == "e":
            val[i] = tuple(x % P for x in ins[2:6])
        elif op == "l":
            val[i] = dec(taps[tap_index[(GROUP[args[ins[2]]], ins[3], ins[4])]])
        elif op == "g":
            val[i] = dec((mix if args[ins[2]] == "mix" else glob)[ins[3]])
        elif op == "+":
            val[i] = _add(val[ins[2]], val[ins[3]])
        elif op == "-":
            val[i] = _sub(val[ins[2]], val[ins[3]])
        elif op == "*":
            val[i] = _mul(val[ins[2]], val[ins[3]])
        elif op == "a":
            val[i] = _add(val[ins[2]], _mul(val[ins[3]], pm[ins[4]]))
        elif op == "b":
            val[i] = _add(val[ins[2]], _mul(_mul(val[ins[3]], val[ins[4]]), pm[ins[5]]))
        elif op == "r":
            return val, pm, i
    raise ValueError("no result")


def first_term(name, taps, mix, glob, poly_mix, with_depth=False):
    """The id of the first violated term, or None. The accumulate chain that ends at the `r`
    record's value (an `a`/`b` record's first operand is the link before it) is walked from its
    first link on for the first link whose added amount, x * mix^k (`a`) or x * y * mix^k (`b`),
    is nonzero. For a `b` the walk repeats inside the operand that is itself a chain, and the
    innermost id is the answer. with_depth: also how many `b` blocks the answer sits inside."""
    val, pm, res = evaluate_row(name, taps, mix, glob, poly_mix)
    byid = {ins[1]: ins for ins in program(name) if ins[0] != "r"}

    def is_acc(v):
        return byid[v][0] in "ab"

    def first_link(end):
        chain = []
        v = end
        while is_acc(v):
            chain.append(v)
            v = byid[v][2]
        for v in reversed(chain):
            ins = byid[v]
            add = _mul(val[ins[3]], pm[ins[4]]) if ins[0] == "a" else _mul(_mul(val[ins[3]], val[ins[4]]), pm[ins[5]])
            if _nonzero(add):
                return v
        return None

    term, depth = first_link(res), 0
    while term is not None and byid[term][0] == "b":
        ins = byid[term]
        inner = first_link(ins[3]) if is_acc(ins[3]) else (first_link(ins[4]) if is_acc(ins[4]) else None)
        if inner is None:
            break
        term, depth = inner, depth + 1
    return (term, depth) if with_depth else term


# ---- witnesses the tests share ------------------------------------------------------------------
def recursion_witness(seed, po2, mix_seed):
    """RP.satisfying_witness with the reference's accumulation under a fixed mix: a dict with the
    groups (accum, code, data), glob, mix (Montgomery words) and the witness dict itself"""
    import recursion_program as RP
    w = RP.satisfying_witness(seed, po2)
    mix = (np.random.default_rng(mix_seed).integers(1, P, 20, dtype=np.uint64)).astype(np.uint32)
    acc = RP.accumulate(w, mix, po2)
    return {"groups": (acc, w["ctrl"], w["data"]), "glob": w["glob"], "mix": mix, "w": w}


def rv32im_witness_host(po2, cycles, seed, mix_seed):
    """the smallest trace the builders make, through the reference's compiled witness generator
    and accumulation on the CPU: groups (accum, code, data), glob, mix"""
    import bigint_accum as BA
    import rv32im_accum_ref as RA
    import rv32im_trace as T
    import rv32im_witgen_ref as W
    t = T.random_trace(po2, cycles, seed=seed)
    n = 1 << po2
    d, g = W.witgen(t)
    d = np.where(d == W.INVALID, 0, d).astype(np.uint32)
    g = np.where(g == W.INVALID, 0, g).astype(np.uint32)
    mix = (np.random.default_rng(mix_seed).integers(1, P, 36, dtype=np.uint64)).astype(np.uint32)
    init = None
    if t.bigint_records():
        init = BA.inject(np.full(RA.ACCUM_COLS * n, W.INVALID, np.uint32), n, mix, t.bigint_records())
    acc = RA.accum(d, g, mix, n, n, accum_init=init)
    acc = np.where(acc == W.INVALID, 0, acc).astype(np.uint32)
    return {"groups": (acc, np.zeros(n, np.uint32), d), "glob": g, "mix": mix, "trace": t}
