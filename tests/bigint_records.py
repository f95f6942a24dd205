"""Back::BigInt record streams for the accumulator-state tests (test infrastructure only).

Everything here returns a NumPy structured array of DTYPE, which is struct r0hip_bigint_back
(28 bytes) and what risc0_amd.bigint_backs takes without a per-record loop. Rows are distinct,
sorted and random in [0, rows).

* `random_stream`: ops uniform over Shift, SetTerm, AddTotal, Carry1, Carry2 (BigIntAccum
  accepts these with any bytes), Reset with a given probability, coeff uniform in [0, 8].
* `valid_stream`: the same with `bigint_accum.program` programs written over it about every
  `every` records. A program starts and ends with Reset, so its EqZero holds whatever
  precedes it. A few hundred programs are made once and reused cyclically.
* the named runs: `shift_only`, `add_total_only`, `set_term_carry2_add_total`,
  `resets_at_boundaries`.
"""
import numpy as np

import bigint_accum as B

DTYPE = np.dtype([("row", "<u4"), ("poly_op", "<u4"), ("coeff", "<u4"), ("bytes", "u1", (16,))])
assert DTYPE.itemsize == 28

_PROGRAMS = None


def with_rows(rng, recs, rows):
    """the records placed on random distinct rows of a segment, in increasing order"""
    n = recs.size
    assert n <= rows
    recs["row"] = np.sort(rng.choice(rows, n, replace=False)) if n else 0
    return recs


def _random(rng, n, p_reset):
    recs = np.zeros(n, DTYPE)
    recs["poly_op"] = rng.integers(B.SHIFT, B.CARRY2 + 1, n)
    recs["poly_op"][rng.random(n) < p_reset] = B.RESET
    recs["coeff"] = rng.integers(0, 9, n)
    recs["bytes"] = rng.integers(0, 256, (n, 16))
    return recs


def random_stream(rng, n, rows, p_reset=1 / 5000):
    return with_rows(rng, _random(rng, n, p_reset), rows)


def programs(count=300):
    """`count` valid BigInt calls (all three kinds) as record arrays, made once"""
    global _PROGRAMS
    if _PROGRAMS is None or len(_PROGRAMS) < count:
        rng = np.random.default_rng(0xB16B16)
        out = []
        for i in range(count):
            prog = B.program(rng, ["add", "mul", "cancel"][i % 3])
            p = np.zeros(len(prog), DTYPE)
            p["poly_op"] = [op for op, _, _ in prog]
            p["coeff"] = [c for _, c, _ in prog]
            p["bytes"] = [by for _, _, by in prog]
            out.append(p)
        _PROGRAMS = out
    return _PROGRAMS[:count]


def valid_stream(rng, n, rows, p_reset=1 / 5000, every=50):
    """random_stream with a valid program over records [pos, pos + len) about every `every`
    records: gaps are uniform in [every / 2, 3 * every / 2], so the EqZero records land at
    every position relative to a tile. The reference accepts the result."""
    recs = _random(rng, n, p_reset)
    progs = programs()
    pos, i = int(rng.integers(0, every)), 0
    while True:
        p = progs[i % len(progs)]
        if pos + p.size > n:
            break
        recs[pos:pos + p.size] = p
        pos += p.size + int(rng.integers(every // 2, 3 * every // 2 + 1))
        i += 1
    return with_rows(rng, recs, rows)


def shift_only(rng, n, rows):
    """poly is multiplied by x^16 n times running: the affine scan's `a` never becomes 0 or 1"""
    recs = _random(rng, n, 0)
    recs["poly_op"] = B.SHIFT
    return with_rows(rng, recs, rows)


def add_total_only(rng, n, rows):
    """total grows at every record, with no clear anywhere"""
    recs = _random(rng, n, 0)
    recs["poly_op"] = B.ADD_TOTAL
    return with_rows(rng, recs, rows)


def set_term_carry2_add_total(rng, n_carry, rows):
    """SetTerm, n_carry Carry2, AddTotal: the term written first is read n_carry + 1 records on"""
    recs = _random(rng, n_carry + 2, 0)
    recs["poly_op"] = B.CARRY2
    recs["poly_op"][0] = B.SET_TERM
    recs["poly_op"][-1] = B.ADD_TOTAL
    return with_rows(rng, recs, rows)


def resets_at_boundaries(rng, n, rows, tiles):
    """no Reset but at every multiple of each tile size in `tiles`, and one record either side"""
    recs = _random(rng, n, 0)
    for t in tiles:
        for d in (-1, 0, 1):
            at = np.arange(t, n, t) + d
            recs["poly_op"][at[(at >= 0) & (at < n)]] = B.RESET
    return with_rows(rng, recs, rows)
