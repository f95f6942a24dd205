"""TEST INFRASTRUCTURE — inputs and CPU references of tests/test_accum_edges_gpu.py, shared with
tests/test_gen_accum_source.py so the generated source is checked on the CPU on the words the
card sees.

Word kinds, as stored Montgomery words (the kinds of test_gpu_op_edges.words):
  random  uniform canonical words
  max     every word p - 1
  mixed   per word one of 0, 1, p - 1, p - 2, the word of 1, the word of -1, or random
Mix kinds: the kind of the rows, or
  holes   random non-zero words with every second FpExt element (1, 3, 5, ...) set to zero: the
          accumulation steps invert sums of mix elements times row words, so a row then hands
          its batch of inverses zero and non-zero inputs together
"""
import functools

import numpy as np

import rv32im_accum_ir as IRI

P = 15 * 2**27 + 1
R_MONT = 2**32 % P       # the stored word of 1
INVALID = 0xFFFFFFFF
EDGE_WORDS = np.array([0, 1, P - 1, P - 2, R_MONT, P - R_MONT], np.uint32)
RV_DATA_COLS, RV_ACCUM_COLS, RV_GLOBAL_WORDS, RV_MIX_WORDS, RV_SPLIT = 211, 103, 90, 36, 23
RV_ARMS = 13             # the selector of arm a is data column 1 + a (test_rv32im_accum_ir.SELECTORS)


def words(rng, n, kind):
    """n stored words of the given kind"""
    if kind == "max":
        return np.full(n, P - 1, np.uint32)
    out = rng.integers(0, P, n, dtype=np.uint32)
    if kind == "random":
        return out
    assert kind == "mixed", kind
    pick = rng.integers(0, EDGE_WORDS.size + 1, n)
    edge = pick < EDGE_WORDS.size
    out[edge] = EDGE_WORDS[pick[edge]]
    return out


def mix_words(rng, n, kind):
    """n mix words (n / 4 FpExt elements): a word kind, or `holes`"""
    if kind != "holes":
        return words(rng, n, kind)
    out = rng.integers(1, P, n, dtype=np.uint32).reshape(-1, 4)
    out[1::2] = 0
    return out.reshape(-1)


def rv_rows(rng, rows, arms, kind):
    """rv32im data group whose row r takes instruction arm arms[r]: words of the kind, then the
    rule of test_rv32im_accum_ir.rows_for_arms (the selectors before the arm zeroed; data
    column 32 zeroed on arm-12 rows), and the row's own selector, where it came out 0, set to
    p - 1"""
    arms = np.asarray(arms)
    assert arms.shape == (rows,) and arms.min() >= 0 and arms.max() < RV_ARMS
    data = words(rng, RV_DATA_COLS * rows, kind).reshape(RV_DATA_COLS, rows)
    for a in range(RV_ARMS):
        at = np.nonzero(arms == a)[0]
        data[1:1 + a, at] = 0
        own = data[1 + a, at]
        data[1 + a, at] = np.where(own == 0, P - 1, own)
        if a == 12:
            data[32, at] = 0
    return data.reshape(-1)


def rv_case(seed, rows, arms, kind, mix_kind):
    """(data, global, mix) of one rv32im case; mix_kind "same" is the kind of the rows"""
    rng = np.random.default_rng(seed)
    data = rv_rows(rng, rows, arms, kind)
    glob = words(rng, RV_GLOBAL_WORDS, kind)
    mix = mix_words(rng, RV_MIX_WORDS, kind if mix_kind == "same" else mix_kind)
    return data, glob, mix


@functools.lru_cache(maxsize=None)
def rv_ops():
    return IRI.load()


def rv_step_reference(data, glob, mix, rows, last, on_inv=None):
    """the accum group after the step alone, from all-INVALID: the numpy IR interpreter"""
    acc = np.full(RV_ACCUM_COLS * rows, INVALID, np.uint32)
    IRI.run(data.copy(), acc, glob, mix, rows, last, ops=rv_ops(), on_inv=on_inv)
    return acc


def rv_reference(oracle, data, glob, mix, rows, last):
    """what r0hip_rv32im_accum must leave: the step, then the oracle's phases 2 and 3"""
    acc = rv_step_reference(data, glob, mix, rows, last)
    oracle.rv32im_accum_finalize(acc, rows, RV_ACCUM_COLS, RV_SPLIT, last)
    return acc


class InverseInputs:
    """on_inv hook of rv32im_accum_ir.run: per row, how many of the inverses its taken blocks
    run saw a zero and how many a non-zero input"""

    def __init__(self, rows):
        self.zero = np.zeros(rows, np.int64)
        self.nonzero = np.zeros(rows, np.int64)
        self.ops = self.ops_with_zero = 0

    def __call__(self, x, live):
        z = live & (x == 0)
        self.zero[:x.size] += z
        self.nonzero[:x.size] += live & (x != 0)
        self.ops += 1
        self.ops_with_zero += bool(z.any())

    def rows_with_both(self):
        return int(((self.zero > 0) & (self.nonzero > 0)).sum())


def recursion_case(seed, oracle, po2, gs, out_size, mix_size, kind, mix_kind):
    """(ctrl, global, data, mix) with accum_ir.synthetic's one-hot control columns (ctrl 1..7
    and 9..17) and every other word of the kind"""
    rng = np.random.default_rng(seed)
    n = 1 << po2
    ctrl = words(rng, gs[1] * n, kind)
    one = oracle.encode(1)
    for cols in (range(1, 8), range(9, 18)):
        cols = list(cols)
        sel = rng.integers(0, len(cols), n)
        for j, c in enumerate(cols):
            ctrl[c * n:(c + 1) * n] = np.where(sel == j, one, 0)
    data = words(rng, gs[2] * n, kind)
    glob = words(rng, out_size, kind)
    mix = mix_words(rng, mix_size, kind if mix_kind == "same" else mix_kind)
    return ctrl, glob, data, mix
