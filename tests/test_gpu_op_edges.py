"""Op-level GPU parity at every kernel variant and at worst-case field values.

test_gpu_parity.py compares every HAL op with the CPU oracle on uniformly random words at a
few sizes per op. This module closes two gaps that leaves, with the same bar (np.array_equal
on the u32 words against oracle/oracle.py; no oracle/_ref needed, nothing here skips):

1. Sizes that pick other kernels. ntt.hip instantiates a row pass per B = 1..13 bits and per
   expand_bits 0..3, and column passes of B = 1..9 bits (plan(L): L <= 13 is one row pass of
   B = L; L = 14..22 adds one column pass of B = L - 13; L = 23..26 two of 5+5, 6+5, 6+6,
   7+6). Forward L = 2..26 at expand_bits 2 launches row (B, EB) = (2..13, 2) and column
   B = 1..9 (tiny branch B < 3, 32 columns B = 3..7, 16 columns and col_block B = 8, 9);
   expand_bits 0, 1, 3 at L = eb, eb + 1, 5, 13, 14 add row (B, EB) = (1, 0), (5, 0), (13, 0),
   (1, 1), (2, 1), (5, 1), (13, 1), (3, 3), (4, 3), (5, 3), (13, 3), with (2, 2) and (3, 3) the
   replicate branch (EB >= B). Inverse L = 1..24 launches row B = 1..13 (the normalising last
   pass) and column B = 1..9. eltwise.hip: batch_evaluate_any below one 4096-coefficient piece,
   at a ragged piece, with empty waves in a chunk and with two chunks; mix_poly_coeffs with
   lanes past `count` and every segment length mod 4 and mod 3; synthetic division on the
   serial path, with a one-lane last block and with more than 256 blocks.

2. Stored words at the bounds the lazy arithmetic relies on. mix_kernel and eval_chunk_kernel
   add raw 64-bit products and fold every 3 / every 4 of them; uniform random words sit a
   factor ~4 below the stated bounds (2^60 + k p^2 < 2^64), so a fold cadence off by one or
   two passes on random inputs. Input kinds, as stored Montgomery words:
     random  uniform canonical words
     zero    all 0
     max     every word p - 1
     mixed   per word one of 0, 1, p - 1, p - 2, the word of 1, the word of -1, or random
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 15 * 2**27 + 1
R_MONT = 2**32 % P       # the stored word of 1 (oracle.encode(1))
EDGE_WORDS = np.array([0, 1, P - 1, P - 2, R_MONT, P - R_MONT], np.uint32)


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def words(oracle, rng, n, kind):
    """n stored words of the given kind (module docstring)"""
    if kind == "random":
        return oracle.rand_elems(rng, n)
    if kind in ("zero", "max"):
        return np.full(n, {"zero": 0, "max": P - 1}[kind], np.uint32)
    assert kind == "mixed", kind
    pick = rng.integers(0, EDGE_WORDS.size + 1, n)
    out = oracle.rand_elems(rng, n)
    edge = pick < EDGE_WORDS.size
    out[edge] = EDGE_WORDS[pick[edge]]
    return out


def ext_one(oracle):
    return np.array([oracle.encode(1), 0, 0, 0], np.uint32)


def ext_max():
    return np.full(4, P - 1, np.uint32)


def ntt_cases(lo, hi, extra_at=(9, 13, 14, 15, 21), extra=("max", "mixed")):
    """(lg, count, kind): every lg in [lo, hi] on random words, 3 polynomials up to lg 16
    (ragged row-pass workgroups) and 1 above; the extra kinds at the sizes around the row /
    column pass boundary and at one deep column pass"""
    out = []
    for lg in range(lo, hi + 1):
        count = 3 if lg <= 16 else 1
        out.append((lg, count, "random"))
        if lg in extra_at:
            out += [(lg, count, k) for k in extra]
    return out


def test_constants(oracle):
    assert P == oracle.P and R_MONT == int(oracle.encode(1))


# ---- A. NTT -----------------------------------------------------------------------------------
def check_expand_evaluate(hal, oracle, lg_out, count, expand_bits, kind):
    rng = np.random.default_rng(1000 * expand_bits + lg_out)
    a = words(oracle, rng, count << (lg_out - expand_bits), kind)
    out = hal.alloc_elem("out", count << lg_out)
    src = hal.copy_from_elem("in", a)
    hal.batch_expand_into_evaluate_ntt(out, src, count, expand_bits)
    got = out.to_numpy()
    out.free()
    src.free()
    ref = np.zeros(count << lg_out, np.uint32)
    oracle.batch_expand_into_evaluate_ntt(ref, a, count, expand_bits)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("lg_out,count,kind", ntt_cases(2, 26))
def test_expand_evaluate_every_size(hal, oracle, lg_out, count, kind):
    """expand_bits = 2 at every output size 2^2 .. 2^26: every row pass B = 2..13, every
    column pass B = 1..9 and all four two-column-pass plans (L = 23..26, the evaluation
    domains of po2 21..24 segments; the two largest cases of this file, about 5 s of oracle
    at L = 26)"""
    check_expand_evaluate(hal, oracle, lg_out, count, 2, kind)


@pytest.mark.parametrize("expand_bits,lg_out", [(eb, lg) for eb in (0, 1, 3) for lg in sorted({eb, eb + 1, 5, 13, 14})]
                         + [(2, 2)])
def test_expand_evaluate_every_expand_form(hal, oracle, expand_bits, lg_out):
    """expand_bits 0, 1 and 3 (2 is above) from the smallest size each allows: lg_out == eb is
    one input word per polynomial, and EB >= B stages the replicated words instead of the
    compact input (lg_out 3 at eb 3, lg_out 2 at eb 2)"""
    check_expand_evaluate(hal, oracle, lg_out, 3, expand_bits, "random")


def test_expand_bits_4_is_an_error(hal, oracle):
    import risc0_amd as r
    a = words(oracle, np.random.default_rng(4), 3 << 2, "random")
    out = hal.alloc_elem("out", 3 << 6)
    with pytest.raises(r.R0HipError):
        hal.batch_expand_into_evaluate_ntt(out, hal.copy_from_elem("in", a), 3, 4)
    # reported, not fatal: the same HAL still transforms
    check_expand_evaluate(hal, oracle, 6, 3, 2, "random")


@pytest.mark.parametrize("lg,count,kind", ntt_cases(1, 24))
def test_interpolate_every_size(hal, oracle, lg, count, kind):
    """every size 2^1 .. 2^24: the normalising row pass at B = 1..13 and the inverse column
    passes B = 1..9 (post-scaled stores), two of them at L = 23, 24"""
    a = words(oracle, np.random.default_rng(2000 + lg), count << lg, kind)
    d = hal.copy_from_elem("io", a)
    hal.batch_interpolate_ntt(d, count)
    got = d.to_numpy()
    d.free()
    oracle.batch_interpolate_ntt(a, count)
    assert np.array_equal(got, a)


@pytest.mark.parametrize("kind", ["random", "max"])
@pytest.mark.parametrize("lg", range(1, 23))
def test_zk_shift_every_size(hal, oracle, lg, kind):
    count = 3 if lg <= 16 else 1
    a = words(oracle, np.random.default_rng(3000 + lg), count << lg, kind)
    d = hal.copy_from_elem("io", a)
    hal.zk_shift(d, count)
    oracle.zk_shift(a, count)
    assert np.array_equal(d.to_numpy(), a)


@pytest.mark.parametrize("lg", range(1, 23))
def test_bit_reverse_every_size(hal, oracle, lg):
    count = 3 if lg <= 16 else 1
    a = words(oracle, np.random.default_rng(4000 + lg), count << lg, "random")
    d = hal.copy_from_elem("io", a)
    hal.batch_bit_reverse(d, count)
    oracle.batch_bit_reverse(a, count)
    assert np.array_equal(d.to_numpy(), a)


# ---- B. mix_poly_coeffs -----------------------------------------------------------------------
MIX_ROWS = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 13}  # combo id -> rows; id 5 unused


@pytest.mark.parametrize("mix_kind", ["worst", "random"])
@pytest.mark.parametrize("kind", ["random", "max", "mixed"])
@pytest.mark.parametrize("count", [1, 255, 257, 4096])
def test_mix_poly_coeffs_segments(hal, oracle, count, kind, mix_kind):
    """Combo ids interleaved, id 5 unused (its output chunk must stay as it was), segment
    lengths 1..9 and 13: every remainder of the 4-loads-in-flight loop and of the fold-every-3
    counter; counts off the 256-lane block. "worst": mix = 1 and mix_start = four words p - 1,
    so every power word the kernel multiplies by is p - 1; with `max` inputs every product is
    (p - 1)^2 and each 64-bit sum runs at the bound stated in mix_kernel. "random" mix and
    mix_start are drawn uniformly."""
    rng = np.random.default_rng(5000 + count)
    combos = rng.permutation(np.repeat(list(MIX_ROWS), list(MIX_ROWS.values()))).astype(np.uint32)
    input_size, chunks = combos.size, max(MIX_ROWS) + 1
    inp = words(oracle, rng, input_size * count, kind)
    init = words(oracle, rng, 4 * count * chunks, kind)
    if mix_kind == "worst":
        start, mix = ext_max(), ext_one(oracle)
    else:
        start, mix = oracle.rand_elems(rng, 4), oracle.rand_elems(rng, 4)
    out = hal.copy_from_extelem("out", init)
    hal.mix_poly_coeffs(out, start, mix, hal.copy_from_elem("in", inp), combos, input_size, count)
    ref = init.copy()
    oracle.mix_poly_coeffs(ref, start, mix, inp, combos, input_size, count)
    got = out.to_numpy()
    assert np.array_equal(got.reshape(chunks, -1)[5], init.reshape(chunks, -1)[5])
    assert np.array_equal(got, ref)


# ---- C. batch_evaluate_any --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zero", "max"])
@pytest.mark.parametrize("log_n", [2, 6, 8, 11, 13, 14, 15])
def test_batch_evaluate_any_pieces(hal, oracle, log_n, kind):
    """n = 4 .. 2048 is a ragged first piece (lanes past n read as 0), 8192 leaves waves 2 and
    3 of the chunk empty, 16384 fills it, 32768 is two chunks combined by Horner. 9 evaluations
    of 3 polynomials with repeated `which`, at five random points and at 0, 1, -1 and the point
    whose four words are p - 1. The table words eval_chunk_kernel multiplies by are powers of
    x and cannot all be forced to p - 1: `max` coefficients against several random x is the
    tightest reachable case for its 64-bit sums (folded every 4 products)."""
    rng = np.random.default_rng(6000 + log_n)
    poly_count = 3
    coeffs = words(oracle, rng, poly_count << log_n, kind)
    which = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1], np.uint32)
    one = ext_one(oracle)
    xs = np.concatenate([oracle.rand_elems(rng, 4 * 5), np.zeros(4, np.uint32), one,
                         np.array([P - one[0], 0, 0, 0], np.uint32), ext_max()]).astype(np.uint32)
    out = hal.alloc_extelem("out", which.size)
    hal.batch_evaluate_any(hal.copy_from_elem("coeffs", coeffs), poly_count, hal.copy_from_elem("which", which),
                           hal.copy_from_extelem("xs", xs), out)
    ref = np.zeros(4 * which.size, np.uint32)
    oracle.batch_evaluate_any(coeffs, poly_count, which, xs, ref)
    assert np.array_equal(out.to_numpy(), ref)


# ---- D. division and the small ops ------------------------------------------------------------
@pytest.mark.parametrize("zkind", ["random", "zero", "one"])
@pytest.mark.parametrize("kind", ["random", "max"])
@pytest.mark.parametrize("cycles", [16, 24, 48, 4112, 1 << 21])
def test_combos_divide_single_chunk(hal, oracle, cycles, kind, zkind):
    """One row divided by (x - z): 16 is one lane, 24 the serial path (not a multiple of 16),
    48 three lanes, 4112 = 16 * 257 a second block with one lane, 2^21 is 512 blocks, so
    div_top_kernel carries across two segments. Words and the bad-chunk index both match."""
    rng = np.random.default_rng(7000 + cycles)
    combos = words(oracle, rng, 4 * cycles, kind)
    z = {"random": oracle.rand_elems(rng, 4), "zero": np.zeros(4, np.uint32), "one": ext_one(oracle)}[zkind]
    begin = np.array([0, 1], np.uint32)
    d = hal.copy_from_extelem("combos", combos)
    bad_gpu = hal.combos_divide(d, z, begin, cycles)
    got = d.to_numpy()
    d.free()
    bad_ref = oracle.combos_divide(combos, z, begin, cycles)
    assert bad_gpu == bad_ref
    assert np.array_equal(got, combos)


@pytest.mark.parametrize("kind", ["max", "mixed"])
@pytest.mark.parametrize("cycles", [8, 1024])
def test_combos_prepare_extreme(hal, oracle, cycles, kind):
    rng = np.random.default_rng(7100 + cycles)
    combos_count = 4
    reg_sizes = np.array([1, 2, 3, 2, 1, 6, 1], np.uint32)
    reg_ids = np.array([0, 1, 2, 3, 0, 2, 1], np.uint32)
    mix = words(oracle, rng, 4, kind)
    coeff_u = words(oracle, rng, 4 * (int(reg_sizes.sum()) + 16), kind)
    combos = words(oracle, rng, 4 * cycles * (combos_count + 1), kind)
    d = hal.copy_from_extelem("combos", combos)
    hal.combos_prepare(d, coeff_u, combos_count, cycles, reg_sizes, reg_ids, mix)
    oracle.combos_prepare(combos, coeff_u, combos_count, cycles, reg_sizes, reg_ids, mix)
    assert np.array_equal(d.to_numpy(), combos)


@pytest.mark.parametrize("count", [1, 257])
def test_fri_fold_max(hal, oracle, count):
    inp = words(oracle, None, count * 4 * 16, "max")
    out = hal.alloc_elem("out", count * 4)
    hal.fri_fold(out, hal.copy_from_elem("in", inp), ext_max())
    ref = np.zeros(count * 4, np.uint32)
    oracle.fri_fold(ref, inp, ext_max())
    assert np.array_equal(out.to_numpy(), ref)


@pytest.mark.parametrize("to_add", [1, 3])
@pytest.mark.parametrize("count", [1, 257])
def test_eltwise_sum_extelem_max(hal, oracle, count, to_add):
    inp = words(oracle, None, 4 * count * to_add, "max")
    out = hal.alloc_elem("out", 4 * count)
    hal.eltwise_sum_extelem(out, hal.copy_from_extelem("in", inp))
    ref = np.zeros(4 * count, np.uint32)
    oracle.eltwise_sum_extelem(ref, inp)
    assert np.array_equal(out.to_numpy(), ref)


def test_eltwise_add_elem_wraps(hal, oracle):
    """a + b == p exactly (the sum that must come back as 0, not p), its neighbours p - 1 and
    p + 1, and p - 1 plus p - 1"""
    rng = np.random.default_rng(7200)
    n = 257
    a = rng.integers(2, P - 1, 4 * n, dtype=np.uint64)
    total = np.repeat(np.array([P, P - 1, P + 1, 0], np.uint64), n)
    b = total - a
    a[3 * n:] = b[3 * n:] = P - 1
    a, b = a.astype(np.uint32), b.astype(np.uint32)
    assert a.max() < P and b.max() < P and np.all(a[:n].astype(np.uint64) + b[:n] == P)
    o = hal.alloc_elem("o", a.size)
    hal.eltwise_add_elem(o, hal.copy_from_elem("a", a), hal.copy_from_elem("b", b))
    ref = np.zeros(a.size, np.uint32)
    oracle.eltwise_add_elem(ref, a, b)
    assert np.all(ref[:n] == 0)
    assert np.array_equal(o.to_numpy(), ref)


@pytest.mark.parametrize("kind", ["max", "zero_mid"])
@pytest.mark.parametrize("n", [1, 2, 300])
def test_prefix_products_extreme(hal, oracle, n, kind):
    rng = np.random.default_rng(7300 + n)
    if kind == "max":
        io = words(oracle, rng, 4 * n, "max")
    else:  # a zero element in the middle: everything from there on is zero
        io = words(oracle, rng, 4 * n, "random")
        io[4 * (n // 2): 4 * (n // 2) + 4] = 0
    d = hal.copy_from_extelem("io", io)
    hal.prefix_products(d)
    oracle.prefix_products(io)
    assert np.array_equal(d.to_numpy(), io)


SUITE_IDS = {"sha-256": 1, "poseidon_254": 2}  # oracle.SHA256, oracle.POSEIDON254


@functools.lru_cache(maxsize=None)
def suite_hal(suite):
    import risc0_amd as r
    return r.HipHal(suite)


@pytest.mark.parametrize("kind", ["zero", "max", "mixed"])
@pytest.mark.parametrize("cols", [1, 16, 17])
@pytest.mark.parametrize("suite", ["sha-256", "poseidon_254"])
def test_hash_rows_extreme(oracle, suite, cols, kind):
    """the shape of test_p2_partial_gpu.test_hash_rows (which covers Poseidon2) for the other
    two suites: five waves and a ragged one; one block, a full block, a block and a word"""
    rows = 321
    h = suite_hal(suite)
    m = words(oracle, np.random.default_rng(cols * 7 + len(kind)), rows * cols, kind)
    out = h.alloc_digest("out", rows)
    h.hash_rows(out, h.copy_from_elem("m", m))
    ref = np.zeros(rows * 8, np.uint32)
    oracle.hash_rows(SUITE_IDS[suite], ref, m)
    assert np.array_equal(out.to_numpy(), ref)


def test_hash_fold_poseidon254_extreme_digests(oracle):
    """digests are canonical BN254 Fr values: 0, r - 1 and random values below r, in every
    left / right pairing"""
    import p254_ref
    assert (oracle.SHA256, oracle.POSEIDON254) == (SUITE_IDS["sha-256"], SUITE_IDS["poseidon_254"])
    h = suite_hal("poseidon_254")
    rng = np.random.default_rng(7400)
    outputs = 99
    vals = []
    for i in range(outputs * 2):
        pick = (i // 2 % 3, i // 6 % 3)[i % 2]  # (left, right) runs over all 9 pairs of kinds
        rand = int.from_bytes(rng.bytes(40), "little") % p254_ref.MOD
        vals.append([0, p254_ref.MOD - 1, rand][pick])
    io = np.zeros(outputs * 4 * 8, np.uint32)
    io[outputs * 2 * 8:] = np.array([p254_ref.to_words(v) for v in vals], np.uint32).reshape(-1)
    d = h.copy_from_digest("io", io)
    h.hash_fold(d, outputs * 2, outputs)
    oracle.hash_fold(oracle.POSEIDON254, io, outputs * 2, outputs)
    assert np.array_equal(d.to_numpy(), io)


# ---- E. eval_check on the device at extreme inputs ----------------------------------------------
_EC_CASES = {}


def ec_extreme_case(oracle, circuit, mode, po2):
    """(Montgomery words per buffer name, poly_mix words, expected check words), computed once
    per case and shared by both tap forms"""
    import ec_extreme as X
    if (circuit, mode, po2) not in _EC_CASES:
        d = oracle.load_circuit_json(circuit)
        plain, poly_mix = X.extreme_inputs(d, mode, po2)
        ref = X.reference(circuit, d, plain, poly_mix, po2)
        _EC_CASES[circuit, mode, po2] = ({k: X.enc(v) for k, v in plain.items()}, X.enc(poly_mix),
                                         X.enc(ref.reshape(-1)))
    return _EC_CASES[circuit, mode, po2]


@pytest.mark.parametrize("wide", ["0", "0xffffffff"])
@pytest.mark.parametrize("mode", ["all_pm1", "edge_mix"])
@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
def test_eval_check_extreme_inputs(hal, oracle, circuit, mode, wide, monkeypatch):
    """The device eval_check kernels, in both tap forms, on the inputs of
    test_ec_host.test_generated_eval_check_extreme_inputs (every word p - 1; mixes of 0, 1, 2,
    p - 2, p - 1) against the numpy IR interpreter times 1/((3 w^c)^N - 1)."""
    monkeypatch.setenv("R0_EC_WIDE", wide)
    po2 = 5
    D = 4 << po2
    bufs, pm, ref = ec_extreme_case(oracle, circuit, mode, po2)
    out = hal.alloc_elem("check", 4 * D)
    hal.eval_check(circuit, out, [hal.copy_from_elem(k, bufs[k]) for k in ("accum", "code", "data")],
                   hal.copy_from_elem("mix", bufs["mix"]), hal.copy_from_elem("global", bufs["global"]), pm, po2)
    assert np.array_equal(out.to_numpy(), ref)
