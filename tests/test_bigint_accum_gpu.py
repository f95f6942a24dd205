"""rv32im BigInt accumulator states from the device's parallel scans
(risc0_amd/csrc/bigint_accum.hip, r0hip_rv32im_bigint_accum_states_device) against the serial
host function (r0hip_rv32im_bigint_accum_states), which tests/test_bigint_accum.py pins to the
Python restatement and to the compiled reference: the same words, the same error texts, and
the same seals through every prover that injects the states.

Tile sizes this file relies on (bigint_accum.hip): a lane takes LANE = 16 consecutive records,
a wave 64 lanes (WAVE records), a workgroup 256 lanes (TILE records); one workgroup scans the
tile sums 256 at a time, so 2^20 records are the most one such pass covers.
"""
import functools

import numpy as np
import pytest

import bigint_accum as B
import bigint_records as G
import rv32im_accum_ref as R

pytestmark = pytest.mark.gpu

LANE, WAVE, TILE = 16, 1024, 4096
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 65537, (1 << 20) + 1]


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def _mix(rng):
    return rng.integers(0, B.P, R.MIX_WORDS, dtype=np.uint64).astype(np.uint32)


def _rows_for(n):
    return 1 << 21 if n > 1 << 17 else 1 << 17


@functools.lru_cache(maxsize=None)
def _stream(n):
    """(mix, records, rows, host states) of the valid stream of n records; made once, not changed"""
    import risc0_amd as r
    rng = np.random.default_rng(0xACC0 + n)
    mix, rows = _mix(rng), _rows_for(n)
    recs = G.valid_stream(rng, n, rows)
    want = r.bigint_accum_states(mix, recs, rows)
    for a in (mix, recs, want):
        a.setflags(write=False)
    return mix, recs, rows, want


def _tuples(recs):
    return [(int(x["row"]), int(x["poly_op"]), int(x["coeff"]), [int(b) for b in x["bytes"]]) for x in recs]


def _same(hal, mix, recs, rows, want=None):
    import risc0_amd as r
    if want is None:
        want = r.bigint_accum_states(mix, recs, rows)
    got = r.bigint_accum_states_device(hal, mix, recs, rows)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(recs)} states differ, first at record {bad[0]}"
    return want


@pytest.mark.parametrize("n", SIZES)
def test_states_match_host(hal, n):
    """Bit for bit at every size where the scans take another path: below, at and above a wave
    of lanes, a tile, and (2^20 + 1) one record more than one pass over the tile sums covers.
    Reset has probability 1/5000, so poly, term and total all carry across many tiles; a
    valid program about every 50 records puts EqZero at every position relative to a tile."""
    mix, recs, rows, want = _stream(n)
    if n > 2 * TILE:
        ops = recs["poly_op"]
        assert (ops == B.EQ_ZERO).sum() > n // 100 and (ops == B.RESET).sum() < n // 10
    _same(hal, mix, recs, rows, want)
    if 0 < n <= 257:
        assert np.array_equal(want, B.states(mix, _tuples(recs)))


RUNS = {
    # no program and so hardly a Reset: poly, term and total carry across every tile boundary
    "random_without_programs": lambda rng: G.random_stream(rng, 5 * TILE + 3, 1 << 17),
    "shift_only": lambda rng: G.shift_only(rng, 10000, 1 << 17),
    "add_total_only": lambda rng: G.add_total_only(rng, 2 * TILE + 77, 1 << 17),
    "set_term_carry2_add_total": lambda rng: G.set_term_carry2_add_total(rng, 3 * TILE + 5, 1 << 17),
    "resets_at_tile_boundaries": lambda rng: G.resets_at_boundaries(rng, 3 * TILE + 5, 1 << 17, (WAVE, TILE)),
    "resets_at_lane_boundaries": lambda rng: G.resets_at_boundaries(rng, TILE + 5, 1 << 17, (LANE,)),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_named_runs_match_host(hal, name):
    rng = np.random.default_rng(0xAD7)
    mix = _mix(rng)
    _same(hal, mix, RUNS[name](rng), 1 << 17)


@pytest.mark.parametrize("kind", ["shift_only", "mixed"])
def test_worst_case_words(hal, kind):
    """Every mix word p - 1, every byte 255, coeff 0 and 8 (the ends of its range), over
    TILE + 1 records: the largest operands the field code sees, across a tile boundary."""
    rng = np.random.default_rng(0xFFFF)
    mix = np.full(R.MIX_WORDS, B.P - 1, np.uint32)
    n, rows = TILE + 1, 1 << 17
    recs = G.shift_only(rng, n, rows) if kind == "shift_only" else G.random_stream(rng, n, rows)
    recs["bytes"] = 255
    recs["coeff"] = np.where(np.arange(n) % 2, 8, 0)
    _same(hal, mix, recs, rows)


def _message(fn):
    import risc0_amd as r
    with pytest.raises(r.R0HipError) as e:
        fn()
    return str(e.value)


def _corrupt(recs, *eqz):
    bad = recs.copy()
    for k in eqz:
        assert bad["poly_op"][k] == B.EQ_ZERO
        bad["bytes"][k, 0] ^= 1  # the integer identity no longer holds
    return bad


def _error_cases():
    mix, recs, rows, _ = _stream(2 * TILE + 1000)
    eqz = np.nonzero(recs["poly_op"] == B.EQ_ZERO)[0]
    e1 = int(eqz[eqz > TILE + 100][0])    # in the second tile
    e2 = int(eqz[eqz > 2 * TILE + 100][0])  # in the third
    cases = {}
    cases["one_eqz"] = (_corrupt(recs, e1), rows, f"(row {recs['row'][e1]})")
    cases["two_eqz"] = (_corrupt(recs, e2, e1), rows, f"(row {recs['row'][e1]})")
    bad = _corrupt(recs, e1)
    bad["poly_op"][e1 + 300] = 7
    cases["op_after_eqz"] = (bad, rows, "Invalid eqz")
    bad = _corrupt(recs, e2)
    bad["poly_op"][e1 + 300] = 9
    cases["op_before_eqz"] = (bad, rows, "invalid poly_op 9")
    bad = recs.copy()
    bad["row"][[TILE + 7, TILE + 8]] = bad["row"][[TILE + 8, TILE + 7]]
    cases["rows_out_of_order"] = (bad, rows, "increasing row order")
    cases["row_outside"] = (recs.copy(), int(recs["row"][-1]), "outside the segment")
    return mix, cases


@pytest.mark.parametrize("case", ["one_eqz", "two_eqz", "op_after_eqz", "op_before_eqz", "rows_out_of_order",
                                  "row_outside"])
def test_errors_match_host(hal, case):
    """The device path fails with the host function's text, row number included, at the
    earliest record in trace order that fails any check; the library stays usable."""
    import risc0_amd as r
    mix, cases = _error_cases()
    bad, rows, expect = cases[case]
    want = _message(lambda: r.bigint_accum_states(mix, bad, rows))
    assert expect in want
    got = _message(lambda: r.bigint_accum_states_device(hal, mix, bad, rows))
    assert got == want
    _same(hal, *_stream(2 * TILE + 1000))


def test_inject_matches_host_scatter(hal):
    """r0hip_rv32im_bigint_accum_inject with 70 000 records into an INVALID-filled 12-column
    group of 2^17 rows: the host states in each record's row, INVALID everywhere else."""
    import risc0_amd as r
    rows, n = 1 << 17, 70000
    rng = np.random.default_rng(0x1EC7)
    mix = _mix(rng)
    recs = G.valid_stream(rng, n, rows)
    want = np.full((12, rows), R.INVALID, np.uint32)
    want[:, recs["row"]] = r.bigint_accum_states(mix, recs, rows).T
    acc = hal.alloc_elem_init("accum", 12 * rows, int(R.INVALID))
    r.bigint_accum_inject(acc, rows, mix, recs)
    got = acc.to_numpy().reshape(12, rows)
    assert np.array_equal(got, want), int((got != want).sum())
    untouched = np.ones(rows, bool)
    untouched[recs["row"]] = False
    assert (got[:, untouched] == R.INVALID).all()


def test_prove_segment_accum_full_of_bigint_matches_reference(hal, oracle):
    """r0hip_prove_segment_accum at po2 12 with BigInt calls until the rows are full: the seal
    and mix equal the oracle prover's on the group the compiled reference accumulates from the
    reference's injected states."""
    import risc0_amd as r
    if oracle.ref_lib() is None or not R.available():
        pytest.skip("oracle/_ref not built")
    po2 = 12
    n = 1 << po2
    d = oracle.load_circuit_json("rv32im")
    rng = np.random.default_rng(0xB2 + po2)
    data, recs = B.lay_out(rng, n, 10 * n)  # more calls than fit: stops when the rows are full
    assert len(recs) > n // 2
    code = oracle.rand_elems(rng, d["group_sizes"][1] * n)
    glob = oracle.rand_elems(rng, d["output_size"])
    acc0 = np.full(d["group_sizes"][0] * n, R.INVALID, np.uint32)
    dev = lambda a: hal.copy_from_elem("x", a)
    dacc = dev(acc0)
    seal, mix = r.prove_segment_accum(hal, "rv32im", po2, dev(code), dev(data), dacc, n, dev(glob), version=2,
                                      bigint=recs)
    glob_z = np.where(glob == R.INVALID, 0, glob).astype(np.uint32)
    ref_acc = R.accum(data, glob_z, mix, n, n, accum_init=B.inject(acc0.copy(), n, mix, recs))
    ref_acc = np.where(ref_acc == R.INVALID, 0, ref_acc).astype(np.uint32)
    got = dacc.to_numpy()
    assert np.array_equal(got, ref_acc), int((got != ref_acc).sum())
    ref_seal, ref_mix, _ = oracle.prove_segment("rv32im", oracle.POSEIDON2, po2, code, data, ref_acc, glob, version=2)
    assert np.array_equal(mix, ref_mix)
    assert np.array_equal(seal, ref_seal)


_JOBS = {}


def _full_job(oracle, i, po2=14):
    """(code, data, None, glob, records) of a po2 14 segment filled with BigInt calls; made once"""
    if i not in _JOBS:
        n = 1 << po2
        d = oracle.load_circuit_json("rv32im")
        rng = np.random.default_rng(0x714E + i)
        data, recs = B.lay_out(rng, n, 10 * n)
        assert len(recs) > 12000
        _JOBS[i] = (oracle.rand_elems(rng, d["group_sizes"][1] * n), data, None,
                    oracle.rand_elems(rng, d["output_size"]), recs)
    return _JOBS[i]


def _prove(hal, oracle, job, recs, po2=14):
    import risc0_amd as r
    n = 1 << po2
    code, data, _, glob, _ = job
    dev = lambda a: hal.copy_from_elem("x", a)
    dacc = dev(np.full(oracle.load_circuit_json("rv32im")["group_sizes"][0] * n, R.INVALID, np.uint32))
    return r.prove_segment_accum(hal, "rv32im", po2, dev(code), dev(data), dacc, n, dev(glob), version=2, bigint=recs)


def test_prove_segments_full_of_bigint_matches_fused(hal, oracle):
    """The segment pipeline with two provers in flight, three po2 14 jobs filled with BigInt
    calls (about 15 k records each, so each prover's scan scratch is in use beside the
    other's): every seal and mix equals r0hip_prove_segment_accum's on the same job."""
    import risc0_amd as r
    jobs = [_full_job(oracle, i) for i in range(3)]
    want = [_prove(hal, oracle, job, job[4]) for job in jobs]
    got = r.prove_segments(hal, "rv32im", 14, jobs, version=2, in_flight=2)
    for (s1, m1), (s2, m2) in zip(got, want):
        assert np.array_equal(m1, m2)
        assert np.array_equal(s1, s2)


def test_prove_segment_accum_rejects_invalid_eqz_on_the_device_path(hal, oracle):
    """With enough records for the prover to take the device path, a failing EqZero in the
    third tile stops the proof with the reference's error and its row, before any seal; the
    library stays usable, and the valid records prove as before."""
    import risc0_amd as r
    job = _full_job(oracle, 0)
    recs = [[row, op, c, list(by)] for row, op, c, by in job[4]]
    eqz = next(i for i, rec in enumerate(recs) if rec[1] == B.EQ_ZERO and i > 2 * TILE + 100)
    recs[eqz][3][0] ^= 1
    with pytest.raises(r.R0HipError, match=rf"Invalid eqz in bigint accum \(row {recs[eqz][0]}\)"):
        _prove(hal, oracle, job, recs)
    seal, _ = _prove(hal, oracle, job, job[4])
    assert r.verify_seal("rv32im", r.POSEIDON2, seal, check_validity=False) == 14
