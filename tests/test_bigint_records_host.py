"""The structured-array form of the BigInt records (risc0_amd.bigint_backs) and the record
generator (tests/bigint_records.py) against the host function; no GPU needed."""
import os

import numpy as np
import pytest

import bigint_accum as B
import bigint_records as G
import rv32im_accum_ref as R


def _lib_or_skip():
    from risc0_amd.hal import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("libr0hip.so not built")


def _mix(rng):
    return rng.integers(0, B.P, R.MIX_WORDS, dtype=np.uint64).astype(np.uint32)


def test_structured_array_equals_tuple_form():
    import risc0_amd as r
    _lib_or_skip()
    assert G.DTYPE == r.BIGINT_BACK_DTYPE
    rng = np.random.default_rng(0x57C)
    mix = _mix(rng)
    _, recs = B.lay_out(rng, 1 << 10, 40)
    arr = np.zeros(len(recs), G.DTYPE)
    arr["row"], arr["poly_op"], arr["coeff"] = ([rec[i] for rec in recs] for i in range(3))
    arr["bytes"] = [rec[3] for rec in recs]
    assert bytes(r.bigint_backs(arr)) == bytes(r.bigint_backs(recs)) == arr.tobytes()
    want = r.bigint_accum_states(mix, recs, 1 << 10)
    assert np.array_equal(r.bigint_accum_states(mix, arr, 1 << 10), want)
    assert np.array_equal(r.bigint_accum_states(mix, np.repeat(arr, 2)[::2], 1 << 10), want)  # strided
    assert r.bigint_backs(arr[:0]) is None


def test_valid_stream_is_accepted_by_the_host_function():
    import risc0_amd as r
    _lib_or_skip()
    rng = np.random.default_rng(0x600D)
    mix = _mix(rng)
    n, rows = 20000, 1 << 16
    recs = G.valid_stream(rng, n, rows)
    assert recs.size == n and (np.diff(recs["row"].astype(np.int64)) > 0).all() and recs["row"][-1] < rows
    assert {int(op) for op in np.unique(recs["poly_op"])} == set(range(7))
    st = r.bigint_accum_states(mix, recs, rows)
    assert st.shape == (n, 12)
    # every EqZero leaves the cleared state, and the Python restatement agrees on a prefix
    eqz = recs["poly_op"] == B.EQ_ZERO
    assert eqz.sum() > n // 100
    assert (st[eqz] == st[eqz][0]).all()
    head = [(int(x["row"]), int(x["poly_op"]), int(x["coeff"]), [int(b) for b in x["bytes"]]) for x in recs[:300]]
    assert np.array_equal(st[:300], B.states(mix, head))
