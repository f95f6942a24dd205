"""Pins the test helper tests/rv32im_backs.py (no GPU, and no library): build_injector restated
over the compact Back records gives, entry for entry, the injector the restated traces build
directly (Trace.injector_arrays). The GPU tests take their expected words from this helper."""
import collections

import numpy as np
import pytest

import rv32im_backs as B
import rv32im_trace as T


def _traces():
    return {"ecall14": lambda: T.ecall_trace(14, seed=3, bigint=True),
            "paging13": lambda: T.random_trace(13, 300, seed=2),
            "addi13": lambda: T.Trace(13, [T.asm("addi", 1, 0, 1)])}


@pytest.fixture(scope="module", params=sorted(_traces()))
def trace(request):
    return request.param, _traces()[request.param]()


def test_expand_of_pack_is_the_injector(trace):
    name, t = trace
    recs, words, inj_rows = B.pack(t)
    rows = 1 << t.po2
    assert inj_rows == rows == len(t.cyc)
    kinds = collections.Counter(int(k) for k in recs[:, 1])
    if name == "ecall14":  # all four kinds
        assert (kinds[B.POSEIDON2], kinds[B.SHA2], kinds[B.BIGINT], kinds[B.ECALL]) == (4808, 141, 18, 15)
    elif name == "paging13":
        assert set(kinds) == {B.POSEIDON2}
    # rows strictly increasing, payloads back to back; no word that becomes a field element is
    # P or more on a real trace (the reduction in Val::from is exercised by the synthetic GPU
    # cases only); the SHA-2 a, e, w words go out bit by bit and are any u32
    assert np.all(np.diff(recs[:, 0].astype(np.int64)) > 0)
    assert words.size == sum(B.WORDS[int(k)] for k in recs[:, 1])
    plain = np.ones(words.size, bool)
    for _, k, w in recs:
        if int(k) == B.SHA2:
            plain[int(w) + 7:int(w) + 10] = False
    assert not plain.any() or int(words[plain].max()) < T.P
    index, offsets, values = B.expand(recs, words, inj_rows, t.cyc, rows)
    ref_index, ref_offsets, ref_values = t.injector_arrays()
    assert np.array_equal(index, ref_index)
    assert np.array_equal(offsets, ref_offsets)
    assert np.array_equal(values, ref_values)
    assert index[-1] == 5 * rows + 39 * kinds[B.POSEIDON2] + 103 * kinds[B.SHA2] + 22 * kinds[B.BIGINT] + \
        3 * kinds[B.ECALL]
    assert B.bigint_records(recs, words) == t.bigint_records()
