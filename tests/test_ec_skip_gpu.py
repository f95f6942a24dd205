"""eval_check's kernel skipping on the device: the zero scan of the selector columns
(r0hip_testing_zero_scan), the per-op r0hip_eval_check and r0hip_constraint_rows with selector columns
zeroed, and one whole proof of a middle segment of the loop guest's session.

A kernel of the generated program is not launched when every term it holds is gated by a column
that is zero on the whole domain (tools/gen_eval_check.py). The result must not change by a word:
  * po2 2: against the numpy IR interpreter (ec_extreme.reference) for eval_check, and against the
    scalar restatement of the program on each row (constraint_rows_ref.evaluate_row) for the rows
    family;
  * po2 8: against the same call under R0_EC_SKIP=0, which launches every kernel (the parent's
    launch sequence, which the parity tests cover);
  * the proof: the seal with skipping on equals the seal with it off and verifies.
r0hip_eval_check_launched tells how many kernels ran. The CPU twin is test_ec_skip_host.py."""
import numpy as np
import pytest

import constraint_rows_ref as CR
import ec_extreme as X
import ec_skip_patterns as S
from ec_skip_patterns import patterns, zeroed

pytestmark = pytest.mark.gpu

P = X.P
GROUPS = ("accum", "code", "data")
POLY_MIX = (P - 2, 1, P - 1, 2)


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def launched():
    from risc0_amd import hal as H
    return H.eval_check_launched()


def words(plain):
    """plain values (numpy, < p) -> Montgomery words"""
    return ((np.asarray(plain, np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


# ---- the zero scan -------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [16, 256, 4096])
def test_zero_scan_mask_equals_numpy(hal, domain):
    """several columns, one nonzero word at each edge of a wave and of a block, or none"""
    from risc0_amd import hal as H
    rng = np.random.default_rng(domain)
    cols = 7
    for pos in (None, 0, 63, 64, 255, 256, domain - 1):
        if pos is not None and pos >= domain:
            continue
        m = np.zeros((cols, domain), np.uint32)
        m[3] = rng.integers(1, P, domain)      # dense
        if pos is not None:
            m[1, pos] = 1                      # one word, the smallest nonzero value
            m[5, pos] = 0x80000000             # one word, the top bit only
        want = sum(1 << c for c in range(cols) if not m[c].any())
        buf = hal.copy_from_elem("m", m)
        assert H.zero_scan(buf, cols, domain) == want, (domain, pos)
        # columns that start one word in and end one word early: no 16-byte alignment, a length
        # that is no multiple of 4 (the word-by-word path)
        if domain > 16:
            w = domain - 2
            want_u = sum(1 << c for c in range(cols - 1) if not m.reshape(-1)[1 + c * w:1 + (c + 1) * w].any())
            assert H.zero_scan(buf.ptr + 4, cols - 1, w) == want_u, (domain, pos, "unaligned")
        buf.free()
    # 64 columns: both flag words
    m = np.zeros((64, domain), np.uint32)
    live = [0, 31, 32, 63]
    for c in live:
        m[c, (c * 7) % domain] = 5
    buf = hal.copy_from_elem("m", m)
    assert H.zero_scan(buf, 64, domain) == (2**64 - 1) ^ sum(1 << c for c in live)
    buf.free()


# ---- per-op eval_check ---------------------------------------------------------------------------
def gpu_eval_check(hal, circuit, w, po2):
    D = 4 << po2
    out = hal.alloc_elem_init("check", 4 * D, 0xFFFFFFFF)
    bufs = [hal.copy_from_elem(k, w[k]) for k in GROUPS + ("mix", "global")]
    hal.eval_check(circuit, out, bufs[:3], bufs[3], bufs[4], X.enc(POLY_MIX), po2)
    got = out.to_numpy()
    for b in bufs + [out]:
        b.free()
    return got, launched()


@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
def test_eval_check_po2_2_matches_the_interpreter(hal, oracle, circuit):
    po2, D = 2, 16
    d = oracle.load_circuit_json(circuit)
    base, poly_mix = X.extreme_inputs(d, "edge_mix", po2)
    assert poly_mix == POLY_MIX
    skipped = {}
    for name, cols in patterns(circuit).items():
        plain = zeroed(base, cols, D)
        got, (n, total) = gpu_eval_check(hal, circuit, {k: words(v) for k, v in plain.items()}, po2)
        assert np.array_equal(got, X.enc(X.reference(circuit, d, plain, poly_mix, po2).reshape(-1))), name
        assert total == S.KERNELS[circuit, "ec"]
        skipped[name] = total - n
    print(circuit, skipped)
    assert skipped == S.SKIPPED[circuit, "ec"]


@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
def test_eval_check_po2_8_matches_the_run_without_skipping(hal, oracle, circuit, monkeypatch):
    po2, D = 8, 4 << 8
    d = oracle.load_circuit_json(circuit)
    base, _ = X.extreme_inputs(d, "edge_mix", po2)
    for name, cols in patterns(circuit).items():
        w = {k: words(v) for k, v in zeroed(base, cols, D).items()}
        monkeypatch.setenv("R0_EC_SKIP", "0")
        want, (n0, total) = gpu_eval_check(hal, circuit, w, po2)
        assert n0 == total == S.KERNELS[circuit, "ec"]
        monkeypatch.delenv("R0_EC_SKIP")
        got, (n, _) = gpu_eval_check(hal, circuit, w, po2)
        assert np.array_equal(got, want), name
        assert total - n == S.SKIPPED[circuit, "ec"][name], name


# ---- per-op constraint_rows ----------------------------------------------------------------------
def gpu_rows(hal, circuit, w, po2):
    import risc0_amd as r
    n = 1 << po2
    out = hal.alloc_elem_init("rows", 4 * n, 0xFFFFFFFF)
    bufs = [hal.copy_from_elem(k, w[k]) for k in GROUPS + ("mix", "global")]
    rep = r.constraint_rows(circuit, po2, bufs[1], bufs[2], bufs[0], bufs[3], bufs[4], X.enc(POLY_MIX), out)
    got = out.to_numpy().reshape(n, 4)
    for b in bufs + [out]:
        b.free()
    return got, rep, launched()


def row_inputs(d, n):
    """edge-value groups of n rows (ec_extreme's generator draws 4 << po2 points per column)"""
    assert n % 4 == 0
    po2 = (n // 4).bit_length() - 1
    return X.extreme_inputs(d, "edge_mix", po2)[0]


@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
def test_constraint_rows_po2_2_matches_the_program_on_each_row(hal, oracle, circuit):
    po2, n = 2, 4
    d = oracle.load_circuit_json(circuit)
    base = row_inputs(d, n)
    skipped = {}
    for name, cols in patterns(circuit).items():
        w = {k: words(v) for k, v in zeroed(base, cols, n).items()}
        got, rep, (k, total) = gpu_rows(hal, circuit, w, po2)
        assert total == S.KERNELS[circuit, "rows"]
        taps = CR.gather_taps(circuit, [w[g] for g in GROUPS], po2)
        for row in range(n):
            val, _, res = CR.evaluate_row(circuit, taps[row], w["mix"], w["global"], X.enc(POLY_MIX))
            assert [int(x) for x in got[row]] == [CR.enc(x) for x in CR._ext(val[res])], (name, row)
        assert rep["bad_rows"] == int(got.any(axis=1).sum())
        skipped[name] = total - k
    print(circuit, skipped)
    assert skipped == S.SKIPPED[circuit, "rows"]


@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
def test_constraint_rows_po2_8_matches_the_run_without_skipping(hal, oracle, circuit, monkeypatch):
    po2, n = 8, 256
    d = oracle.load_circuit_json(circuit)
    base = row_inputs(d, n)
    for name, cols in patterns(circuit).items():
        w = {k: words(v) for k, v in zeroed(base, cols, n).items()}
        monkeypatch.setenv("R0_EC_SKIP", "0")
        want, want_rep, (n0, total) = gpu_rows(hal, circuit, w, po2)
        assert n0 == total == S.KERNELS[circuit, "rows"]
        monkeypatch.delenv("R0_EC_SKIP")
        got, rep, (k, _) = gpu_rows(hal, circuit, w, po2)
        assert np.array_equal(got, want) and rep == want_rep, name
        assert total - k == S.SKIPPED[circuit, "rows"][name], name


# ---- one whole proof ------------------------------------------------------------------------------
def test_middle_segment_of_the_loop_session_proves_the_same_seal(hal, monkeypatch):
    """The second of three consecutive po2 16 segments of the loop guest uses majors 0, 2, 7, 9 and
    10 only: 14 of the 30 kernels have nothing live. The seal is word for word the one proved with
    every kernel launched, and the verifier accepts it with the validity equation."""
    import risc0_amd as r
    import rv32im_trace as T
    import rv32im_witgen_ref as W
    po2 = 16
    t = T.LoopSession(po2, T.loop_s_session_iterations(po2, 3), seed=11).segment(1)
    cyc, tx = t.arrays()
    idx, off, val = W.injector_arrays(t)

    def prove():
        return r.prove_segment_trace(hal, po2, W.global_words(t), idx, off, val, cyc, tx, t.table_split_cycle)

    monkeypatch.setenv("R0_EC_SKIP", "0")
    want_seal, want_mix = prove()
    assert launched() == (30, 30)
    monkeypatch.delenv("R0_EC_SKIP")
    seal, mix = prove()
    counts = launched()
    print("launched", counts)
    assert np.array_equal(seal, want_seal) and np.array_equal(mix, want_mix)
    assert r.verify_seal("rv32im", hal.suite, seal, check_validity=True) == po2
    assert counts == (16, 30)
