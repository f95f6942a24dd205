"""Poseidon254 openings of the receipt check on the GPU, behind r0hip_set_verify_device_poseidon254:
r0hip_merkle_open_digests(2, ...) against the oracle's hash_elems / hash_pair, r0hip_verify_seal_on
(DEVICE) against the host check on accepted and corrupted Poseidon254 seals (verdict, message, po2,
code root), one kernel launch per check with the switch on and none with it off, memory, and
verify = 2 in the worker. Every comparison is exact. Every test that turns the switch on turns it
off again: it is process-wide and the other tests rely on its default."""
import itertools

import numpy as np
import pytest

import recursion_program as RP
from test_verify_device_gpu import (DEVICE, KEY, WAIT_S, _opening, _structure, _structure_on, _verify, _verify_on,
                                    corruptions, expected, seal_layout, seals_of)

pytestmark = pytest.mark.gpu

P = 15 * 2**27 + 1
R254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr
SUITE = 2


@pytest.fixture(scope="module")
def r():
    import risc0_amd as r
    return r


@pytest.fixture(scope="module")
def hal(r):
    return r.HipHal("poseidon2")


@pytest.fixture
def switch_on(r):
    r.set_verify_device_poseidon254(1)
    try:
        yield
    finally:
        r.set_verify_device_poseidon254(0)


def _digest(v):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)


EDGES = [_digest(v) for v in (0, R254 - 1, R254, 2**256 - 1)]

# ---- 1. the op against the oracle's hashes ------------------------------------------------------
COLS = (1, 7, 8, 9, 15, 16, 17, 32, 33, 103, 256)  # the pack-of-8 and rate-16 boundaries
LEVELS = (0, 1, 2, 17)
N_OPEN = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 250)  # around a quad, a wave of quads and a wave of lanes


def _index(kind, levels):
    lead = 1 << levels
    return lead | {"left": 0, "right": lead - 1, "alt": 0xAAAAAAAAAAAAAAAA & (lead - 1)}[kind]


def _launches(seed):
    """the launch sizes of N_OPEN, their 503 openings cycling through the 396 (cols, levels, index,
    row data) combinations; path digests are random 256-bit words, with 0, r - 1, r and all ones put
    at the first and the last level in turn"""
    rng = np.random.default_rng(seed)
    combos = itertools.cycle(itertools.product(COLS, LEVELS, ("left", "right", "alt"), ("max", "zero", "rand")))
    edge = itertools.cycle(range(4))
    out = []
    for n in N_OPEN:
        words, table, pos = [], [], 0
        for _ in range(n):
            cols, levels, kind, data = next(combos)
            row = {"max": np.full(cols, P - 1, np.uint32), "zero": np.zeros(cols, np.uint32),
                   "rand": rng.integers(0, P, cols, dtype=np.uint64).astype(np.uint32)}[data]
            path = rng.integers(0, 2**32, 8 * levels, dtype=np.uint64).astype(np.uint32)
            if levels:
                path[:8] = EDGES[next(edge)]
            if levels > 1:
                path[-8:] = EDGES[next(edge)]
            table.append((pos, pos + cols, _index(kind, levels), cols, levels))
            words += [row, path]
            pos += cols + 8 * levels
        out.append((np.concatenate(words), table))
    return out


def test_op_matches_the_oracle_hashes(r, hal, oracle, switch_on):
    seen, edges_seen = set(), set()
    for words, table in _launches(0x70323534):
        want_d, want_s = expected(oracle, SUITE, words, table)
        got_d, got_s = r.merkle_open_digests(SUITE, words, table)
        assert not want_s.any() and not got_s.any(), len(table)  # any 256-bit path digest is status 0
        bad = np.flatnonzero((got_d != want_d).any(axis=1))
        assert bad.size == 0, f"n_open {len(table)}: openings {bad[:8]} differ, first {table[bad[0]]}"
        seen |= {(t[3], t[4]) for t in table}
        edges_seen |= {words[t[1]:t[1] + 8].tobytes() for t in table if t[4]}
    assert seen == set(itertools.product(COLS, LEVELS))
    assert edges_seen == {e.tobytes() for e in EDGES}
    assert r.merkle_open_digests(SUITE, np.zeros(4, np.uint32), [])[0].shape == (0, 8)


def test_op_shared_rows_and_overlapping_ranges(r, hal, oracle, switch_on):
    """test_verify_device_gpu.test_op_shared_rows_and_overlapping_ranges' table at suite 2. Paths
    that lie inside rows are field words there, and are hashed as the digests they spell."""
    words = np.random.default_rng(0x33 + SUITE).integers(0, P, 600, dtype=np.uint64).astype(np.uint32)
    table = [(0, 300, 0b100, 64, 2), (0, 316, 0b111, 64, 2),   # one row, two paths
             (10, 300, 0b101, 103, 2),                          # a row overlapping the first, the first's path
             (40, 5, 0b110, 17, 2),                             # a path that lies inside other openings' rows
             (584, 600, 1, 16, 0),                              # the last words of the buffer, no path
             (0, 464, 1 << 17, 256, 17)]                        # path up to the buffer's last word
    want_d, want_s = expected(oracle, SUITE, words, table)
    got_d, got_s = r.merkle_open_digests(SUITE, words, table)
    assert np.array_equal(got_s, want_s) and not got_s.any() and np.array_equal(got_d, want_d)
    assert not np.array_equal(got_d[0], got_d[1])


def test_op_is_refused_with_the_switch_off(r, hal):
    with pytest.raises(r.R0HipError, match="suite = 2"):
        r.merkle_open_digests(SUITE, np.zeros(64, np.uint32), [(0, 16, 5, 16, 2)])


# ---- 2. seals -----------------------------------------------------------------------------------
def _p254_corruptions(seal, po2):
    """corruptions(seal, 2, po2), and the Poseidon2-only case made for Poseidon254: a path word = p
    is a legal word of a 256-bit digest here, so it is a wrong digest, not a non-canonical one"""
    out = corruptions(seal, SUITE, po2)
    _, opens = seal_layout("recursion", po2, seal.size)
    acc = _opening(opens, "accum", 30)
    bad = seal.copy()
    bad[acc[3] + 8 + 1] = P
    out["path word = p"] = bad
    return out


@pytest.mark.parametrize("po2", [8, 11])
def test_device_check_matches_the_host_check_on_poseidon254_seals(r, hal, oracle, po2, switch_on):
    valid, rand = seals_of(oracle, SUITE, po2)
    _, opens = seal_layout("recursion", po2, valid.size)
    assert len(opens) == (200 if po2 == 8 else 250)
    want = _verify(r, "recursion", SUITE, valid)
    assert want[0] is None and want[1] == po2
    r.set_kernel_timing(True)
    try:
        got = _verify_on(r, DEVICE, "recursion", SUITE, valid)
        kt = r.kernel_times()
    finally:
        r.set_kernel_timing(False)
    assert got == want  # verdict, po2_out and the code root
    assert {k: v[1] for k, v in kt.items()} == {"merkle_open_poseidon254": 1}
    assert _structure_on(r, DEVICE, "recursion", SUITE, rand) == _structure(r, "recursion", SUITE, rand) == (None, po2)
    # the allow-list is enforced on the device leg too
    root = np.frombuffer(want[2], np.uint32)
    assert r.verify_seal("recursion", SUITE, valid, code_roots=root, where="device") == po2
    with pytest.raises(r.R0HipError, match="code root"):
        r.verify_seal("recursion", SUITE, valid, code_roots=root ^ np.uint32(1), where="device")
    for seal, fn_host, fn_dev in ((valid, lambda s: _verify(r, "recursion", SUITE, s)[0],
                                   lambda s: _verify_on(r, DEVICE, "recursion", SUITE, s)[0]),
                                  (rand, lambda s: _structure(r, "recursion", SUITE, s)[0],
                                   lambda s: _structure_on(r, DEVICE, "recursion", SUITE, s)[0])):
        for name, bad in _p254_corruptions(seal, po2).items():
            h, d = fn_host(bad), fn_dev(bad)
            # (the zero witness's rows are all equal: a top-layer digest no query reaches may change)
            assert h is not None or (seal is valid and name == "top-layer digest word"), name
            assert d == h, (name, d, h)
            if name.startswith("path") or name in ("check path word", "fri path word"):
                assert h == "merkle path mismatch", (name, h)


def test_first_corrupted_opening_in_opening_order_wins(r, hal, oracle, switch_on):
    """Poseidon254 openings have one message ("merkle path mismatch": no path word is
    non-canonical), so two corrupted openings give it whichever comes first; the device leg must
    give it for each flip alone and for both, as the host does. A failure the host finds before it
    hashes any opening (a row word >= p, refused while the seal is read) still comes first when a
    later opening's path is corrupted too. Since the message cannot tell the two orders apart, the
    op says which openings the device found changed: over the seal's own opening table (any one
    side pattern, the same for both seals) exactly the corrupted openings' digests differ from the
    good seal's, so the first that differs is the earlier one, the one check_pending reaches first."""
    _, rand = seals_of(oracle, SUITE, 8)
    _, opens = seal_layout("recursion", 8, rand.size)
    early, late = _opening(opens, "code", 4), _opening(opens, "data", 40)
    table = [(row_off, path_off, 1 << levels, cols, levels) for _, row_off, cols, path_off, levels in opens]
    good_d, _ = r.merkle_open_digests(SUITE, rand, table)
    for flips, changed in (([(early[3] + 5, 1)], [early]), ([(late[3] + 2, 2)], [late]),
                           ([(early[3] + 5, 1), (late[3] + 2, 2)], [early, late])):
        bad = rand.copy()
        for at, bit in flips:
            bad[at] ^= np.uint32(bit)
        h = _structure(r, "recursion", SUITE, bad)
        assert h[0] == "merkle path mismatch"
        assert _structure_on(r, DEVICE, "recursion", SUITE, bad) == h
        bad_d, bad_s = r.merkle_open_digests(SUITE, bad, table)
        differ = list(np.flatnonzero((bad_d != good_d).any(axis=1)))
        assert not bad_s.any() and differ == [opens.index(o) for o in changed], differ
        assert opens.index(early) < opens.index(late)
    bad = rand.copy()
    bad[late[3] + 2] ^= np.uint32(2)
    bad[early[1] + 3] = P
    h = _structure(r, "recursion", SUITE, bad)
    assert h[0] == "non-canonical field element in seal"
    assert _structure_on(r, DEVICE, "recursion", SUITE, bad) == h


def test_top_layers_on_the_verifier_threads_change_nothing(r, hal, oracle, switch_on, monkeypatch):
    """R0_VERIFY_P254_TOPS=1 (read at each check): the nodes above each tree's top layer come from
    hash_tops instead of the serial loop. Verdict, po2, code root and messages are the host's, on
    the accepted seal and with a top-layer digest or a path word corrupted."""
    valid, rand = seals_of(oracle, SUITE, 11)
    monkeypatch.setenv("R0_VERIFY_P254_TOPS", "1")
    want = _verify(r, "recursion", SUITE, valid)
    assert want[0] is None and _verify_on(r, DEVICE, "recursion", SUITE, valid) == want
    cases = _p254_corruptions(rand, 11)
    for name in ("top-layer digest word", "check path word"):
        h = _structure(r, "recursion", SUITE, cases[name])
        assert h[0] is not None and _structure_on(r, DEVICE, "recursion", SUITE, cases[name]) == h, name


def test_switch_off_launches_nothing(r, hal, oracle):
    valid, _ = seals_of(oracle, SUITE, 8)
    r.set_kernel_timing(True)
    try:
        assert r.verify_seal("recursion", SUITE, valid, where="device") == 8
        kt = r.kernel_times()
    finally:
        r.set_kernel_timing(False)
    assert kt == {}


# ---- 3. memory ----------------------------------------------------------------------------------
def test_device_check_keeps_no_memory(r, hal, oracle, switch_on):
    valid, rand = seals_of(oracle, SUITE, 8)
    r.trim()
    before = r.mem_stats()["live"]
    assert r.verify_seal("recursion", SUITE, valid, where="device") == 8
    r.trim()
    assert r.mem_stats()["live"] == before
    bad = rand.copy()
    bad[rand.size - 40] ^= np.uint32(1)  # a path word of the last opening
    with pytest.raises(r.R0HipError, match="merkle path mismatch"):
        r.verify_seal("recursion", SUITE, bad, check_validity=False, where="device")
    r.trim()
    assert r.mem_stats()["live"] == before


# ---- 4. the worker ------------------------------------------------------------------------------
def test_worker_checks_a_poseidon254_receipt_on_the_device(r, hal):
    """one Poseidon254 recursion job at po2 11, verify = 1 against verify = 2 with the switch on:
    both verified, and the same seal. (A failing receipt inside the worker is not covered: the
    library's seal-corruption hook is in the trace pipeline only, which proves no recursion jobs.)"""
    rng = np.random.default_rng(7101)
    prog, inp = RP.random_program(rng, 300)
    wom, cyc, iops = RP.trace_arrays(RP.preflight(prog, inp))
    results = {}
    for verify in (1, 2):
        r.set_verify_device_poseidon254(1 if verify == 2 else 0)
        try:
            with r.Worker(hal, max_po2=11, in_flight=2, verify=verify, noise_key=KEY) as w:
                assert w.verify == verify
                assert w.submit_recursion(11, RP.ctrl_group(prog, 11), wom, cyc, iops, suite="poseidon254") == 0
                res = w.wait(WAIT_S)  # raises if a job without an error came back unverified
        finally:
            r.set_verify_device_poseidon254(0)
        assert res is not None and res[0] == 0
        ticket, seal, mix, err, verify_ms, prove_ms = res
        assert err is None and verify_ms > 0, err
        results[verify] = seal
    assert np.array_equal(results[1], results[2])
