"""The opt-in device receipt check on the GPU: r0hip_merkle_open_digests against the oracle's
hash_elems / hash_pair (the transcript's hash functions), r0hip_verify_seal_on(DEVICE) against
the host check on accepted and corrupted seals (verdict, message, po2, code root), memory and
thread modes, and verify = 2 in the trace pipeline and the worker. Every comparison is exact."""
import itertools
import threading

import numpy as np
import pytest

import recursion_program as RP
import rv32im_trace as T
import verifier
from test_verify_device_host import _structure, _structure_on, _verify, _verify_on, zero_witness_seal

pytestmark = pytest.mark.gpu

P = 15 * 2**27 + 1
HOST, DEVICE = 0, 1
KEY = np.arange(8, dtype=np.uint32) * np.uint32(0x9E3779B9) + np.uint32(7)
WAIT_S = 120.0


@pytest.fixture(scope="module")
def r():
    import risc0_amd as r
    return r


@pytest.fixture(scope="module")
def hal(r):
    return r.HipHal("poseidon2")


# ---- 1. the op against the host hashes ---------------------------------------------------------
def expected(oracle, suite, words, table):
    """(digests, status) by MerkleVerifier::check's recurrence with the oracle's hashes"""
    dg, st = np.zeros((len(table), 8), np.uint32), np.zeros(len(table), np.uint32)
    for k, (row_off, path_off, index, cols, levels) in enumerate(table):
        path = words[path_off:path_off + 8 * levels].reshape(levels, 8)
        if suite == 0 and (path >= P).any():
            st[k] = 2
            continue
        cur = oracle.hash_elems(suite, np.ascontiguousarray(words[row_off:row_off + cols]))
        idx = index
        for lv in range(levels):
            other = np.ascontiguousarray(path[lv])
            cur = oracle.hash_pair(suite, other, cur) if idx & 1 else oracle.hash_pair(suite, cur, other)
            idx >>= 1
        dg[k] = cur
    return dg, st


COLS = (1, 15, 16, 17, 32, 33, 64, 103, 211, 256)
LEVELS = (0, 1, 2, 17)
N_OPEN = (1, 3, 4, 5, 63, 64, 65, 350)


def _index(kind, levels):
    lead = 1 << levels  # any heap index has a leading one above the bits the path reads
    return lead | {"left": 0, "right": lead - 1, "alt": 0xAAAAAAAAAAAAAAAA & (lead - 1)}[kind]


def _launches(suite, seed):
    """the launch sizes of N_OPEN, their openings cycling through every (cols, levels, index, row
    data) combination: 555 openings over 360 combinations"""
    rng = np.random.default_rng(seed)
    combos = itertools.cycle(itertools.product(COLS, LEVELS, ("left", "right", "alt"), ("max", "zero", "rand")))
    out = []
    for n in N_OPEN:
        words, table = [], []
        pos = 0
        for _ in range(n):
            cols, levels, kind, data = next(combos)
            row = {"max": np.full(cols, P - 1, np.uint32), "zero": np.zeros(cols, np.uint32),
                   "rand": rng.integers(0, P, cols, dtype=np.uint64).astype(np.uint32)}[data]
            # SHA-256 path digests are any 32-bit words: >= p and all ones among them
            hi = P if suite == 0 else 2**32
            path = rng.integers(0, hi, 8 * levels, dtype=np.uint64).astype(np.uint32)
            if suite == 1 and levels:
                path[0], path[-1] = 0xFFFFFFFF, P
            table.append((pos, pos + cols, _index(kind, levels), cols, levels))
            words += [row, path]
            pos += cols + 8 * levels
        out.append((np.concatenate(words), table))
    return out


@pytest.mark.parametrize("suite", [0, 1])
def test_op_matches_the_host_hashes(r, hal, oracle, suite):
    seen = set()
    for words, table in _launches(suite, 0x6F70656E + suite):
        want_d, want_s = expected(oracle, suite, words, table)
        got_d, got_s = r.merkle_open_digests(suite, words, table)
        assert not want_s.any() and np.array_equal(got_s, want_s), len(table)
        bad = np.flatnonzero((got_d != want_d).any(axis=1))
        assert bad.size == 0, f"n_open {len(table)}: openings {bad[:8]} differ, first {table[bad[0]]}"
        seen |= {(t[3], t[4]) for t in table}
    assert seen == set(itertools.product(COLS, LEVELS))
    assert r.merkle_open_digests(suite, np.zeros(4, np.uint32), [])[0].shape == (0, 8)


def test_op_poseidon2_noncanonical_path_word_is_status_2(r, hal, oracle):
    """one path word = p at the first, a middle and the last level: status 2 for that opening
    (zeros for its digest), the other openings of the launch untouched"""
    rng = np.random.default_rng(0x32)
    levels, cols, n = 5, 33, 9
    words = rng.integers(0, P, n * (cols + 8 * levels), dtype=np.uint64).astype(np.uint32)
    table = [(k * (cols + 8 * levels), k * (cols + 8 * levels) + cols, _index("alt", levels) + k % 2, cols, levels)
             for k in range(n)]
    for k, level, word in ((2, 0, 3), (4, 2, 0), (6, levels - 1, 7)):
        words[table[k][1] + 8 * level + word] = P
    want_d, want_s = expected(oracle, 0, words, table)
    assert list(np.flatnonzero(want_s == 2)) == [2, 4, 6]
    got_d, got_s = r.merkle_open_digests(0, words, table)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_d, want_d)
    assert not got_d[[2, 4, 6]].any() and got_d[[0, 1, 3, 5, 7, 8]].any(axis=1).all()
    # SHA-256 takes the same words as they are
    want_d, want_s = expected(oracle, 1, words, table)
    got_d, got_s = r.merkle_open_digests(1, words, table)
    assert not got_s.any() and np.array_equal(got_d, want_d)


@pytest.mark.parametrize("suite", [0, 1])
def test_op_shared_rows_and_overlapping_ranges(r, hal, oracle, suite):
    words = np.random.default_rng(0x33 + suite).integers(0, P, 600, dtype=np.uint64).astype(np.uint32)
    table = [(0, 300, 0b100, 64, 2), (0, 316, 0b111, 64, 2),   # one row, two paths
             (10, 300, 0b101, 103, 2),                          # a row overlapping the first, the first's path
             (40, 5, 0b110, 17, 2),                             # a path that lies inside other openings' rows
             (584, 600, 1, 16, 0),                              # the last words of the buffer, no path
             (0, 464, 1 << 17, 256, 17)]                        # path up to the buffer's last word
    want_d, want_s = expected(oracle, suite, words, table)
    got_d, got_s = r.merkle_open_digests(suite, words, table)
    assert np.array_equal(got_s, want_s) and not got_s.any() and np.array_equal(got_d, want_d)
    assert np.array_equal(got_d[0], got_d[1]) is False


# ---- 2. seals -----------------------------------------------------------------------------------
def top_size(rows):
    layers, top_layer = rows.bit_length() - 1, 0
    for i in range(1, layers):
        if (1 << i) > 50:
            break
        top_layer = i
    return 1 << top_layer


def seal_layout(circuit, po2, size):
    """word offsets of a seal's parts (verify_core.h's reads in order): tops[name], and the openings
    in order as (tree name, row_off, cols, path_off, levels)"""
    taps = verifier.Taps(circuit)
    d, n = taps.d, 1 << po2
    gs = d["group_sizes"]
    pos = (1 if circuit == "rv32im" else 0) + d["output_size"] + 1
    trees, tops = {}, {}

    def tree(name, rows, cols):
        nonlocal pos
        ts = top_size(rows)
        tops[name] = pos
        pos += 8 * ts
        trees[name] = (cols, (rows.bit_length() - 1) - (ts.bit_length() - 1))

    for name, g in (("code", 1), ("data", 2), ("accum", 0)):
        tree(name, 4 * n, gs[g])
    tree("check", 4 * n, 16)
    pos += (taps.num_taps + 16) * 4
    degree, domain, rounds = n, 4 * n, []
    while degree > 256:
        domain //= 16
        tree(f"fri{len(rounds)}", domain, 64)
        rounds.append(f"fri{len(rounds)}")
        degree //= 16
    pos += 4 * degree
    openings = []
    for _ in range(50):
        for name in ["accum", "code", "data", "check"] + rounds:
            cols, levels = trees[name]
            openings.append((name, pos, cols, pos + cols, levels))
            pos += cols + 8 * levels
    assert pos == size, (pos, size)
    return tops, openings


def random_witness_seal(oracle, suite, po2):
    """a seal whose rows all differ (synthetic witness: the structure check accepts it)"""
    d = oracle.load_circuit_json("recursion")
    rng = np.random.default_rng(0x5EA1 + po2)
    n, gs = 1 << po2, d["group_sizes"]
    code, data, accum = (oracle.rand_elems(rng, gs[g] * n) for g in (1, 2, 0))
    seal, _mix, _ = oracle.prove_segment("recursion", suite, po2, code, data, accum,
                                         oracle.rand_elems(rng, d["output_size"]))
    return seal


_SEALS = {}


def seals_of(oracle, suite, po2):
    """(accepted zero-witness seal, random-witness seal), made once per (suite, po2) and never changed"""
    if (suite, po2) not in _SEALS:
        pair = zero_witness_seal(oracle, suite, po2), random_witness_seal(oracle, suite, po2)
        for s in pair:
            s.setflags(write=False)
        _SEALS[(suite, po2)] = pair
    return _SEALS[(suite, po2)]


def _opening(openings, name, which):
    return [o for o in openings if o[0] == name][which]


def corruptions(seal, suite, po2):
    """name -> corrupted copy: one flipped bit (or one word set to p) per case of the issue"""
    tops, opens = seal_layout("recursion", po2, seal.size)
    out = {}

    def flip(name, at, bit=1):
        bad = seal.copy()
        bad[at] ^= np.uint32(bit)
        out[name] = bad

    data, check = _opening(opens, "data", 7), _opening(opens, "check", 11)
    flip("data row word", data[1] + 5)
    flip("check path word", check[3] + 8 * (check[4] // 2) + 3, 1 << 9)
    flip("top-layer digest word", tops["data"] + 8 * 3 + 2, 1 << 4)
    if "fri0" in tops:
        fri = _opening(opens, "fri0", 20)
        flip("fri row word", fri[1] + 17)
        flip("fri path word", fri[3] + 8 * (fri[4] - 1) + 6, 1 << 20)
    if suite == 0:
        acc = _opening(opens, "accum", 30)
        bad = seal.copy()
        bad[acc[3] + 8 + 1] = P
        out["path word = p"] = bad
    # two corruptions in different openings: the earlier one's message wins. Both are path words (a
    # flipped row word fails the FRI arithmetic, which runs before any opening is hashed); with
    # Poseidon2 one of the two is a word = p, so the two orders give two different messages.
    early, late = _opening(opens, "code", 4), _opening(opens, "data", 40)
    bad = seal.copy()
    bad[early[3] + 5] ^= np.uint32(1)
    bad[late[3] + 2] = P if suite == 0 else bad[late[3] + 2] ^ np.uint32(2)
    out["path flip, then a later path word = p"] = bad
    bad = seal.copy()
    bad[early[3] + 2] = P if suite == 0 else bad[early[3] + 2] ^ np.uint32(2)
    bad[late[3] + 5] ^= np.uint32(1)
    out["path word = p, then a later path flip"] = bad
    return out


@pytest.mark.parametrize("po2", [8, 11])
@pytest.mark.parametrize("suite", [0, 1, 2])
def test_device_check_matches_the_host_check_on_recursion_seals(r, hal, oracle, suite, po2):
    valid, rand = seals_of(oracle, suite, po2)
    _, opens = seal_layout("recursion", po2, valid.size)
    assert len(opens) == (200 if po2 == 8 else 250)
    want = _verify(r, "recursion", suite, valid)
    assert want[0] is None and want[1] == po2
    assert _verify_on(r, DEVICE, "recursion", suite, valid) == want  # verdict, po2_out and the code root
    assert _structure_on(r, DEVICE, "recursion", suite, rand) == _structure(r, "recursion", suite, rand) == (None, po2)
    # the allow-list is enforced on the device leg too
    root = np.frombuffer(want[2], np.uint32)
    assert r.verify_seal("recursion", suite, valid, code_roots=root, where="device") == po2
    with pytest.raises(r.R0HipError, match="code root"):
        r.verify_seal("recursion", suite, valid, code_roots=root ^ np.uint32(1), where="device")
    for seal, fn_host, fn_dev in ((valid, lambda s: _verify(r, "recursion", suite, s)[0],
                                   lambda s: _verify_on(r, DEVICE, "recursion", suite, s)[0]),
                                  (rand, lambda s: _structure(r, "recursion", suite, s)[0],
                                   lambda s: _structure_on(r, DEVICE, "recursion", suite, s)[0])):
        for name, bad in corruptions(seal, suite, po2).items():
            h, d = fn_host(bad), fn_dev(bad)
            # (the zero witness's rows are all equal: a top-layer digest no query reaches may change)
            assert h is not None or (seal is valid and name == "top-layer digest word"), name
            assert d == h, (name, d, h)
            if name == "path word = p" or name.startswith("path word = p, then"):
                assert h == ("non-canonical Poseidon2 digest word in seal" if suite == 0 else "merkle path mismatch"), name
            elif name.startswith("path flip, then") or name in ("check path word", "fri path word"):
                assert h == "merkle path mismatch", name


def test_device_check_matches_the_host_check_on_an_rv32im_seal(r, hal):
    """a po2-13 seal from the GPU prover (300 openings, two FRI rounds): both entry points"""
    t = T.random_trace(13, 200, seed=0x5249)
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    seal, _mix = r.prove_segment_trace(hal, 13, t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle)
    tops, opens = seal_layout("rv32im", 13, seal.size)
    assert len(opens) == 300
    want = _verify(r, "rv32im", 0, seal)
    assert want[0] is None and want[1] == 13
    assert _verify_on(r, DEVICE, "rv32im", 0, seal) == want
    assert _structure_on(r, DEVICE, "rv32im", 0, seal) == _structure(r, "rv32im", 0, seal) == (None, 13)
    data, fri1 = _opening(opens, "data", 13), _opening(opens, "fri1", 49)
    for at, val_ in ((data[1] + 200, None), (fri1[3] + 4, None), (fri1[3] + 9, P), (tops["check"] + 5, None)):
        bad = seal.copy()
        bad[at] = val_ if val_ is not None else bad[at] ^ np.uint32(1)
        h = _verify(r, "rv32im", 0, bad)
        assert h[0] is not None and _verify_on(r, DEVICE, "rv32im", 0, bad)[0] == h[0], (at, h[0])
        assert _structure_on(r, DEVICE, "rv32im", 0, bad)[0] == _structure(r, "rv32im", 0, bad)[0]


# ---- 3. memory and mode -------------------------------------------------------------------------
def test_device_check_keeps_no_memory_and_works_in_every_thread_mode(r, hal, oracle):
    valid, rand = seals_of(oracle, 0, 11)
    r.trim()
    before = r.mem_stats()["live"]
    assert r.verify_seal("recursion", 0, valid, where="device") == 11
    bad = rand.copy()
    bad[rand.size - 40] ^= np.uint32(1)
    with pytest.raises(r.R0HipError):
        r.verify_seal("recursion", 0, bad, check_validity=False, where="device")
    r.trim()
    assert r.mem_stats()["live"] == before
    # the device leg is one launch of the opening kernel per seal; Poseidon254 and the host leg launch none
    r.set_kernel_timing(True)
    try:
        r.verify_seal("recursion", 0, valid, where="device")
        r.verify_seal("recursion", 1, seals_of(oracle, 1, 11)[0], where="device")
        r.verify_seal("recursion", 2, seals_of(oracle, 2, 8)[0], where="device")
        r.verify_seal("recursion", 0, valid, where="host")
        kt = r.kernel_times()
    finally:
        r.set_kernel_timing(False)
    assert {k: v[1] for k, v in kt.items()} == {"merkle_open_poseidon2": 1, "merkle_open_sha256": 1}
    got = {}

    def deferred():
        L = r.lib()
        try:
            r.check(L.r0hip_set_deferred(1, None))
            buf = hal.alloc_elem("x", 1 << 12)
            hal.eltwise_zeroize_elem(buf)  # queued, not drained
            c0 = r.call_stats()
            got["deferred"] = r.verify_seal("recursion", 0, valid, where="device")
            c1 = r.call_stats()
            got["drained"] = c1["drained"] - c0["drained"]
            got["sha"] = r.verify_seal("recursion", 1, seals_of(oracle, 1, 11)[0], where="device")
            buf.free()
            r.check(L.r0hip_set_deferred(0, None))
        except Exception as e:  # noqa: BLE001
            got["deferred_error"] = e

    def streams():
        try:
            was = r.set_proof_streams(2)
            got["streams"] = (was, r.verify_seal("recursion", 0, valid, where="device"))
            r.set_proof_streams(1)
        except Exception as e:  # noqa: BLE001
            got["streams_error"] = e

    for fn in (deferred, streams):
        th = threading.Thread(target=fn)
        th.start()
        th.join()
    assert "deferred_error" not in got and "streams_error" not in got, got
    assert got["deferred"] == 11 and got["sha"] == 11 and got["drained"] == 1
    assert got["streams"] == (1, 11)
    r.trim()
    assert r.mem_stats()["live"] == before


# ---- 4. pipelines -------------------------------------------------------------------------------
def _trace_job(r, t):
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    return r.TraceJob(t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())


def test_trace_pipeline_with_device_receipt_checks(r, hal, monkeypatch):
    jobs = [_trace_job(r, T.random_trace(13, 150 + 40 * i, seed=90 + i)) for i in range(4)]
    host = r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify=1, per_job=True)
    dev = r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify=2, per_job=True)
    for (hs, hm, he, hms, _), (ds, dm, de, dms, _) in zip(host, dev):
        assert he is None and de is None and hms > 0 and dms > 0
        assert np.array_equal(hs, ds) and np.array_equal(hm, dm)
    # the non-per-job form asserts `verified` on every job; "device" is 2
    again = r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify="device")
    assert all(np.array_equal(a[0], h[0]) for a, h in zip(again, host))
    monkeypatch.setenv("R0HIP_TESTING_CORRUPT_SEAL_JOB", "1")
    try:
        host_bad = r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify=1, per_job=True)
        dev_bad = r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify=2, per_job=True)
        with pytest.raises(r.R0HipError, match="segment 1: receipt verification failed"):
            r.prove_trace_segments(hal, 13, jobs, in_flight=2, verify=2)
    finally:
        monkeypatch.delenv("R0HIP_TESTING_CORRUPT_SEAL_JOB")
    for i, (h, d) in enumerate(zip(host_bad, dev_bad)):
        if i == 1:
            assert h[2] is not None and h[2].startswith("receipt verification failed: ") and d[2] == h[2], (h[2], d[2])
        else:
            assert h[2] is None and d[2] is None and np.array_equal(d[0], host[i][0])


def test_worker_with_device_receipt_checks(r, hal):
    """one rv32im po2-13 job, one kind-3 recursion po2-11 job checked against the handle's control
    id, one Poseidon254 recursion job (its openings stay on the host threads): all verified"""
    rng = np.random.default_rng(7101)
    prog, inp = RP.random_program(rng, 300)
    wom, cyc, iops = RP.trace_arrays(RP.preflight(prog, inp))
    tjob = _trace_job(r, T.random_trace(13, 250, seed=21))
    results = {}
    for verify in (1, 2):
        with r.RecursionProgram.create(hal, 11, prog.encoded()) as handle:
            with r.Worker(hal, max_po2=13, in_flight=2, verify=verify, noise_key=KEY) as w:
                assert w.verify == verify
                assert w.submit_trace(tjob, 13) == 0
                assert w.submit_recursion_program(handle, wom, cyc, iops) == 1
                assert w.submit_recursion(11, RP.ctrl_group(prog, 11), wom, cyc, iops, suite="poseidon254") == 2
                got = {}
                for _ in range(3):
                    res = w.wait(WAIT_S)  # raises if a job without an error came back unverified
                    assert res is not None
                    got[res[0]] = res
        assert sorted(got) == [0, 1, 2]
        for ticket, seal, mix, err, verify_ms, prove_ms in got.values():
            assert err is None and verify_ms > 0, (ticket, err)
        results[verify] = got
    for ticket in range(3):
        assert np.array_equal(results[1][ticket][1], results[2][ticket][1])
