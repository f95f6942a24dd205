"""The injector from the preflight's Back records on the device (r0hip_rv32im_inject_backs,
r0hip_prove_segment_trace_backs, the worker's R0HIP_JOB_RV32IM_BACKS): the expansion's words
against build_injector restated in numpy (tests/rv32im_backs.py, pinned to the traces' own
injector by tests/test_rv32im_backs.py), and every seal against the CSR path's on the
equivalent injector."""
import numpy as np
import pytest

import rv32im_backs as B
import rv32im_trace as T
import rv32im_witgen_ref as W

pytestmark = pytest.mark.gpu

P = T.P
WAIT_S = 120.0
KEY = np.arange(8, dtype=np.uint32) + 0x01020304


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


class _Seg:
    """a restated trace, its Back records, and (each at most once) the CSR single call's seal"""

    def __init__(self, po2, trace):
        self.po2, self.t = po2, trace
        self.recs, self.words, self.inj_rows = B.pack(trace)
        self.cyc, self.tx = trace.arrays()
        self.glob = W.global_words(trace)
        self._csr = {}

    def backs(self, r, recs=None, words=None, inj_rows=None, **kw):
        return r.Backs(self.recs if recs is None else recs, self.words if words is None else words,
                       self.inj_rows if inj_rows is None else inj_rows, **kw)

    def prove_backs(self, r, hal, backs=None):
        t = self.t
        return r.prove_segment_trace_backs(hal, self.po2, self.glob, self.backs(r) if backs is None else backs,
                                           self.cyc, self.tx, t.table_split_cycle, bigint=t.bigint_array())

    def prove_csr(self, r, hal, injector=None, records=None):
        """r0hip_prove_segment_trace on the trace's injector, or on the given CSR arrays"""
        t = self.t
        key = hal.suite if injector is None else None
        if key is None or key not in self._csr:
            idx, off, val = injector or W.injector_arrays(t)
            out = r.prove_segment_trace(hal, self.po2, self.glob, idx, off, val, self.cyc, self.tx,
                                        t.table_split_cycle, bigint=t.bigint_array(),
                                        bigint_records=t.bigint_records() if records is None else records)
            if key is None:
                return out
            self._csr[key] = out
        return self._csr[key]


@pytest.fixture(scope="module")
def segs():
    return dict(ecall14=_Seg(14, T.ecall_trace(14, seed=3, bigint=True)),
                paging13=_Seg(13, T.random_trace(13, 300, seed=2)),
                addi13=_Seg(13, T.Trace(13, [T.asm("addi", 1, 0, 1)])))


def _inject(r, hal, rows, cyc, backs):
    data = hal.alloc_elem_init("data", 211 * rows, T.INVALID)
    try:
        r.rv32im_inject_backs(data, rows, cyc, backs)
        return data.to_numpy()
    finally:
        data.free()


# ---- words ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ecall14", "paging13", "addi13"])
def test_inject_backs_words_match_the_scattered_injector(hal, segs, name):
    """into an all-INVALID group the expansion writes the data group hal_generate_witness prepares
    (W.inputs: INVALID with build_injector's output scattered in), word for word"""
    import risc0_amd as r
    s = segs[name]
    rows = 1 << s.po2
    got = _inject(r, hal, rows, s.cyc, s.backs(r))
    want = W.inputs(s.t)[0]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} words differ; first (col, row): {[(int(i) // rows, int(i) % rows) for i in bad[:8]]}"
    assert (got == T.INVALID).any()


# ---- edges ------------------------------------------------------------------------------------
SPECIAL = [0, P - 1, P, 0xFFFFFFFF]


def _payload(rng, kind, k):
    """plain words cycle through 0, P - 1, P, 2^32 - 1 (the reduction) and random words; the
    SHA-2 bit words are all ones, top and bottom bit only (bit order), then random"""
    n = B.WORDS[kind]
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[k % n] = SPECIAL[k % 4]
    w[(k + 3) % n] = SPECIAL[(k + 1) % 4]
    if kind == B.SHA2:
        w[7:10] = [(0xFFFFFFFF, 0x80000001, 0x00000001), (0x80000001, 0xFFFFFFFF, 0x7FFFFFFE)][k % 2]
        if k % 5 == 4:
            w[7:10] = rng.integers(0, 1 << 32, 3, dtype=np.uint64).astype(np.uint32)
    return w


def _edge_records(case, rows, inj_rows, rng):
    if case.startswith("kind"):
        kinds = [int(case[4:])]
        at = sorted({x for x in (0, 1, 63, 64, rows - 1, inj_rows - 1) if x < inj_rows})
    elif case.startswith("sha"):  # a wave tail (65) and two workgroups (257) of consecutive records
        kinds, n = [B.SHA2], int(case[3:])
        at = list(range(inj_rows - n - 1, inj_rows - 1))
    else:  # every kind, on a random half of the rows
        kinds = [B.ECALL, B.POSEIDON2, B.SHA2, B.BIGINT]
        at = sorted(rng.choice(inj_rows, inj_rows // 2, replace=False).tolist())
    recs, words = [], []
    for k, row in enumerate(at):
        kind = kinds[int(rng.integers(len(kinds)))]
        recs.append((row, kind, len(words)))
        words += _payload(rng, kind, k).tolist()
    return np.array(recs, np.uint32).reshape(-1, 3), np.array(words, np.uint32)


EDGES = [(rows, short, case) for rows in (64, 512) for short in (0, 3)
         for case in ("kind1", "kind2", "kind3", "kind4", "sha65", "sha257", "mixed")
         if not case.startswith("sha") or rows == 512]  # 65 consecutive records need more than 64 rows


@pytest.mark.parametrize("rows,short,case", EDGES)
def test_inject_backs_edges(hal, rows, short, case):
    """synthetic records over random cycle records: the helper's expansion scattered in numpy"""
    import risc0_amd as r
    inj_rows = rows - short
    rng = np.random.default_rng([rows, short, sum(map(ord, case))])
    cyc = np.zeros(rows, T.CYCLE_DTYPE)
    cyc["pc"] = rng.integers(0, 1 << 32, rows, dtype=np.uint64).astype(np.uint32)
    cyc["state"] = rng.integers(0, 1 << 32, rows, dtype=np.uint64).astype(np.uint32)
    cyc["state"][:4] = SPECIAL
    cyc["pc"][:3] = [0xFFFFFFFF, 0x0001FFFF, 0xFFFF0000]
    cyc["machineMode"] = rng.integers(0, 256, rows).astype(np.uint8)
    cyc["major"] = rng.integers(0, 256, rows).astype(np.uint8)  # not read without the prover's flag
    recs, words = _edge_records(case, rows, inj_rows, rng)
    assert recs.shape[0] > 0 and np.isin(np.array(SPECIAL[2:], np.uint32), words).all()
    got = _inject(r, hal, rows, cyc, r.Backs(recs, words, inj_rows))
    want = B.scattered(*B.expand(recs, words, inj_rows, cyc, rows), rows)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} words differ; first (col, row): {[(int(i) // rows, int(i) % rows) for i in bad[:8]]}"
    # rows at and past inj_rows are untouched
    assert np.all(got.reshape(211, rows)[:, inj_rows:] == T.INVALID)


# ---- seals ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu14(segs, oracle):
    """the CPU path on the po2=14 trace, once: (seal, mix, data group zeroized, ...)"""
    return W.prove_from_trace(segs["ecall14"].t, oracle.POSEIDON2, oracle)


def test_prove_from_backs_matches_csr_and_cpu_path(hal, segs, cpu14):
    """po2 14, all four kinds, Poseidon2: the seal and mix of r0hip_prove_segment_trace on the CSR
    arrays with the BigInt records, of the CPU path, and the validity equation holds"""
    import risc0_amd as r
    s = segs["ecall14"]
    seal, mix = s.prove_backs(r, hal)
    csr_seal, csr_mix = s.prove_csr(r, hal)
    assert np.array_equal(mix, csr_mix) and np.array_equal(seal, csr_seal)
    ref_seal, ref_mix = cpu14[0], cpu14[1]
    assert np.array_equal(mix, ref_mix) and np.array_equal(seal, ref_seal)
    assert r.verify_seal("rv32im", hal.suite, seal, check_validity=True) == 14


def test_prove_from_backs_sha256_suite(segs):
    import risc0_amd as r
    h = r.HipHal("sha-256")
    s = segs["paging13"]
    seal, mix = s.prove_backs(r, h)
    csr_seal, csr_mix = s.prove_csr(r, h)
    assert np.array_equal(mix, csr_mix) and np.array_equal(seal, csr_seal)


# ---- a record on a row of another arm ---------------------------------------------------------
def _outcome(f):
    import risc0_amd as r
    try:
        seal, mix = f()
        return ("seal", seal.tobytes(), mix.tobytes())
    except r.R0HipError as e:
        return ("error", str(e))


@pytest.mark.parametrize("kind,major,same", [(B.ECALL, m, False) for m in range(7)] +
                         [(B.SHA2, 2, False), (B.BIGINT, 10, False), (B.ECALL, 2, True), (B.ECALL, 4, True)])
def test_record_on_a_row_of_another_arm_matches_the_csr_path(hal, segs, cpu14, kind, major, same):
    """an Ecall record on a row of each other instruction arm, a SHA-2 record on a non-SHA row
    (columns the row's arm does not take from the injector), and a BigInt record in place of a
    Poseidon2 row's (columns that arm does take). same: the Ecall record holds the very values
    the row's arm stores in those columns (from the CPU path's data group), which Buffer::set
    accepts. The outcome, a seal or an error text, is that of r0hip_prove_segment_trace on the
    expansion of the same records."""
    import risc0_amd as r
    s = segs["ecall14"]
    cyc = s.cyc
    free = [i for i in range(100, s.t.table_split_cycle) if cyc["major"][i] == major and
            ((i in s.t.backs) == (kind == B.BIGINT))]
    if not free:
        assert kind == B.ECALL  # the trace has no row of this arm: nothing to put the record on
        return
    row = free[len(free) // 2]
    payload = {B.ECALL: [5, 6, 7], B.SHA2: [1, 2, 3, 4, 5, 6, 32, 0xFFFFFFFF, 0x80000001, 0],
               B.BIGINT: [0, 1, 2, 0, 4] + list(range(16)) + [40]}[kind]
    if same:  # Montgomery words of the finished row back to plain integers
        rows = 1 << s.po2
        payload = [int(cpu14[2][c * rows + row]) * pow(1 << 32, -1, P) % P for c in T.layout()["ecall_s"]]
    at = int(np.searchsorted(s.recs[:, 0], row))
    keep = at + (kind == B.BIGINT)  # the BigInt record replaces the row's own
    recs = np.concatenate([s.recs[:at], np.array([[row, kind, s.words.size]], np.uint32), s.recs[keep:]])
    words = np.concatenate([s.words, np.array(payload, np.uint32)])
    injector = B.expand(recs, words, s.inj_rows, cyc, 1 << s.po2)
    want = _outcome(lambda: s.prove_csr(r, hal, injector=injector, records=B.bigint_records(recs, words)))
    got = _outcome(lambda: s.prove_backs(r, hal, s.backs(r, recs=recs, words=words)))
    print(f"kind {kind} on row {row} (major {int(cyc['major'][row])}): CSR path {want[0]}"
          f"{': ' + want[1] if want[0] == 'error' else ''}")
    assert got[0] == want[0], (got[:2] if got[0] == "error" else got[0], want[:2] if want[0] == "error" else want[0])
    assert got == want
    if same:
        assert got[0] == "seal"
    # and the next valid call is unaffected
    seal, mix = s.prove_backs(r, hal)
    assert np.array_equal(seal, s.prove_csr(r, hal)[0])


# ---- validation -------------------------------------------------------------------------------
def _bad_backs(r, s):
    """(name, Backs, message) of every refused input, over the po2=13 paging trace's records"""
    recs, words, n = s.recs, s.words, s.inj_rows
    k = recs.shape[0] // 2
    out = []
    a = recs.copy()
    a[k, 0] = a[k - 1, 0]
    out.append(("equal rows", s.backs(r, recs=a), f"record {k} .*rows must strictly increase"))
    a = recs.copy()
    a[k, 0] = a[k - 1, 0] - 1
    out.append(("decreasing rows", s.backs(r, recs=a), f"record {k} .*rows must strictly increase"))
    for kind in (0, 5):
        a = recs.copy()
        a[k, 1] = kind
        out.append((f"kind {kind}", s.backs(r, recs=a), f"record {k} \\(row {int(recs[k, 0])}\\): kind {kind} is not 1..4"))
    a = recs.copy()
    a[-1, 2] = words.size - 38
    out.append(("payload past n_words", s.backs(r, recs=a), f"record {recs.shape[0] - 1} .*end past n_words {words.size}"))
    out.append(("n_words cut", s.backs(r, n_words=words.size - 1), "end past n_words"))
    last = int(recs[-1, 0])
    out.append(("row at inj_rows", s.backs(r, inj_rows=last), f"row {last}\\): row at or past inj_rows {last}"))
    out.append(("inj_rows above the segment", s.backs(r, inj_rows=n + 1), "inj_rows 8193 above the segment's 8192 rows"))
    b = s.backs(r)
    b.struct.recs = None
    out.append(("NULL recs", b, "recs is NULL"))
    b = s.backs(r)
    b.struct.words = None
    out.append(("NULL words", b, "words is NULL"))
    out.append(("NULL backs", None, "backs is NULL"))
    return out


def test_bad_records_are_refused_before_any_launch(hal, segs):
    """each bad input is refused with a message naming the record, with no kernel launched (the
    kernel timer sees none) and the per-op call's group untouched; the next valid call gives the
    CSR path's seal"""
    import risc0_amd as r
    s = segs["paging13"]
    rows = 1 << s.po2
    data = hal.alloc_elem_init("data", 211 * rows, T.INVALID)
    r.set_kernel_timing(True)
    try:
        before = r.kernel_times()  # (reading the timer clears it)
        assert "rv32im_backs_inject" not in before
        before = {}
        for name, backs, msg in _bad_backs(r, s):
            with pytest.raises(r.R0HipError, match=msg):
                s.prove_backs(r, hal, backs) if backs is not None else \
                    r.prove_segment_trace_backs(hal, s.po2, s.glob, None, s.cyc, s.tx, s.t.table_split_cycle)
            if backs is not None:
                with pytest.raises(r.R0HipError, match=msg):
                    r.rv32im_inject_backs(data, rows, s.cyc, backs)
            assert r.kernel_times() == before, name
    finally:
        r.set_kernel_timing(False)
    assert np.all(data.to_numpy() == T.INVALID)
    data.free()
    seal, mix = s.prove_backs(r, hal)
    csr_seal, csr_mix = s.prove_csr(r, hal)
    assert np.array_equal(seal, csr_seal) and np.array_equal(mix, csr_mix)


# ---- the worker -------------------------------------------------------------------------------
def _backs_job(r, s, backs=None):
    return r.BacksJob(s.glob, s.backs(r) if backs is None else backs, s.cyc, s.tx, s.t.table_split_cycle,
                      bigint=s.t.bigint_array())


def _drain(w, count):
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        assert res[0] not in got
        got[res[0]] = res
    return got


def test_worker_backs_jobs(hal, segs):
    """one queue with kind-2 jobs at po2 13 and 14, a CSR job and a recursion job: each seal is the
    single call's; a kind-2 job with a bad record is refused at submit and takes no ticket; after
    destroy and trim the live device bytes are what they were before create"""
    import recursion_program as RP
    import risc0_amd as r
    po2 = 14
    rng = np.random.default_rng(3000 + po2)
    prog, inp = RP.random_program(rng, (1 << po2) - RP.ZK_CYCLES - 1)
    wom, rcyc, iops = RP.trace_arrays(RP.preflight(prog, inp))
    ctrl = RP.ctrl_group(prog, po2)
    d_ctrl = hal.copy_from_elem("ctrl", ctrl)
    rec_ref = r.prove_recursion_keyed(hal, po2, d_ctrl, wom, rcyc, iops, KEY, 3)  # ticket 3 below
    d_ctrl.free()
    big, small = segs["ecall14"], segs["paging13"]
    csr = r.TraceJob(small.glob, *W.injector_arrays(small.t), small.cyc, small.tx, small.t.table_split_cycle)
    bad = small.recs.copy()
    bad[7, 1] = 9
    r.trim()
    before = r.mem_stats()["live"]
    with r.Worker(hal, max_po2=14, in_flight=2, verify=True, noise_key=KEY) as w:
        t0 = w.submit_backs(_backs_job(r, small), 13)
        t1 = w.submit_backs(_backs_job(r, big), 14)
        with pytest.raises(r.R0HipError, match="r0hip_worker_submit: backs: record 7 .*kind 9 is not 1..4"):
            w.submit_backs(_backs_job(r, small, small.backs(r, recs=bad)), 13)
        t2 = w.submit_trace(csr, 13)
        t3 = w.submit_recursion(14, ctrl, wom, rcyc, iops)
        t4 = w.submit_backs(_backs_job(r, small), 13)  # a smaller job into a set a larger one grew
        assert [t0, t1, t2, t3, t4] == [0, 1, 2, 3, 4]
        got = _drain(w, 5)
        assert w.wait(0) is None
    r.trim()
    assert r.mem_stats()["live"] == before
    for res in got.values():
        assert res[3] is None, res[3]
    for i, s in ((0, small), (1, big), (2, small), (4, small)):
        seal, mix = s.prove_csr(r, hal)
        assert np.array_equal(got[i][1], seal) and np.array_equal(got[i][2], mix), i
    assert np.array_equal(got[3][1], rec_ref[0]) and np.array_equal(got[3][2], rec_ref[1])
    # the single call from the records gives the same words again
    assert np.array_equal(big.prove_backs(r, hal)[0], got[1][1])
