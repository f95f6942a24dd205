"""The GPU worker (r0hip_worker_*) and its keyed ZK noise (r0hip_fill_chacha20,
r0hip_prove_recursion_keyed) on the device: the noise kernel against the plain-Python ChaCha20
of tests/chacha_model.py, the keyed recursion proof against the oracle prover on the compiled
reference's witness, and the worker's queue (mixed sizes and kinds, streaming, failures,
capacity growth, memory) against the single calls it is built from. Every wait passes a finite
timeout and a job that does not come back fails the test."""
import numpy as np
import pytest

import chacha_model as M
import rv32im_trace as T
import rv32im_witgen_ref as W

pytestmark = pytest.mark.gpu

WAIT_S = 120.0
KEY = np.array([0x03020100, 0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xFFFFFFFF],
               dtype=np.uint32)


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


@pytest.fixture(scope="module")
def hal_sha():
    import risc0_amd as r
    return r.HipHal("sha-256")


# ---- r0hip_fill_chacha20 ----------------------------------------------------------------------
def _fill(hal, key, nonce, count, offset=0, pad=8):
    """`count` stream elements written at word `offset` of a buffer pre-filled with a marker;
    returns the whole buffer"""
    import risc0_amd as r
    buf = hal.alloc_elem_init("noise", offset + count + pad, 0xA5A5A5A5)
    r.fill_chacha20(buf, key, nonce, count=count, offset=offset)
    out = buf.to_numpy()
    buf.free()
    return out


def test_fill_chacha20_rfc_vector_elements(hal):
    """with RFC 8439 2.3.2's key and nonce, block 1 of the stream is elements 4..7"""
    out = _fill(hal, M.RFC_KEY, M.RFC_NONCE, 8)
    assert [int(v) for v in out[4:8]] == [728272357, 838115523, 261376304, 378995873]
    assert np.array_equal(out[:8], M.elements(M.RFC_KEY, M.RFC_NONCE, 8))


@pytest.fixture(scope="module")
def model_stream():
    nonce = np.array([1, 0x89ABCDEF, 0x01234567], dtype=np.uint32)
    return nonce, M.elements(KEY, nonce, 128 * 1024)


@pytest.mark.parametrize("count", [1, 3, 4, 5, 255, 1025, 128 * 1024])
def test_fill_chacha20_matches_the_model(hal, model_stream, count):
    """every count (a partial block, whole blocks, a tail, more than one workgroup, a recursion
    proof's largest noise matrix) gives the model's words, all below p, and writes nothing past
    `count`"""
    nonce, ref = model_stream
    out = _fill(hal, KEY, nonce, count)
    assert np.array_equal(out[:count], ref[:count])
    assert int(out[:count].max()) < M.P
    assert np.all(out[count:] == 0xA5A5A5A5)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_fill_chacha20_unaligned_destination(hal, model_stream, offset):
    """a destination 4, 8 or 12 bytes past 16-byte alignment (no uint4 store possible) gives the
    same words and touches nothing before or after them"""
    nonce, ref = model_stream
    count = 1027
    out = _fill(hal, KEY, nonce, count, offset=offset)
    assert np.array_equal(out[offset:offset + count], ref[:count])
    assert np.all(out[:offset] == 0xA5A5A5A5) and np.all(out[offset + count:] == 0xA5A5A5A5)


# ---- r0hip_prove_recursion_keyed --------------------------------------------------------------
@pytest.fixture(scope="module")
def rec14():
    """one recursion program filling a po2=14 segment, its preflight and control group (as
    test_prove_recursion_from_program builds them)"""
    import recursion_program as RP
    if not RP.available():
        pytest.skip("oracle/_ref/libref_recursion.so not built")
    po2 = 14
    rng = np.random.default_rng(3000 + po2)
    prog, inp = RP.random_program(rng, (1 << po2) - RP.ZK_CYCLES - 1)
    pf = RP.preflight(prog, inp)
    wom, cyc, iops = RP.trace_arrays(pf)
    return dict(po2=po2, prog=prog, pf=pf, wom=wom, cyc=cyc, iops=iops, ctrl=RP.ctrl_group(prog, po2))


def _nonce(which, stream_id):
    return np.array([which, stream_id & 0xFFFFFFFF, stream_id >> 32], dtype=np.uint32)


def _keyed(r, hal, rec, key, stream_id):
    d_ctrl = hal.copy_from_elem("ctrl", rec["ctrl"])
    out = r.prove_recursion_keyed(hal, rec["po2"], d_ctrl, rec["wom"], rec["cyc"], rec["iops"], key, stream_id)
    d_ctrl.free()
    return out


def test_prove_recursion_keyed_matches_oracle(hal, oracle, rec14):
    """po2=14, Poseidon2, a fixed key: the seal and the mix equal the oracle prover's on the
    witness the compiled reference's witgen and accumulation make with the model's ChaCha noise
    words in the last 1024 rows (data: nonce {0, lo, hi}; accum: {1, lo, hi}); another
    stream_id gives another seal that verifies; two OS-keyed calls differ and both pass the
    verifier with the validity equation"""
    import recursion_program as RP
    import risc0_amd as r
    import verifier
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    po2, n, zk = rec14["po2"], 1 << rec14["po2"], RP.ZK_CYCLES
    s = oracle.POSEIDON2
    stream_id = (0x0BADC0DE << 32) | 0x12345678
    seal, mix = _keyed(r, hal, rec14, KEY, stream_id)
    assert r.verify_seal("recursion", s, seal) == po2
    assert verifier.verify(oracle, "recursion", seal, s, check_validity=True)["validity"] is True

    ctrl = rec14["ctrl"]
    _, data, glob = RP.witgen(rec14["prog"], rec14["pf"], po2, raw=True)
    data = data.reshape(RP.DATA, n)
    data[:, n - zk:] = M.elements(KEY, _nonce(0, stream_id), RP.DATA * zk).reshape(RP.DATA, zk)
    data = np.where(data == RP.INVALID, 0, data).astype(np.uint32).reshape(-1)
    glob = np.where(glob == RP.INVALID, 0, glob).astype(np.uint32)
    acc0 = np.full((RP.ACCUM, n), RP.INVALID, np.uint32)
    acc0[:, n - zk:] = M.elements(KEY, _nonce(1, stream_id), RP.ACCUM * zk).reshape(RP.ACCUM, zk)
    w = dict(ctrl=ctrl, data=data, glob=glob, work=len(rec14["prog"].rows), acc0=acc0.reshape(-1))
    acc = RP.accumulate(w, mix, po2)
    ref_seal, ref_mix, _ = oracle.prove_segment("recursion", s, po2, ctrl, data, acc, glob)
    assert np.array_equal(mix, ref_mix)
    assert np.array_equal(seal, ref_seal)

    again, _ = _keyed(r, hal, rec14, KEY, stream_id)
    assert np.array_equal(again, seal)
    other, _ = _keyed(r, hal, rec14, KEY, stream_id + 1)
    assert not np.array_equal(other, seal)
    assert r.verify_seal("recursion", s, other) == po2

    a, _ = _keyed(r, hal, rec14, None, 0)
    b, _ = _keyed(r, hal, rec14, None, 0)
    assert not np.array_equal(a, b)
    assert r.verify_seal("recursion", s, a) == po2 and r.verify_seal("recursion", s, b) == po2


# ---- the worker -------------------------------------------------------------------------------
def _trace_job(r, t):
    cyc, tx = t.arrays()
    idx, off, val = W.injector_arrays(t)
    return r.TraceJob(W.global_words(t), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())


class _Seg:
    """a trace, its TraceJob and (on first use) the seal and mix of r0hip_prove_segment_trace"""

    def __init__(self, r, hal, po2, trace):
        self.r, self.hal, self.po2, self.t = r, hal, po2, trace
        self.job = _trace_job(r, trace)
        self._single = None

    def single(self):
        if self._single is None:
            j, t = self.job, self.t
            self._single = self.r.prove_segment_trace(self.hal, self.po2, j.glob, j.index, j.offsets, j.values,
                                                      j.cycles, j.txns, t.table_split_cycle, bigint=t.bigint_array(),
                                                      bigint_records=t.bigint_records())
        return self._single


@pytest.fixture(scope="module")
def segs(hal):
    """the rv32im segments the worker tests share, each proved alone at most once"""
    import risc0_amd as r
    return dict(rand13=_Seg(r, hal, 13, T.random_trace(13, 250, seed=21)),
                loop14a=_Seg(r, hal, 14, T.loop_s_trace(14, 300, seed=40)),
                loop14b=_Seg(r, hal, 14, T.loop_s_trace(14, 397, seed=41)),
                ecall14=_Seg(r, hal, 14, T.ecall_trace(14, seed=6, bigint=True)))


def _drain(w, count):
    """`count` finished jobs by ticket; a wait that times out fails the test"""
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        assert res[0] not in got, f"ticket {res[0]} returned twice"
        got[res[0]] = res
    return got


def test_worker_mixed_queue(hal, hal_sha, segs, rec14):
    """max_po2=14, two provers, verification on, a fixed key; rv32im jobs of po2 13 and 14 (one
    with BigInt records) interleaved with a Poseidon2 and a SHA-256 recursion job. Every rv32im
    seal and mix equal r0hip_prove_segment_trace's at the job's po2, the po2=14 ones also
    r0hip_prove_trace_segments' on the same jobs; every recursion seal equals
    r0hip_prove_recursion_keyed(key, ticket); all are verified; each job comes back once."""
    import risc0_amd as r
    order = [("t", "rand13"), ("r", hal), ("t", "loop14a"), ("t", "ecall14"), ("r", hal_sha), ("t", "loop14b")]
    # the recursion jobs' references first: their control roots are the allow-lists
    rec_ref = {i: _keyed(r, h, rec14, KEY, i) for i, (kind, h) in enumerate(order) if kind == "r"}
    roots = {i: r.verify_seal("recursion", order[i][1].suite, rec_ref[i][0], return_code_root=True)[1]
             for i in rec_ref}
    with r.Worker(hal, max_po2=14, in_flight=2, verify=True, noise_key=KEY) as w:
        for i, (kind, what) in enumerate(order):
            if kind == "t":
                ticket = w.submit_trace(segs[what].job, segs[what].po2)
            else:
                decoy = np.arange(8, dtype=np.uint32)
                ticket = w.submit_recursion(14, rec14["ctrl"], rec14["wom"], rec14["cyc"], rec14["iops"],
                                            code_roots=np.concatenate([decoy, roots[i]]), suite=what.suite)
            assert ticket == i
        assert w.outstanding() == len(order)
        got = _drain(w, len(order))
        assert w.wait(0) is None
    assert sorted(got) == list(range(len(order)))
    for i, (kind, what) in enumerate(order):
        ticket, seal, mix, err, verify_ms, prove_ms = got[i]
        assert err is None, err
        assert verify_ms > 0 and prove_ms > 0
        ref_seal, ref_mix = segs[what].single() if kind == "t" else rec_ref[i]
        assert np.array_equal(seal, ref_seal), (i, kind)
        assert np.array_equal(mix, ref_mix), (i, kind)
    names14 = ["loop14a", "ecall14", "loop14b"]
    piped = r.prove_trace_segments(hal, 14, [segs[k].job for k in names14], in_flight=2)
    for k, (seal, mix) in zip(names14, piped):
        i = order.index(("t", k))
        assert np.array_equal(got[i][1], seal) and np.array_equal(got[i][2], mix)


def test_worker_streaming(hal, segs):
    """jobs submitted while others are in flight: two in, one out, two more in, three out; then a
    poll and an unbounded wait both return nothing at once, since nothing is outstanding"""
    import risc0_amd as r
    names = ["rand13", "loop14a", "loop14b", "rand13"]
    with r.Worker(hal, max_po2=14, in_flight=2, verify=True, noise_key=KEY) as w:
        assert w.wait(0) is None and w.wait(None) is None  # nothing submitted yet
        tickets = [w.submit_trace(segs[k].job, segs[k].po2) for k in names[:2]]
        got = _drain(w, 1)
        tickets += [w.submit_trace(segs[k].job, segs[k].po2) for k in names[2:]]
        more = _drain(w, 3)
        assert not set(got) & set(more)
        got.update(more)
        assert w.wait(0) is None
        assert w.wait(None) is None
        assert w.outstanding() == 0
    assert tickets == [0, 1, 2, 3] and sorted(got) == tickets
    for i, k in enumerate(names):
        assert got[i][3] is None, got[i][3]
        assert np.array_equal(got[i][1], segs[k].single()[0]) and np.array_equal(got[i][2], segs[k].single()[1])


def test_worker_failures_stay_local(hal, segs, rec14):
    """a trace job whose injector index decreases fails with the host check's text and the jobs
    around it return the seals of a clean run; a po2=15 job is refused at submit and queues
    nothing; a recursion job whose allow-list lacks its control root alone reports `receipt
    verification failed`"""
    import risc0_amd as r
    good = segs["loop14a"]
    bad = _trace_job(r, good.t)
    bad.index[1001] = bad.index[1000] - 1
    big = _trace_job(r, good.t)
    with r.Worker(hal, max_po2=14, in_flight=2, verify=True, noise_key=KEY) as w:
        t0 = w.submit_trace(good.job, 14)
        t1 = w.submit_trace(bad, 14)
        with pytest.raises(r.R0HipError, match="po2 15 above the worker's max_po2 14"):
            w.submit_trace(big, 15)
        t2 = w.submit_recursion(14, rec14["ctrl"], rec14["wom"], rec14["cyc"], rec14["iops"],
                                code_roots=np.arange(16, dtype=np.uint32))
        t3 = w.submit_trace(segs["ecall14"].job, 14)
        t4 = w.submit_recursion(14, rec14["ctrl"], rec14["wom"], rec14["cyc"], rec14["iops"])
        assert [t0, t1, t2, t3, t4] == [0, 1, 2, 3, 4]  # the refused job took no ticket
        assert w.outstanding() == 5
        got = _drain(w, 5)
        assert w.wait(0) is None
    assert got[0][3] is None and np.array_equal(got[0][1], good.single()[0])
    assert got[1][3] is not None and "injector index decreases at row 1000" in got[1][3]
    assert got[1][1].size == 0
    assert got[2][3] is not None and got[2][3].startswith("receipt verification failed: "), got[2][3]
    assert got[3][3] is None and np.array_equal(got[3][1], segs["ecall14"].single()[0])
    assert got[4][3] is None and got[4][1].size > 0
    # the refused allow-list was the only thing wrong with job 2: its seal is job 4's but for the noise
    assert r.verify_seal("recursion", hal.suite, got[2][1]) == 14
    assert got[2][1].size == got[4][1].size and not np.array_equal(got[2][1], got[4][1])


def test_worker_capacity_growth(hal):
    """one prover and two sets: small jobs (po2 13) land in both sets, a po2=16 job whose injector
    is four times and whose transaction array a hundred times larger then grows a used set,
    and small jobs follow it into the grown sets; every seal is the single call's"""
    import risc0_amd as r
    small = [_Seg(r, hal, 13, T.random_trace(13, 1, seed=s)) for s in (1, 2)]
    large = _Seg(r, hal, 16, T.loop_trace(16, body_len=24, seed=13))
    assert large.job.index[-1] > 3 * small[0].job.index[-1] and large.job.txns.size > 50 * small[0].job.txns.size
    seq = [small[0], small[1], large, small[1], small[0], large, small[0]]
    with r.Worker(hal, max_po2=16, in_flight=1, verify=True, noise_key=KEY) as w:
        for s in seq:
            w.submit_trace(s.job, s.po2)
        got = _drain(w, len(seq))
    for i, s in enumerate(seq):
        assert got[i][3] is None, got[i][3]
        assert np.array_equal(got[i][1], s.single()[0]) and np.array_equal(got[i][2], s.single()[1]), i


def test_worker_returns_its_device_memory(hal, segs, rec14):
    """after destroy and trim the library's live device bytes are what they were before create"""
    import risc0_amd as r
    r.trim()
    before = r.mem_stats()["live"]
    with r.Worker(hal, max_po2=14, in_flight=2, verify=True, noise_key=KEY) as w:
        assert r.mem_stats()["live"] > before
        w.submit_trace(segs["ecall14"].job, 14)
        w.submit_recursion(14, rec14["ctrl"], rec14["wom"], rec14["cyc"], rec14["iops"])
        w.submit_trace(segs["rand13"].job, 13)
        got = _drain(w, 3)
        assert all(res[3] is None for res in got.values())
    r.trim()
    assert r.mem_stats()["live"] == before
