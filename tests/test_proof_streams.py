"""One proof's independent work on several streams (r0hip_set_proof_streams).

With n >= 2 the code group's commitment (interpolate, evaluate, row hashes, tree layers) runs on
a side stream: beside the witness generation in r0hip_prove_recursion*, beside the data group's
commitment in the other prove calls. The roots still enter the transcript code first, and the
arithmetic is the same kernels on the same words, so everything here compares a run at n = 2 or
n = 3 with the same call at n = 1, word for word, and checks the seal with the verifier. The
setting is the calling thread's: the pipeline's and the worker's own threads stay at 1."""
import gc
import threading

import numpy as np
import pytest

import rv32im_trace as T
import test_golden as G

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
SUITES = ("poseidon2", "sha-256", "poseidon_254")


@pytest.fixture(scope="module")
def r():
    import risc0_amd
    return risc0_amd


@pytest.fixture(scope="module")
def hals(r):
    return {s: r.HipHal(s) for s in SUITES}


@pytest.fixture(scope="module")
def hal(hals):
    return hals["poseidon2"]


@pytest.fixture(autouse=True)
def one_stream_after(r):
    """no test leaves its thread above one stream, or with kernel timing on"""
    yield
    r.set_proof_streams(1)
    r.set_kernel_timing(False)


def dev(h, a):
    return h.copy_from_elem("x", a)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the switch -----------------------------------------------------------------------------------
def test_switch_semantics(r, hal):
    assert r.set_proof_streams(1) == 1  # the default
    assert r.set_proof_streams(3) == 1 and r.set_proof_streams(2) == 3  # returns the previous value
    for bad in (0, 4):
        with pytest.raises(r.R0HipError, match="proof streams must be 1..3"):
            r.set_proof_streams(bad)
        assert r.set_proof_streams(2) == 2  # unchanged by the failed call
    r.set_proof_streams(3)
    seen = {}

    def other():
        seen["n"] = r.set_proof_streams(1)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["n"] == 1  # thread-local: 1 on a new thread while this one holds 3
    assert r.set_proof_streams(1) == 3
    with hal.proof_streams(2):
        assert r.set_proof_streams(2) == 2
    assert r.set_proof_streams(1) == 1


# ---- seals ----------------------------------------------------------------------------------------
def at_each_n(r, prove):
    """prove() at n = 1, 2 and 3"""
    out = []
    for n in (1, 2, 3):
        r.set_proof_streams(n)
        out.append(prove())
    r.set_proof_streams(1)
    return out


@pytest.mark.parametrize("case", G.INDEX["seals"], ids=lambda c: f"{c['circuit']}-{c['suite']}-po2{c['po2']}")
def test_prove_segment_golden_seals(r, hals, oracle, case):
    circuit, po2 = case["circuit"], case["po2"]
    h = hals[case["suite"]]
    w = [dev(h, a) for a in G.seal_inputs(oracle, circuit, po2)]
    one, two, three = at_each_n(r, lambda: r.prove_segment(h, circuit, po2, *w, version=2 if circuit == "rv32im" else None))
    assert G.digest(one[0]) == case["seal_sha256"]
    assert same(two, one) and same(three, one)
    assert r.verify_seal(circuit, h.suite, two[0], check_validity=False) == po2


@pytest.mark.parametrize("suite,po2", [("poseidon2", 10), ("sha-256", 9)])
def test_prove_segment_accum_seals(r, hals, oracle, suite, po2):
    from test_rv32im_accum_ir import rows_for_arms
    h = hals[suite]
    d = oracle.load_circuit_json("rv32im")
    gs, n = d["group_sizes"], 1 << po2
    rng = np.random.default_rng(0x41434355 + po2)
    code = oracle.rand_elems(rng, gs[1] * n)
    data = rows_for_arms(rng, n, list(rng.integers(0, 13, n)))
    glob = oracle.rand_elems(rng, d["output_size"])
    acc0 = np.full(gs[0] * n, INVALID, np.uint32)

    def prove():  # the call fills the accum group and zeroizes glob in place: fresh buffers each time
        return r.prove_segment_accum(h, "rv32im", po2, dev(h, code), dev(h, data), dev(h, acc0), n, dev(h, glob), version=2)
    one, two, three = at_each_n(r, prove)
    assert same(two, one) and same(three, one)
    assert r.verify_seal("rv32im", h.suite, two[0], check_validity=False) == po2


@pytest.mark.parametrize("suite,po2", [("poseidon2", 14), ("sha-256", 11)])
def test_prove_recursion_seals(r, hals, suite, po2):
    """a program of tests/recursion_program.py; po2 11 is the smallest the ZK rows allow"""
    import recursion_program as RP
    if not RP.available():
        pytest.skip("oracle/_ref not built")
    h = hals[suite]
    rng = np.random.default_rng(5000 + po2)
    prog, inp = RP.random_program(rng, (1 << po2) - RP.ZK_CYCLES - 1)
    wom, cyc, iops = RP.trace_arrays(RP.preflight(prog, inp))
    ctrl = dev(h, RP.ctrl_group(prog, po2))
    one, two, three = at_each_n(r, lambda: r.prove_recursion(h, po2, ctrl, wom, cyc, iops, 0x5EED00 + po2))
    ctrl.free()
    assert same(two, one) and same(three, one)
    assert r.verify_seal("recursion", h.suite, two[0], check_validity=True) == po2


def trace_job(r, t):
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    return r.TraceJob(t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())


def prove_trace(r, hal, po2, t, job):
    return r.prove_segment_trace(hal, po2, job.glob, job.index, job.offsets, job.values, job.cycles, job.txns,
                                 t.table_split_cycle, bigint=t.bigint_array(), bigint_records=t.bigint_records())


@pytest.fixture(scope="module")
def trace13(r, hal):
    """a po2 13 trace (the smoke run's size), its job and its seal and mix at n = 1"""
    t = T.random_trace(13, 200, seed=0x5249534330)
    job = trace_job(r, t)
    r.set_proof_streams(1)
    return t, job, prove_trace(r, hal, 13, t, job)


def test_prove_segment_trace_seal(r, hal, trace13):
    t, job, one = trace13
    for n in (2, 3):
        r.set_proof_streams(n)
        assert same(prove_trace(r, hal, 13, t, job), one), n
    assert r.verify_seal("rv32im", hal.suite, one[0], check_validity=True) == 13


# ---- the library's own threads stay at one stream ---------------------------------------------------
def test_pipeline_and_worker_from_a_thread_at_three(r, hal, trace13):
    t, job, one = trace13
    r.set_proof_streams(3)
    (piped,) = r.prove_trace_segments(hal, 13, [job], in_flight=2)
    assert same(piped, one)
    with r.Worker(hal, max_po2=13, in_flight=2, verify=True) as w:
        w.submit_trace(job, 13)
        res = w.wait(120.0)
    assert res is not None and res[3] is None, res
    assert np.array_equal(res[1], one[0]) and np.array_equal(res[2], one[1])
    assert r.set_proof_streams(1) == 3  # and the caller's setting is its own


# ---- memory ---------------------------------------------------------------------------------------
def test_memory_goes_back_and_is_reused(r, hal, trace13):
    """live bytes after n = 3 proofs and a trim are what they were (the blocks used on the side
    stream are handed back with the rest); a second proof of the same size allocates nothing"""
    t, job, one = trace13
    r.set_proof_streams(1)
    gc.collect()  # buffers of earlier tests are freed now, not between the two readings
    r.trim()
    live = r.mem_stats()["live"]
    r.set_proof_streams(3)
    assert same(prove_trace(r, hal, 13, t, job), one)
    assert r.mem_stats()["live"] == live  # nothing stays with the thread between calls
    mallocs = r.mem_stats()["mallocs"]
    assert same(prove_trace(r, hal, 13, t, job), one)
    assert r.mem_stats()["mallocs"] == mallocs
    r.trim()
    assert r.mem_stats()["live"] == live


# ---- kernel timing --------------------------------------------------------------------------------
def test_kernel_timing_runs_on_one_stream(r, hal, trace13):
    """while kernel timing is on the thread behaves as n = 1 (the timing events bracket work on
    the main stream): the same seal, the same kernel families"""
    t, job, one = trace13
    fam = []
    for n in (1, 3):
        r.set_proof_streams(n)
        r.set_kernel_timing(True)
        r.kernel_times()  # start from an empty list
        assert same(prove_trace(r, hal, 13, t, job), one)
        times = r.kernel_times()
        r.set_kernel_timing(False)
        fam.append(sorted(times))
    assert "eval_check" in fam[0] and fam[1] == fam[0]
