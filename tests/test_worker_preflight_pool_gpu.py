"""The worker's kind-4 preflights on a pool of host threads (r0hip_worker_set_preflight_threads,
r0hip_worker_get_stats) on the device: every seal, mix and output word for word against
r0hip_prove_recursion_program_input with the worker's key and stream_id = ticket, and against the
same jobs on a worker without a pool; a handle without a plan; failures that stay with their job
and carry the message of the worker without a pool; a queue of every kind; more jobs than slots;
the setter's refusals and the memory after destroy. Programs are
recursion_program.satisfying_witness at po2 11 and 13 and those of recursion_input_programs.
Every wait passes a finite timeout and a job that does not come back fails the test before the
worker is destroyed."""
import numpy as np
import pytest

import recursion_input_programs as IP
import recursion_program as RP

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not RP.available(), reason="oracle/_ref/libref_recursion.so is not built")]

P = RP.P
WAIT_S = 60.0
KEY = np.array([0x03020100, 0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xFFFFFFFF],
               dtype=np.uint32)


@pytest.fixture(scope="module")
def hals():
    import risc0_amd as r
    return {s: r.HipHal(s) for s in ("poseidon2", "sha-256")}


class _Rec:
    """a program, one input of it, and the Python preflight's arrays (what kinds 1 and 3 take)"""

    def __init__(self, po2, w):
        self.po2, self.prog, self.input, self.code = po2, w["program"], list(w["input"]), w["program"].encoded()
        self.wom, self.cyc, self.iops = RP.trace_arrays(w["preflight"])
        self.output = [int(x) for x in w["preflight"].output]


@pytest.fixture(scope="module")
def recs():
    """11 and 13: the programs of test_recursion_input_gpu.py, which fill their segment"""
    return {po2: _Rec(po2, RP.satisfying_witness(8100 + po2, po2)) for po2 in (11, 13)}


@pytest.fixture(scope="module")
def two_inputs():
    """a po2-11 program whose rows read the input through the IOP, and two inputs of it"""
    b = RP.Builder(np.random.default_rng(11))
    for _ in range(8):
        b.block_iop()
        b.block_arith()
    prog, inp_a = b.finish()
    assert len(prog.rows) <= (1 << 11) - RP.ZK_CYCLES
    inp_b = [int(x) for x in np.random.default_rng(99).integers(0, P, len(inp_a))]
    return prog.encoded(), [list(inp_a), inp_b]


def _drain(w, count):
    """`count` finished jobs by ticket; a wait that times out fails the test"""
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        assert res[0] not in got, f"ticket {res[0]} returned twice"
        got[res[0]] = res
    assert w.wait(0) is None and w.outstanding() == 0
    return got


def _same(a, b):
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _run(r, hal, n, submit, count, max_po2=11, in_flight=2, verify=True):
    """one worker with n pool threads: submit(w) queues `count` jobs; returns (results by ticket,
    kind-4 outputs by ticket, the stats after the last job came back)"""
    with r.Worker(hal, max_po2=max_po2, in_flight=in_flight, verify=verify, noise_key=KEY) as w:
        assert w.set_preflight_threads(n) == 0
        submit(w)
        got = _drain(w, count)
        outs = {t: w.outputs.pop(t) for t in list(w.outputs)}
        st = w.stats()
        assert st.preflight_threads == n and st.preflight_slots == (n + in_flight + 1 if n else 0)
        assert st.peak_slots_in_use <= st.preflight_slots
    return got, outs, st


# ---- 1. seals under the pool -------------------------------------------------------------------
@pytest.mark.parametrize("suite", ["poseidon2", "sha-256"])
def test_seals_under_the_pool(hals, two_inputs, suite):
    import risc0_amd as r
    hal = hals[suite]
    code, inputs = two_inputs
    with r.RecursionProgram.create(hal, 11, code) as prog:
        prog.prepare_input()
        cid = prog.info()[3]

        def submit(w):
            for i in range(8):
                assert w.submit_recursion_input(prog, inputs[i % 2]) == i
        # the second input's witness is not known to satisfy the circuit, so no receipt check here
        pooled, pooled_out, st = _run(r, hal, 2, submit, 8, verify=False)
        plain, plain_out, st0 = _run(r, hal, 0, submit, 8, verify=False)
        want = [prog.prove_input(inputs[i % 2], KEY, i) for i in range(8)]
    assert (st.pool_jobs, st.inline_jobs) == (8, 0) and st.pool_busy_ms > 0 and st.slot_bytes > 0
    assert (st0.pool_jobs, st0.inline_jobs) == (0, 8) and st0.uploader_preflight_ms > 0 and st0.slot_bytes == 0
    for i in range(8):
        assert pooled[i][3] is None and plain[i][3] is None, (i, pooled[i][3], plain[i][3])
        assert _same(pooled[i][1:3], want[i][:2]), i
        assert _same(pooled[i][1:3], plain[i][1:3]), i
        assert np.array_equal(pooled_out[i], want[i][2]) and np.array_equal(plain_out[i], want[i][2]), i
    assert not np.array_equal(pooled[0][1], pooled[1][1])
    assert r.verify_seal("recursion", hal.suite, pooled[0][1], code_roots=cid) == 11


# ---- 2. a handle without a plan ----------------------------------------------------------------
def test_a_handle_without_a_plan(hals, recs):
    """the first job finds no plan and is left to the uploader, which makes it; whichever thread ran
    a preflight, the seal is the single call's"""
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs[11]
    with r.RecursionProgram.create(hal, 11, rec.code) as prog:
        assert not prog.input_info().prepared

        def submit(w):
            for i in range(4):
                assert w.submit_recursion_input(prog, rec.input, prepare=False, output_cap=len(rec.output)) == i
        got, outs, st = _run(r, hal, 2, submit, 4)
        assert prog.input_info().prepared
        want = [prog.prove_input(rec.input, KEY, i) for i in range(4)]
    assert st.inline_jobs >= 1 and st.pool_jobs + st.inline_jobs == 4
    for i in range(4):
        assert got[i][3] is None, (i, got[i][3])  # verified by the worker
        assert _same(got[i][1:3], want[i][:2]), i
        assert [int(x) for x in outs[i]] == rec.output, i


# ---- 3. failures stay with their job -----------------------------------------------------------
def test_failures_stay_with_their_job(hals, recs):
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs[11]
    eq_prog, eq_inp, eq_po2, eq_msg = IP.ERRORS["eq"]()
    assert eq_po2 == 11 and len(rec.output) > 0
    order = ["good", "eq", "good", "short", "good", "small", "good"]
    peq = r.RecursionProgram.create(hal, 11, eq_prog.encoded())
    prog = r.RecursionProgram.create(hal, 11, rec.code)
    try:
        peq.prepare_input()
        prog.prepare_input()

        def submit(w):
            for i, what in enumerate(order):
                if what == "eq":
                    t = w.submit_recursion_input(peq, eq_inp)
                elif what == "short":
                    t = w.submit_recursion_input(prog, rec.input[:-1])
                elif what == "small":
                    t = w.submit_recursion_input(prog, rec.input, output_cap=len(rec.output) - 1)
                else:
                    t = w.submit_recursion_input(prog, rec.input)
                assert t == i
        pooled, pooled_out, st = _run(r, hal, 2, submit, len(order))
        plain, _plain_out, st0 = _run(r, hal, 0, submit, len(order))
        want = {i: prog.prove_input(rec.input, KEY, i) for i, what in enumerate(order) if what == "good"}
    finally:
        # the workers are closed: every use count was released, or destroy would be refused
        peq.close()
        prog.close()
    assert (st.pool_jobs, st.inline_jobs) == (len(order), 0) and (st0.pool_jobs, st0.inline_jobs) == (0, len(order))
    import re
    for i, what in enumerate(order):
        ticket, seal, mix, err, _v, _p = pooled[i]
        if what == "good":
            assert err is None and plain[i][3] is None, (i, err, plain[i][3])
            assert _same((seal, mix), want[i][:2]) and _same((seal, mix), plain[i][1:3]), i
            assert [int(x) for x in pooled_out[i]] == rec.output, i
            continue
        assert err is not None and err == plain[i][3], (i, err, plain[i][3])
        assert seal.size == 0 and plain[i][1].size == 0, i
        if what == "eq":
            assert re.search(eq_msg, err), err
        elif what == "short":
            assert re.search(r"input exhausted: .* \(cycle \d+\)$", err), err
        else:
            assert f"output buffer too small: the program writes {len(rec.output)} words" in err, err


# ---- 4. a queue of every kind ------------------------------------------------------------------
def test_mixed_queue(hals, recs):
    import risc0_amd as r
    import rv32im_trace as T
    import rv32im_witgen_ref as W
    hal, r11, r13 = hals["poseidon2"], recs[11], recs[13]
    t = T.random_trace(13, 250, seed=21)
    cyc, tx = t.arrays()
    idx, off, val = W.injector_arrays(t)
    tjob = r.TraceJob(W.global_words(t), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())
    ctrl11 = RP.ctrl_group(r11.prog, 11)
    order = [(4, 11), (0, 13), (4, 13), (1, 11), (4, 11), (3, 13), (4, 13), (3, 11), (4, 11)]
    with r.RecursionProgram.create(hal, 11, r11.code) as p11, r.RecursionProgram.create(hal, 13, r13.code) as p13:
        progs = {11: (p11, r11), 13: (p13, r13)}
        p11.prepare_input()
        p13.prepare_input()

        def submit(w):
            for i, (kind, po2) in enumerate(order):
                prog, rec = progs[po2]
                if kind == 0:
                    ticket = w.submit_trace(tjob, 13)
                elif kind == 1:
                    ticket = w.submit_recursion(11, ctrl11, rec.wom, rec.cyc, rec.iops)
                elif kind == 3:
                    ticket = w.submit_recursion_program(prog, rec.wom, rec.cyc, rec.iops)
                else:
                    ticket = w.submit_recursion_input(prog, rec.input)
                assert ticket == i
        got, outs, st = _run(r, hal, 2, submit, len(order), max_po2=13)
        n4 = sum(1 for kind, _ in order if kind == 4)
        assert (st.pool_jobs, st.inline_jobs) == (n4, 0)
        for i, (kind, po2) in enumerate(order):
            ticket, seal, mix, err, _v, _p = got[i]
            assert err is None, (i, kind, err)  # each verified by the worker
            prog, rec = progs[po2]
            if kind == 0:
                want = r.prove_segment_trace(hal, 13, tjob.glob, tjob.index, tjob.offsets, tjob.values, tjob.cycles,
                                             tjob.txns, t.table_split_cycle, bigint=t.bigint_array(),
                                             bigint_records=t.bigint_records())
            elif kind == 1:
                d_ctrl = hal.copy_from_elem("ctrl", ctrl11)
                want = r.prove_recursion_keyed(hal, 11, d_ctrl, rec.wom, rec.cyc, rec.iops, KEY, ticket)
                d_ctrl.free()
            elif kind == 3:
                want = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, ticket)
            else:
                want = prog.prove_input(rec.input, KEY, ticket)
                assert [int(x) for x in outs[i]] == rec.output == [int(x) for x in want[2]], i
            assert _same((seal, mix), want[:2]), (i, kind)
    assert sorted(outs) == [i for i, (kind, _) in enumerate(order) if kind == 4]


# ---- 5. more jobs than slots -------------------------------------------------------------------
def test_back_pressure(hals, recs):
    """one prover, three pool threads, twelve jobs at once: the pool runs ahead only as far as its
    five slots allow, the slots grow when a po2-13 job follows a po2-11 one, and every job
    completes with the single call's seal"""
    import risc0_amd as r
    hal = hals["poseidon2"]
    with r.RecursionProgram.create(hal, 11, recs[11].code) as p11, \
            r.RecursionProgram.create(hal, 13, recs[13].code) as p13:
        progs = {11: (p11, recs[11]), 13: (p13, recs[13])}
        p11.prepare_input()
        p13.prepare_input()
        order = [11, 13] * 6

        def submit(w):
            for i, po2 in enumerate(order):
                assert w.submit_recursion_input(progs[po2][0], progs[po2][1].input) == i
        got, outs, st = _run(r, hal, 3, submit, 12, max_po2=13, in_flight=1)
        assert st.preflight_slots == 3 + 1 + 1 and 1 <= st.peak_slots_in_use <= st.preflight_slots
        assert (st.pool_jobs, st.inline_jobs) == (12, 0)
        i13 = p13.input_info()
        assert st.slot_bytes >= 16 * (i13.n_wom + i13.n_iops)  # at least one slot grew to a po2-13 job
        want = {po2: progs[po2][0].prove_input(progs[po2][1].input, KEY, order.index(po2)) for po2 in (11, 13)}
        for i, po2 in enumerate(order):
            assert got[i][3] is None, (i, got[i][3])
            assert [int(x) for x in outs[i]] == progs[po2][1].output, i
        for po2 in (11, 13):
            i = order.index(po2)
            assert _same(got[i][1:3], want[po2][:2]), i


# ---- 6. the setter -----------------------------------------------------------------------------
def test_the_setter(hals, recs):
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs[11]
    with r.RecursionProgram.create(hal, 11, rec.code) as prog:
        prog.prepare_input()
        want0 = prog.prove_input(rec.input, KEY, 0)
        r.trim()
        before = r.mem_stats()["live"]
        w = r.Worker(hal, max_po2=11, in_flight=2, verify=True, noise_key=KEY)
        try:
            assert w.stats().preflight_threads == 0 and w.stats().preflight_slots == 0
            assert w.set_preflight_threads(3) == 0
            assert w.set_preflight_threads(2) == 3
            assert w.set_preflight_threads(2) == 2
            with pytest.raises(r.R0HipError, match=r"r0hip_worker_set_preflight_threads: n 9 above 8"):
                w.set_preflight_threads(9)
            st = w.stats()
            assert (st.preflight_threads, st.preflight_slots) == (2, 2 + 2 + 1)
            # a job outstanding (queued, running or finished and not yet waited for): refused
            assert w.submit_recursion_input(prog, rec.input) == 0
            with pytest.raises(r.R0HipError, match=r"r0hip_worker_set_preflight_threads: n 0 refused with 1 jobs"):
                w.set_preflight_threads(0)
            st = w.stats()
            assert (st.preflight_threads, st.preflight_slots) == (2, 5)
            first = _drain(w, 1)[0]
            assert first[3] is None and _same(first[1:3], want0[:2])
            st = w.stats()
            assert (st.pool_jobs, st.inline_jobs) == (1, 0)
            # back to the uploader between batches: the next batch is inline only
            assert w.set_preflight_threads(0) == 2
            for i in (1, 2):
                assert w.submit_recursion_input(prog, rec.input) == i
            got = _drain(w, 2)
            st = w.stats()
            assert (st.preflight_threads, st.preflight_slots, st.slot_bytes) == (0, 0, 0)
            assert (st.pool_jobs, st.inline_jobs) == (1, 2)
            assert all(got[i][3] is None for i in (1, 2))
            # and on again
            assert w.set_preflight_threads(1) == 0
            assert w.submit_recursion_input(prog, rec.input) == 3
            last = _drain(w, 1)[3]
            st = w.stats()
            assert last[3] is None and (st.pool_jobs, st.inline_jobs) == (2, 2)
            assert r.mem_stats()["live"] > before
        finally:
            w.close()
        r.trim()
        assert r.mem_stats()["live"] == before
        assert _same(last[1:3], prog.prove_input(rec.input, KEY, 3)[:2])
