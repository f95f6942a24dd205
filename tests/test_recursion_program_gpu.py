"""Resident recursion programs on the device (r0hip_recursion_program_*, worker kind 3): the
expansion kernel word for word against numpy, the control id against the verifier's code root
and the per-op pipeline, and the seal of r0hip_prove_recursion_program against
r0hip_prove_recursion_keyed on the expanded control group: single calls, a handle used again and
again, two handles alive together, four threads on one handle, the worker's queue, memory, and a
failing witness. Programs are the hand-encoded ones of tests/recursion_program.py at po2 11..13."""
import threading

import numpy as np
import pytest

import recursion_program as RP
import rv32im_trace as T
import rv32im_witgen_ref as W

pytestmark = pytest.mark.gpu

P = RP.P
WAIT_S = 120.0
KEY = np.array([0x03020100, 0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xFFFFFFFF],
               dtype=np.uint32)
SPECIAL = [0, 1, P - 1, P, P + 1, 2**31, 2**32 - 1]
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def hals():
    import risc0_amd as r
    return {s: r.HipHal(s) for s in ("poseidon2", "sha-256", "poseidon254")}


class _Rec:
    """one program, its preflight trace and its control group as the host lays it out"""

    def __init__(self, po2, seed, rows):
        rng = np.random.default_rng(seed)
        self.po2 = po2
        self.prog, inp = RP.random_program(rng, rows)
        self.wom, self.cyc, self.iops = RP.trace_arrays(RP.preflight(self.prog, inp))
        self.code = self.prog.encoded()
        self.ctrl = RP.ctrl_group(self.prog, po2)


@pytest.fixture(scope="module")
def recs():
    """a: po2 11; b: po2 11, another program; c: po2 12; d: po2 13 (coefficients stay bit-reversed)"""
    return dict(a=_Rec(11, 7001, 300), b=_Rec(11, 7002, 420), c=_Rec(12, 7003, 500), d=_Rec(13, 7004, 700))


def _keyed(r, hal, rec, stream_id, trace=None):
    t = trace or rec
    d_ctrl = hal.copy_from_elem("ctrl", rec.ctrl)
    out = r.prove_recursion_keyed(hal, rec.po2, d_ctrl, t.wom, t.cyc, t.iops, KEY, stream_id)
    d_ctrl.free()
    return out


def _same(a, b):
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the expansion kernel ---------------------------------------------------------------------
def _expected_ctrl(code, rows, po2, form):
    n = 1 << po2
    c = code[:23 * rows].astype(np.uint64).reshape(rows, 23)
    if form == 0:
        c = (c % P) * RP.R % P  # Elem::from: the Montgomery word of x mod p
    out = np.zeros((23, n), dtype=np.uint32)
    out[:, :rows] = c.T.astype(np.uint32)
    return out.reshape(-1)


def _program_words(rows, rotation, seed):
    """rows x 23 random u32 words with the special words in the first, middle and last column of
    the first and last row (cell k holds SPECIAL[(rotation + k) % 7]: over the seven rotations
    every cell sees every word), followed by a sentinel tail the callee must never read"""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 2**32, size=23 * rows + 64, dtype=np.uint64).astype(np.uint32)
    k = 0
    for row in (0, rows - 1):
        for col in (0, 11, 22):
            code[23 * row + col] = SPECIAL[(rotation + k) % 7]
            k += 1
    code[23 * rows:] = SENTINEL
    return code


@pytest.mark.parametrize("po2, rows", [(11, 1), (11, 63), (11, 64), (11, 65), (11, 255), (11, 256), (11, 257),
                                       (11, 1024), (12, 3072)])
def test_expansion_matches_numpy(hals, po2, rows):
    """encoded and Montgomery form, the special words in every corner cell, every padding row
    zero, and no word past n_words (a sentinel, nonzero in either form) in the group"""
    import risc0_amd as r
    n = 1 << po2
    sentinel_words = [SENTINEL, int(SENTINEL % P * RP.R % P)]
    for rotation in range(7):
        words = _program_words(rows, rotation, 100 * rows + rotation)
        for form in (r.CODE_ENCODED, r.CODE_MONTGOMERY):
            code = words if form == r.CODE_ENCODED else np.where(words == SENTINEL, words, words % P).astype(np.uint32)
            with r.RecursionProgram.create(hals["poseidon2"], po2, code, form=form, n_words=23 * rows) as prog:
                suite, got_po2, got_rows, _cid, _dev = prog.info()
                got = prog.ctrl()
            assert (suite, got_po2, got_rows) == (0, po2, rows)
            want = _expected_ctrl(code, rows, po2, form)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (f"form {form} rotation {rotation}: {bad.size} words differ; first col {bad[0] // n} "
                                   f"row {bad[0] % n}: {got[bad[0]]:#x} != {want[bad[0]]:#x}")
            g = got.reshape(23, n)
            assert not g[:, rows:].any(), "a padding row is not zero"
            # the tail's word (as given, or as Elem::from would make it) is nowhere the program did not put it
            assert np.isin(got, sentinel_words).sum() == np.isin(want, sentinel_words).sum()


def test_expansion_equals_the_host_layout(hals, recs):
    """on a real program the group is the one WitnessGenerator::new's host transposition makes"""
    import risc0_amd as r
    for rec in recs.values():
        with r.RecursionProgram.create(hals["poseidon2"], rec.po2, rec.code) as prog:
            assert np.array_equal(prog.ctrl(), rec.ctrl)
        mont = np.array([RP.enc(int(x)) for x in rec.code], dtype=np.uint32)
        with r.RecursionProgram.create(hals["poseidon2"], rec.po2, mont, form=r.CODE_MONTGOMERY) as prog:
            assert np.array_equal(prog.ctrl(), rec.ctrl)


# ---- the control id ---------------------------------------------------------------------------
@pytest.mark.parametrize("suite", ["poseidon2", "sha-256", "poseidon254"])
def test_control_id(hals, recs, suite):
    """the handle's control id is the code root r0hip_verify_seal reports for a keyed seal on the
    same control group, and the root of r0hip_merkle_tree over the per-op pipeline
    (compute_control_id_inner: interpolate, zk shift, expand + evaluate, tree)"""
    import risc0_amd as r
    hal, rec = hals[suite], recs["a"]
    n = 1 << rec.po2
    with r.RecursionProgram.create(hal, rec.po2, rec.code) as prog:
        cid = prog.info()[3]
        assert prog.info()[4] == 4 * (23 * n + 23 * n + 92 * n) + 64 * 4 * n
    seal, _mix = _keyed(r, hal, rec, 5)
    po2, root = r.verify_seal("recursion", hal.suite, seal, return_code_root=True)
    assert po2 == rec.po2
    assert np.array_equal(cid, root)
    coeffs = hal.copy_from_elem("coeffs", rec.ctrl)
    hal.batch_interpolate_ntt(coeffs, 23)
    hal.zk_shift(coeffs, 23)
    ev = hal.alloc_elem("evaluated", 23 * 4 * n)
    hal.batch_expand_into_evaluate_ntt(ev, coeffs, 23, 2)
    nodes = hal.alloc_digest("nodes", 2 * 4 * n)
    hal.merkle_tree(nodes, ev, 4 * n)
    assert np.array_equal(nodes.to_numpy().reshape(-1)[8:16], cid)
    for b in (coeffs, ev, nodes):
        b.free()


# ---- seal parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("suite, which, streams", [
    ("poseidon2", "a", 1), ("poseidon2", "d", 1), ("sha-256", "a", 1), ("sha-256", "d", 1), ("poseidon254", "a", 1),
    ("poseidon2", "d", 2)])
def test_seal_equals_the_keyed_call(hals, recs, suite, which, streams):
    """po2 11 (coefficients put in natural order) and 13 (left bit-reversed); one case with two
    proof streams set on the thread, where the handle has no code commit left to fork"""
    import risc0_amd as r
    hal, rec = hals[suite], recs[which]
    stream_id = (0x0BADC0DE << 32) | rec.po2
    want = _keyed(r, hal, rec, stream_id)
    with r.RecursionProgram.create(hal, rec.po2, rec.code) as prog:
        if streams == 1:
            got = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, stream_id)
        else:
            with hal.proof_streams(streams):
                got = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, stream_id)
    assert _same(got, want)
    assert r.verify_seal("recursion", hal.suite, got[0]) == rec.po2


@pytest.fixture(scope="module")
def two_inputs():
    """one program that reads its input through the IOP (rows fixed, values free) and two inputs
    of it, A and B: another IOP stream and another WOM under the same control group"""
    po2 = 13
    b = RP.Builder(np.random.default_rng(11))
    for _ in range(20):
        b.block_iop()
        b.block_arith()
    prog, inp_a = b.finish()
    inp_b = [int(x) for x in np.random.default_rng(99).integers(0, P, len(inp_a))]
    out = []
    for inp in (inp_a, inp_b):
        t = _Rec.__new__(_Rec)
        t.po2, t.prog, t.code, t.ctrl = po2, prog, prog.encoded(), RP.ctrl_group(prog, po2)
        t.wom, t.cyc, t.iops = RP.trace_arrays(RP.preflight(prog, inp))
        out.append(t)
    assert not np.array_equal(out[0].wom, out[1].wom) and not np.array_equal(out[0].iops, out[1].iops)
    return out


def test_the_handle_is_read_only(hals, two_inputs):
    """input A, then input B, then A again from one handle: seals 1 and 3 are equal, every seal
    is the keyed call's, and the control id and the control group are what they were"""
    import risc0_amd as r
    hal = hals["poseidon2"]
    ra, rb = two_inputs
    with r.RecursionProgram.create(hal, ra.po2, ra.code) as prog:
        cid0, ctrl0 = prog.info()[3].copy(), prog.ctrl()
        s1 = prog.prove(ra.wom, ra.cyc, ra.iops, KEY, 1)
        s2 = prog.prove(rb.wom, rb.cyc, rb.iops, KEY, 2)
        s3 = prog.prove(ra.wom, ra.cyc, ra.iops, KEY, 1)
        assert np.array_equal(prog.info()[3], cid0) and np.array_equal(prog.ctrl(), ctrl0)
    assert np.array_equal(ctrl0, ra.ctrl)
    assert _same(s1, s3)
    assert not np.array_equal(s1[0], s2[0])
    assert _same(s1, _keyed(r, hal, ra, 1))
    assert _same(s2, _keyed(r, hal, rb, 2))
    assert r.verify_seal("recursion", hal.suite, s2[0]) == ra.po2


def test_two_handles_alive_together(hals, recs):
    """one suite, po2 11 and 12, proofs interleaved: a handle that had borrowed pooled blocks
    would see them reused by the other's proofs"""
    import risc0_amd as r
    hal, ra, rc = hals["poseidon2"], recs["a"], recs["c"]
    want = {("a", 1): _keyed(r, hal, ra, 1), ("c", 2): _keyed(r, hal, rc, 2), ("a", 3): _keyed(r, hal, ra, 3),
            ("c", 4): _keyed(r, hal, rc, 4)}
    with r.RecursionProgram.create(hal, ra.po2, ra.code) as pa, r.RecursionProgram.create(hal, rc.po2, rc.code) as pc:
        for (name, sid), ref in want.items():
            prog, rec = (pa, ra) if name == "a" else (pc, rc)
            assert _same(prog.prove(rec.wom, rec.cyc, rec.iops, KEY, sid), ref), (name, sid)
        assert np.array_equal(pa.ctrl(), ra.ctrl) and np.array_equal(pc.ctrl(), rc.ctrl)


def test_four_threads_prove_from_one_handle(hals, recs):
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs["c"]
    want = [_keyed(r, hal, rec, 10 + i) for i in range(4)]
    got, errors = [None] * 4, []
    with r.RecursionProgram.create(hal, rec.po2, rec.code) as prog:
        def run(i):
            try:
                got[i] = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 10 + i)
            except Exception as e:  # noqa: BLE001
                errors.append((i, repr(e)))
        threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(WAIT_S)
            assert not t.is_alive(), "a proving thread did not finish"
    assert not errors, errors
    for i in range(4):
        assert _same(got[i], want[i]), i


# ---- the worker -------------------------------------------------------------------------------
def _drain(w, count):
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        assert res[0] not in got, f"ticket {res[0]} returned twice"
        got[res[0]] = res
    return got


def test_worker_kind_3(hals, recs):
    """in_flight 3, verification on, a fixed key; eight jobs at once: four of kind 3 over two
    handles, two of kind 1 on the same programs, one rv32im trace job, one kind 3 with a wrong
    digest in its allow-list"""
    import risc0_amd as r
    hal, ra, rc = hals["poseidon2"], recs["a"], recs["c"]
    t = T.random_trace(13, 250, seed=21)
    cyc, tx = t.arrays()
    idx, off, val = W.injector_arrays(t)
    tjob = r.TraceJob(W.global_words(t), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())
    with r.RecursionProgram.create(hal, ra.po2, ra.code) as pa, r.RecursionProgram.create(hal, rc.po2, rc.code) as pc:
        progs = {"a": (pa, ra), "c": (pc, rc)}
        order = [("p", "a"), ("p", "c"), ("k", "a"), ("t", None), ("p", "a"), ("k", "c"), ("bad", "c"), ("p", "c")]
        with r.Worker(hal, max_po2=13, in_flight=3, verify=True, noise_key=KEY) as w:
            # refused without queuing: another suite, another po2, a trace of another length, no handle
            with pytest.raises(r.R0HipError, match="suite"):
                w.submit_recursion_program(pa, ra.wom, ra.cyc, ra.iops, suite="sha-256")
            with pytest.raises(r.R0HipError, match="po2"):
                w.submit_recursion_program(pa, ra.wom, ra.cyc, ra.iops, po2=12)
            with pytest.raises(r.R0HipError, match="n_cycles"):
                w.submit_recursion_program(pa, ra.wom, ra.cyc[:-1], ra.iops)
            with pytest.raises(r.R0HipError, match="program is NULL"):
                pj = r.WorkerProgramJobStruct()  # program left NULL
                pj.job.kind, pj.job.po2, pj.job.suite = 3, 11, hal.suite
                w._submit(pj.job, 20, pj)
            assert w.outstanding() == 0 and w.wait(0) is None
            for i, (kind, name) in enumerate(order):
                if kind == "t":
                    ticket = w.submit_trace(tjob, 13)
                elif kind == "k":
                    prog, rec = progs[name]
                    ticket = w.submit_recursion(rec.po2, rec.ctrl, rec.wom, rec.cyc, rec.iops,
                                                code_roots=prog.info()[3])
                else:
                    prog, rec = progs[name]
                    roots = np.arange(8, dtype=np.uint32) if kind == "bad" else None
                    ticket = w.submit_recursion_program(prog, rec.wom, rec.cyc, rec.iops, code_roots=roots)
                assert ticket == i
            # a handle with jobs outstanding cannot be destroyed
            with pytest.raises(r.R0HipError, match="in use"):
                pa.close()
            got = _drain(w, len(order))
            assert w.wait(0) is None
        # every job was handed back: the handles are free again (the `with` closes them)
        for i, (kind, name) in enumerate(order):
            ticket, seal, mix, err, verify_ms, prove_ms = got[i]
            if kind == "bad":
                assert err is not None and err.startswith("receipt verification failed: "), err
            else:
                assert err is None, (i, err)
            if kind == "t":
                continue
            prog, rec = progs[name]
            assert _same((seal, mix), prog.prove(rec.wom, rec.cyc, rec.iops, KEY, ticket)), (i, kind)
            assert _same((seal, mix), _keyed(r, hal, rec, ticket)), (i, kind)
        single = r.prove_segment_trace(hal, 13, tjob.glob, tjob.index, tjob.offsets, tjob.values, tjob.cycles,
                                       tjob.txns, t.table_split_cycle, bigint=t.bigint_array(),
                                       bigint_records=t.bigint_records())
        assert _same((got[3][1], got[3][2]), single)
    # a kind-3 and a kind-1 job of the same input and ticket give one seal: run the pair again in
    # two workers, where both take ticket 0
    with r.RecursionProgram.create(hal, ra.po2, ra.code) as pa:
        with r.Worker(hal, max_po2=11, in_flight=1, verify=True, noise_key=KEY) as w:
            with r.RecursionProgram.create(hal, rc.po2, rc.code) as pc:
                with pytest.raises(r.R0HipError, match="po2 12 above the worker's max_po2 11"):
                    w.submit_recursion_program(pc, rc.wom, rc.cyc, rc.iops)
            assert w.submit_recursion_program(pa, ra.wom, ra.cyc, ra.iops) == 0
            s3 = _drain(w, 1)[0]
        with r.Worker(hal, max_po2=11, in_flight=1, verify=True, noise_key=KEY) as w:
            assert w.submit_recursion(ra.po2, ra.ctrl, ra.wom, ra.cyc, ra.iops) == 0
            s1 = _drain(w, 1)[0]
    assert s3[3] is None and s1[3] is None
    assert _same((s3[1], s3[2]), (s1[1], s1[2]))


# ---- memory -----------------------------------------------------------------------------------
def test_memory(hals, recs):
    """ten proofs after a warm-up make no hipMalloc; device_bytes is the four buffers; after
    destroy, worker destroy and trim the live bytes are back where they started"""
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs["c"]
    n = 1 << rec.po2
    r.trim()
    before = r.mem_stats()["live"]
    prog = r.RecursionProgram.create(hal, rec.po2, rec.code)
    dev_bytes = prog.info()[4]
    assert dev_bytes == 4 * (23 * n + 23 * n + 92 * n) + 64 * 4 * n
    assert r.mem_stats()["live"] >= before + dev_bytes
    prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 0)
    mallocs = r.mem_stats()["mallocs"]
    for i in range(10):
        prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 1 + i)
    assert r.mem_stats()["mallocs"] == mallocs
    with r.Worker(hal, max_po2=rec.po2, in_flight=2, verify=True, noise_key=KEY) as w:
        w.submit_recursion_program(prog, rec.wom, rec.cyc, rec.iops)
        w.submit_recursion_program(prog, rec.wom, rec.cyc, rec.iops)
        got = _drain(w, 2)
        assert all(res[3] is None for res in got.values())
    prog.close()
    r.trim()
    assert r.mem_stats()["live"] == before


# ---- a failing witness ------------------------------------------------------------------------
def test_a_failing_witness_leaves_the_handle_usable(hals, recs):
    """a hole in the write-once memory fails the sorted-memory check (the reference's eqz at
    zirgen/circuit/recursion/wom.cpp:74) from the handle as from the keyed call; a handle that
    saw a failed proof still gives the right seal"""
    import risc0_amd as r
    hal, po2 = hals["poseidon2"], 11
    b = RP.Builder(np.random.default_rng(5))
    b.consts([(3, 0), (4, 0)])
    b.next += 1
    b.consts([(5, 0)])
    bad_prog, inp = b.finish()
    wom, cyc, iops = RP.trace_arrays(RP.preflight(bad_prog, inp))
    d_ctrl = hal.copy_from_elem("ctrl", RP.ctrl_group(bad_prog, po2))
    with pytest.raises(r.R0HipError, match="wom.cpp:74") as keyed_err:
        r.prove_recursion_keyed(hal, po2, d_ctrl, wom, cyc, iops, KEY, 0)
    d_ctrl.free()
    with r.RecursionProgram.create(hal, po2, bad_prog.encoded()) as prog:
        with pytest.raises(r.R0HipError, match="wom.cpp:74") as handle_err:
            prog.prove(wom, cyc, iops, KEY, 0)
    assert str(handle_err.value) == str(keyed_err.value)
    # a good program handed a trace with a wrong WOM value, then its own trace, from one handle
    rec = recs["a"]
    broken = rec.wom.copy()
    broken[1, 0] = (int(broken[1, 0]) + 1) % P
    d_ctrl = hal.copy_from_elem("ctrl", rec.ctrl)
    with pytest.raises(r.R0HipError, match="eqz failed at: zirgen/circuit/recursion/wom.cpp:") as keyed_err:
        r.prove_recursion_keyed(hal, rec.po2, d_ctrl, broken, rec.cyc, rec.iops, KEY, 9)
    d_ctrl.free()
    with r.RecursionProgram.create(hal, rec.po2, rec.code) as prog:
        with pytest.raises(r.R0HipError, match="eqz failed at: zirgen/circuit/recursion/wom.cpp:") as handle_err:
            prog.prove(broken, rec.cyc, rec.iops, KEY, 9)
        assert str(handle_err.value) == str(keyed_err.value)
        assert _same(prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 9), _keyed(r, hal, rec, 9))
        assert np.array_equal(prog.ctrl(), rec.ctrl)
