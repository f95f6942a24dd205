"""Recursion proofs from a resident program and its input words on the device
(r0hip_prove_recursion_program_input, r0hip_recursion_program_prepare_input, worker kind 4): the
seal and mix word for word against r0hip_prove_recursion_program on the arrays of the Python
preflight, the validity equation, the returned output; the plan's boundaries (more than 256 runs,
a single bucket); a handle used again and from two threads, its memory; the worker with kinds 3
and 4 mixed, a job whose input fails, refusals at submit. Programs are
recursion_program.satisfying_witness at po2 11 and 13."""
import threading

import numpy as np
import pytest

import recursion_program as RP

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not RP.available(), reason="oracle/_ref/libref_recursion.so is not built")]

P = RP.P
WAIT_S = 120.0
KEY = np.array([0x03020100, 0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xFFFFFFFF],
               dtype=np.uint32)


@pytest.fixture(scope="module")
def hals():
    import risc0_amd as r
    return {s: r.HipHal(s) for s in ("poseidon2", "sha-256", "poseidon254")}


class _Rec:
    """a program, one input of it, and the Python preflight's arrays"""

    def __init__(self, po2, prog, inp, preflight=RP.preflight):
        self.po2, self.prog, self.input, self.code = po2, prog, list(inp), prog.encoded()
        pf = preflight(prog, inp)
        self.wom, self.cyc, self.iops = RP.trace_arrays(pf)
        self.output = [int(x) for x in pf.output]

    def with_input(self, inp):
        return _Rec(self.po2, self.prog, inp)


@pytest.fixture(scope="module")
def recs():
    """11 and 13: programs that fill their segment and satisfy the circuit"""
    out = {}
    for po2 in (11, 13):
        w = RP.satisfying_witness(8100 + po2, po2)
        out[po2] = _Rec(po2, w["program"], w["input"])
    return out


def _same(a, b):
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- seal equality ----------------------------------------------------------------------------
@pytest.mark.parametrize("suite, po2", [("poseidon2", 11), ("poseidon2", 13), ("sha-256", 11), ("sha-256", 13),
                                        ("poseidon254", 11)])
def test_seal_equals_the_proof_from_the_python_preflight(hals, recs, suite, po2):
    import risc0_amd as r
    hal, rec = hals[suite], recs[po2]
    stream_id = (0x0BADC0DE << 32) | po2
    with r.RecursionProgram.create(hal, po2, rec.code) as prog:
        want = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, stream_id)
        seal, mix, output = prog.prove_input(rec.input, KEY, stream_id)
        cid = prog.info()[3]
    assert _same((seal, mix), want)
    assert [int(x) for x in output] == rec.output and len(rec.output) > 0
    # the validity equation, and the handle's control id as the only allowed code root
    assert r.verify_seal("recursion", hal.suite, seal, code_roots=cid) == po2


def test_a_program_with_sha_compressions(hals):
    """the SHA macro ops: the seal is the one from the restated preflight's arrays, the validity
    equation holds, and RecursionProgram.preflight gives those arrays"""
    import recursion_input_programs as IP
    import recursion_sha_program as S
    import risc0_amd as r
    hal = hals["poseidon2"]
    rec = _Rec(11, *IP.CASES["sha_shorts"](), preflight=S.preflight)
    with r.RecursionProgram.create(hal, 11, rec.code) as prog:
        want = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 9)
        seal, mix, output = prog.prove_input(rec.input, KEY, 9)
        cid = prog.info()[3]
        wom, cyc, iops, _out = prog.preflight(rec.input)
    assert _same((seal, mix), want)
    assert np.array_equal(wom, rec.wom) and np.array_equal(iops, rec.iops)
    assert np.array_equal(cyc, np.array(rec.cyc, dtype=np.uint32).reshape(-1, 2))
    assert r.verify_seal("recursion", hal.suite, seal, code_roots=cid) == 11


# ---- the plan's boundaries ---------------------------------------------------------------------
def test_more_than_256_runs(hals, recs):
    """the po2-13 program's runs cross workgroup boundaries of the run kernels, and every bucket
    the program's blocks give is used"""
    import risc0_amd as r
    rec = recs[13]
    with r.RecursionProgram.create(hals["poseidon2"], 13, rec.code) as prog:
        assert not prog.input_info().prepared
        prog.prepare_input()
        info = prog.input_info()
        assert info.prepared and info.n_runs > 256 and sum(info.bucket_runs) == info.n_runs
        assert sum(1 for k in info.bucket_runs if k) >= 2
        cyc = np.array(rec.cyc, dtype=np.uint32).reshape(-1, 2)
        assert info.n_runs == 1 + int(np.count_nonzero(cyc[1:, 1]))
        assert (info.n_wom, info.n_iops, info.n_output) == (rec.wom.shape[0], rec.iops.shape[0], len(rec.output))
        assert info.n_input == len(rec.input)
        assert info.plan_device_bytes >= 4 * (2 * info.n_runs + 1 + len(rec.cyc))


def test_a_single_bucket(hals):
    """302 macro rows and nothing else (wom_init, nops, wom_fini): one bucket holds every run, the
    other eight launches are empty, the runs still cross a workgroup boundary, and the write-once
    memory and the IOP are empty"""
    import risc0_amd as r
    hal = hals["poseidon2"]
    rows = RP.Program()
    rows.macro("wom_init")
    for _ in range(300):
        rows.macro("nop")
    rows.macro("wom_fini", 1)
    rec = _Rec(11, rows, [])
    assert rec.wom.shape[0] == 0 and rec.iops.shape[0] == 0
    with r.RecursionProgram.create(hal, 11, rec.code) as prog:
        want = prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 3)
        got = prog.prove_input([], KEY, 3)
        info = prog.input_info()
    assert info.n_runs == 302 and sorted(info.bucket_runs)[-1] == 302 and sorted(info.bucket_runs)[-2] == 0
    assert _same(got[:2], want) and got[2].size == 0
    assert r.verify_seal("recursion", hal.suite, got[0], check_validity=False) == 11


# ---- one handle, many proofs -------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_inputs():
    """one program whose rows read the input through the IOP, and two inputs of it"""
    b = RP.Builder(np.random.default_rng(11))
    for _ in range(20):
        b.block_iop()
        b.block_arith()
    prog, inp_a = b.finish()
    inp_b = [int(x) for x in np.random.default_rng(99).integers(0, P, len(inp_a))]
    ra = _Rec(13, prog, inp_a)
    rb = ra.with_input(inp_b)
    assert not np.array_equal(ra.wom, rb.wom) and not np.array_equal(ra.iops, rb.iops)
    return ra, rb


def test_a_b_a_from_one_handle(hals, two_inputs):
    import risc0_amd as r
    hal = hals["poseidon2"]
    ra, rb = two_inputs
    with r.RecursionProgram.create(hal, ra.po2, ra.code) as prog:
        s1 = prog.prove_input(ra.input, KEY, 1)
        s2 = prog.prove_input(rb.input, KEY, 2)
        s3 = prog.prove_input(ra.input, KEY, 1)
        assert _same(s1[:2], prog.prove(ra.wom, ra.cyc, ra.iops, KEY, 1))
        assert _same(s2[:2], prog.prove(rb.wom, rb.cyc, rb.iops, KEY, 2))
    assert _same(s1[:2], s3[:2]) and not np.array_equal(s1[0], s2[0])
    assert [int(x) for x in s1[2]] == ra.output and [int(x) for x in s2[2]] == rb.output


def test_two_threads_prove_from_one_handle(hals, two_inputs):
    """the first proofs race to make the plan"""
    import risc0_amd as r
    hal = hals["poseidon2"]
    pair = two_inputs
    got, errors = [None, None], []
    with r.RecursionProgram.create(hal, pair[0].po2, pair[0].code) as prog:
        want = [prog.prove(t.wom, t.cyc, t.iops, KEY, 20 + i) for i, t in enumerate(pair)]

        def run(i):
            try:
                got[i] = prog.prove_input(pair[i].input, KEY, 20 + i)
            except Exception as e:  # noqa: BLE001
                errors.append((i, repr(e)))
        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(WAIT_S)
            assert not t.is_alive(), "a proving thread did not finish"
    assert not errors, errors
    for i in range(2):
        assert _same(got[i][:2], want[i]), i


def test_memory_and_info(hals, recs):
    """info's device_bytes is what it was before the plan; after destroy and trim the live bytes
    are back where they started; a preflight failure leaves the handle usable"""
    import risc0_amd as r
    hal, rec = hals["poseidon2"], recs[11]
    n = 1 << rec.po2
    r.trim()
    before = r.mem_stats()["live"]
    prog = r.RecursionProgram.create(hal, rec.po2, rec.code)
    dev_bytes = prog.info()[4]
    assert dev_bytes == 4 * (23 * n + 23 * n + 92 * n) + 64 * 4 * n
    live = r.mem_stats()["live"]
    prog.prepare_input()
    prog.prepare_input()  # idempotent
    info = prog.input_info()
    assert prog.info()[4] == dev_bytes
    assert r.mem_stats()["live"] >= live + info.plan_device_bytes
    with pytest.raises(r.R0HipError, match=r"input exhausted: .* \(cycle \d+\)$"):
        prog.prove_input(rec.input[:-1], KEY, 0)
    assert _same(prog.prove_input(rec.input, KEY, 5)[:2], prog.prove(rec.wom, rec.cyc, rec.iops, KEY, 5))
    prog.close()
    r.trim()
    assert r.mem_stats()["live"] == before


# ---- the worker --------------------------------------------------------------------------------
def _drain(w, count):
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        assert res[0] not in got, f"ticket {res[0]} returned twice"
        got[res[0]] = res
    return got


@pytest.fixture(scope="module")
def eq_program():
    """a program that checks one input word against a constant (EQ): the good input and a bad one"""
    b = RP.Builder(np.random.default_rng(31))
    b.block_arith()
    b.micro([(RP.READ_IOP_HEADER, 1, 2 * 1, 0)])
    got = b.micro([(RP.READ_IOP_BODY, 0, 0, 0)])[0]
    want = b.consts([(5, 0)])[0]
    b.micro([(RP.EQ, got, want, 0)])
    b.input.append(RP.enc(5))
    b.block_iop()
    prog, inp = b.finish()
    good = _Rec(11, prog, inp)
    bad = list(inp)
    bad[0] = RP.enc(6)
    return good, bad


def test_worker_kinds_3_and_4(hals, recs, eq_program):
    import risc0_amd as r
    hal, r11, r13 = hals["poseidon2"], recs[11], recs[13]
    good, bad_input = eq_program
    with r.RecursionProgram.create(hal, 11, r11.code) as p11, r.RecursionProgram.create(hal, 13, r13.code) as p13, \
            r.RecursionProgram.create(hal, 11, good.code) as peq:
        progs = {"11": (p11, r11), "13": (p13, r13), "eq": (peq, good)}
        order = [(4, "13"), (3, "13"), (4, "11"), (4, "bad"), (3, "11"), (4, "eq"), (4, "13"), (3, "eq")]
        with r.Worker(hal, max_po2=13, in_flight=2, verify=True, noise_key=KEY) as w:
            with pytest.raises(r.R0HipError, match="suite"):
                w.submit_recursion_input(p11, r11.input, suite="sha-256")
            with pytest.raises(r.R0HipError, match="po2"):
                w.submit_recursion_input(p11, r11.input, po2=12)
            with pytest.raises(r.R0HipError, match="program is NULL"):
                ij = r.WorkerInputJobStruct()
                ij.job.kind, ij.job.po2, ij.job.suite = 4, 11, hal.suite
                w._submit(ij.job, 20, ij)
            assert w.outstanding() == 0 and w.wait(0) is None
            for i, (kind, name) in enumerate(order):
                prog, rec = progs["eq" if name == "bad" else name]
                if kind == 3:
                    ticket = w.submit_recursion_program(prog, rec.wom, rec.cyc, rec.iops)
                else:
                    ticket = w.submit_recursion_input(prog, bad_input if name == "bad" else rec.input)
                assert ticket == i
            # a queued job holds its handle: destroy is refused and frees nothing
            with pytest.raises(r.R0HipError, match="in use"):
                p13.close()
            got = _drain(w, len(order))
            assert w.wait(0) is None
            outputs = {i: w.output(i) for i, (kind, name) in enumerate(order) if kind == 4}
        for i, (kind, name) in enumerate(order):
            ticket, seal, mix, err, _verify_ms, _prove_ms = got[i]
            if name == "bad":
                assert err is not None and "Equality check failed: Expecting [6, 0, 0, 0] == [5, 0, 0, 0] (cycle" in err
                continue
            assert err is None, (i, err)  # verified by the worker, the validity equation included
            prog, rec = progs[name]
            # the kind-3 seal of the same input and ticket (test_worker_kind_3 pins kind 3 to this call)
            assert _same((seal, mix), prog.prove(rec.wom, rec.cyc, rec.iops, KEY, ticket)), (i, kind)
            if kind == 4:
                assert [int(x) for x in outputs[i]] == rec.output, i
    # a kind-4 and a kind-3 job of one input in two workers, where both take ticket 0
    with r.RecursionProgram.create(hal, 11, r11.code) as p11:
        with r.Worker(hal, max_po2=11, in_flight=2, verify=True, noise_key=KEY) as w:
            with r.RecursionProgram.create(hal, 13, r13.code) as p13:
                with pytest.raises(r.R0HipError, match="po2 13 above the worker's max_po2 11"):
                    w.submit_recursion_input(p13, r13.input)
            assert w.submit_recursion_input(p11, r11.input) == 0
            s4 = _drain(w, 1)[0]
        with r.Worker(hal, max_po2=11, in_flight=2, verify=True, noise_key=KEY) as w:
            assert w.submit_recursion_program(p11, r11.wom, r11.cyc, r11.iops) == 0
            s3 = _drain(w, 1)[0]
    assert s4[3] is None and s3[3] is None
    assert _same((s4[1], s4[2]), (s3[1], s3[2]))
