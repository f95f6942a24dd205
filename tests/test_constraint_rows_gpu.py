"""The constraint-rows check on the device (r0hip_constraint_rows, r0hip_set_witness_check,
r0hip_worker_set_witness_check) against the reference's own compiled poly_fp
(oracle.poly_fp_at_taps on each row's gathered taps, constraint_rows_ref.PolyFp) and the Python
restatement of the term walk (constraint_rows_ref.first_term):
  * recursion po2 11: a satisfying witness gives zeros on all 2048 rows, equal to the oracle and
    to RP.row_constraints; then one cell changed in data row 0, data row N-1 (the wrap), the
    first ZK row, accum, ctrl, global and mix, every row's value and the whole report compared;
  * both circuits at po2 2, 5, 8 on groups that satisfy nothing, with the worst-case words;
  * rv32im po2 13 on the smallest built trace (device witness generation and accumulation);
  * the provers with the thread mode on and off, and the worker with its switch on and off.
The oracle's value of a row is a pure function of the row's taps, mix, global and poly_mix, so
PolyFp evaluates each distinct row once; no row is left out of any comparison."""
import numpy as np
import pytest

import constraint_rows_ref as CR
import recursion_program as RP
import rv32im_trace as T
import rv32im_witgen_ref as W
from ec_extreme import extreme_inputs

pytestmark = pytest.mark.gpu

P = CR.P
INVALID = 0xFFFFFFFF
WAIT_S = 120.0
POLY_MIX = np.array([CR.enc(x) for x in (7, 11, 13, 17)], np.uint32)
KEY = np.array([0x03020100, 0x9E3779B9, 0x7F4A7C15, 0xDEADBEEF, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0xFFFFFFFF],
               dtype=np.uint32)
MESSAGE = "constraint check failed: {k} of {n} rows, first at cycle {r} (term {t})"


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def _plus_one(word):
    return (int(word) + CR.enc(1)) % P


def _rows(r, hal, name, po2, groups, mix, glob, poly_mix=POLY_MIX, want_out=True):
    """r0hip_constraint_rows on host copies of the groups (accum, code, data): (values (n, 4), report)"""
    n = 1 << po2
    bufs = [hal.copy_from_elem(k, v) for k, v in zip(("accum", "code", "data", "mix", "global"), (*groups, mix, glob))]
    out = hal.alloc_extelem("rows", n) if want_out else None
    rep = r.constraint_rows(name, po2, bufs[1], bufs[2], bufs[0], bufs[3], bufs[4], poly_mix, out)
    vals = out.to_numpy().reshape(n, 4) if want_out else None
    for b in bufs + ([out] if want_out else []):
        b.free()
    return vals, rep


def _expect(fp, name, po2, groups, mix, glob):
    """the oracle's values of every row, the report they imply and the restated walk's term"""
    taps = CR.gather_taps(name, groups, po2)
    vals = fp.rows(taps, mix, glob, POLY_MIX)
    rep = CR.report_of(vals)
    rep["first_term"] = (None if rep["first_row"] is None else
                         CR.first_term(name, taps[rep["first_row"]], mix, glob, POLY_MIX))
    return vals, rep


def _compare(r, hal, fp, name, po2, groups, mix, glob, what):
    want_vals, want = _expect(fp, name, po2, groups, mix, glob)
    vals, rep = _rows(r, hal, name, po2, groups, mix, glob)
    bad = np.nonzero((vals != want_vals).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ from the reference's poly_fp, first row {bad[0]}"
    assert rep == want, f"{what}: report {rep}, the oracle's nonzero set gives {want}"
    return want


# ---- recursion, po2 11 --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec(oracle):
    if not RP.available():
        pytest.skip("oracle/_ref not built")
    w = CR.recursion_witness(3100, 11, 3101)
    w["fp"] = CR.PolyFp(oracle, "recursion")
    return w


def test_recursion_satisfying_witness_is_zero_on_every_row(hal, rec):
    import risc0_amd as r
    po2, n = 11, 2048
    want = _compare(r, hal, rec["fp"], "recursion", po2, rec["groups"], rec["mix"], rec["glob"], "satisfying witness")
    assert want["bad_rows"] == 0
    vals, rep = _rows(r, hal, "recursion", po2, rec["groups"], rec["mix"], rec["glob"])
    assert not vals.any() and rep == {"bad_rows": 0, "first_row": None, "first_term": None, "rows": []}
    acc, ctrl, data = rec["groups"]
    plain = RP.row_constraints(ctrl, data, acc, rec["glob"], rec["mix"], po2, poly_mix=(7, 11, 13, 17))
    assert np.array_equal(vals, np.array([CR.enc(x) for x in plain.T.reshape(-1)], np.uint32).reshape(n, 4))
    # without d_out, and with a poly_mix of the OS's, the report is the same
    assert _rows(r, hal, "recursion", po2, rec["groups"], rec["mix"], rec["glob"], want_out=False)[1] == rep
    assert _rows(r, hal, "recursion", po2, rec["groups"], rec["mix"], rec["glob"], poly_mix=None)[1] == rep


# (group, column, row) of the changed cell; rows relative to n where negative. The ZK rows and
# the row before row 0 carry no live constraint in this circuit (their selectors are zero), so the
# oracle's nonzero set for those two is empty and the values stay zero: the comparison with the
# oracle holds all the same, and the wrap itself is exercised by the worst-case test below, where
# every `back` wraps.
REC_CELLS = [("data row 0", 2, 0, 0), ("data row N-1", 2, 0, -1), ("first ZK row", 2, 0, -1024),
             ("accum cell", 0, 3, 100), ("ctrl cell", 1, 3, 50)]


@pytest.mark.parametrize("what, g, col, row", REC_CELLS, ids=[c[0].replace(" ", "_") for c in REC_CELLS])
def test_recursion_one_changed_cell(hal, rec, what, g, col, row):
    import risc0_amd as r
    n = 2048
    groups = [a.copy() for a in rec["groups"]]
    i = col * n + row % n
    groups[g][i] = _plus_one(groups[g][i])
    want = _compare(r, hal, rec["fp"], "recursion", 11, groups, rec["mix"], rec["glob"], what)
    if what in ("data row 0", "accum cell", "ctrl cell"):
        assert want["bad_rows"] >= 1 and want["first_row"] == row and want["first_term"] is not None, want


@pytest.mark.parametrize("what, index", [("global", 5), ("mix", 7)])
def test_recursion_one_changed_word(hal, rec, what, index):
    import risc0_amd as r
    mix, glob = rec["mix"].copy(), rec["glob"].copy()
    arr = glob if what == "global" else mix
    arr[index] = _plus_one(arr[index])
    want = _compare(r, hal, rec["fp"], "recursion", 11, rec["groups"], mix, glob, what + " word")
    assert want["bad_rows"] >= 1, want
    if what == "mix":  # hundreds of rows: the list holds the first 16, ascending
        assert want["bad_rows"] > 16 and len(want["rows"]) == 16


# ---- worst-case words ---------------------------------------------------------------------------
def _special_groups(d, n, seed):
    """random canonical words with the worst-case ones among them: the Montgomery words 0, 1 and
    p - 1, and the values of ec_extreme's edge mix (0, 1, 2, p - 2, p - 1) as Montgomery words"""
    rng = np.random.default_rng(seed)
    special = np.array([0, 1, P - 1] + [CR.enc(x) for x in (0, 1, 2, P - 2, P - 1)], np.uint32)
    out = {}
    for k, size in (("accum", d["group_sizes"][0] * n), ("code", d["group_sizes"][1] * n),
                    ("data", d["group_sizes"][2] * n), ("mix", d["mix_size"]), ("global", d["output_size"])):
        a = rng.integers(0, P, size, dtype=np.uint64).astype(np.uint32)
        pick = rng.random(size) < 0.4
        a[pick] = rng.choice(special, int(pick.sum()))
        a[:min(size, special.size)] = special[:min(size, special.size)]
        out[k] = a
    return out


@pytest.mark.parametrize("po2", [2, 5, 8])
@pytest.mark.parametrize("name", ["rv32im", "recursion"])
def test_worst_case_words_match_the_reference(hal, oracle, name, po2):
    """groups that satisfy nothing: every row's value is the reference's poly_fp word for word.
    At these sizes most taps wrap (back up to 68 against 4, 32 and 256 rows)."""
    import risc0_amd as r
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    d = oracle.load_circuit_json(name)
    n = 1 << po2
    fp = CR.PolyFp(oracle, name)
    cases = [("random and special words", _special_groups(d, n, 40 + po2), POLY_MIX)]
    for mode in ("all_pm1", "edge_mix"):
        plain, pm = extreme_inputs(d, mode, po2 - 2)  # buffers of 4 << (po2 - 2) = n rows
        cases.append((mode, {k: np.array([CR.enc(x) for x in v], np.uint32) for k, v in plain.items()},
                      np.array([CR.enc(x) for x in pm], np.uint32)))
    for what, b, pm in cases:
        groups = (b["accum"], b["code"], b["data"])
        want = fp.rows(CR.gather_taps(name, groups, po2), b["mix"], b["global"], pm)
        vals, rep = _rows(r, hal, name, po2, groups, b["mix"], b["global"], poly_mix=pm)
        assert np.array_equal(vals, want), f"{what}: rows {np.nonzero((vals != want).any(axis=1))[0][:8]} differ"
        exp = CR.report_of(want)
        assert (rep["bad_rows"], rep["first_row"], rep["rows"]) == (exp["bad_rows"], exp["first_row"], exp["rows"])
        assert exp["bad_rows"] > n // 2, "these groups should satisfy next to nothing"


# ---- rv32im, po2 13 -----------------------------------------------------------------------------
def _trace_job(r, t):
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    return r.TraceJob(t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())


def _rv_accumulate(r, hal, t, d_data, d_glob, mix, n):
    """WitnessGenerator::accum per op (witgen/mod.rs:178-221) on the device; returns the host copy"""
    accum = hal.alloc_elem_init("accum", 103 * n, INVALID)
    d_mix = hal.copy_from_elem("mix", mix)
    r.bigint_accum_inject(accum, n, mix, t.bigint_records())
    hal.rv32im_accum(d_data, accum, d_glob, d_mix, n, n)
    hal.eltwise_zeroize_elem(accum)
    out = accum.to_numpy()
    accum.free()
    d_mix.free()
    return out


@pytest.fixture(scope="module")
def rv(hal, oracle):
    """the smallest trace the builders make (200 cycles in a po2 13 segment): the witness by
    r0hip_rv32im_witgen, the accumulation by the hal under a fixed mix"""
    import risc0_amd as r
    if not W.RA.available():
        pytest.skip("oracle/_ref not built")
    po2, n = 13, 1 << 13
    t = T.random_trace(po2, 200, seed=0x5249534330)
    job = _trace_job(r, t)
    data = hal.alloc_elem_init("data", 211 * n, INVALID)
    glob = hal.copy_from_elem("global", job.glob)
    hal.scatter(data, job.index, job.offsets, job.values)
    r.rv32im_witgen(data, glob, job.cycles, job.txns, t.table_split_cycle, bigint=t.bigint_array())
    hal.eltwise_zeroize_elem(data)
    hal.eltwise_zeroize_elem(glob)
    mix = np.random.default_rng(3102).integers(1, P, 36, dtype=np.uint64).astype(np.uint32)
    acc = _rv_accumulate(r, hal, t, data, glob, mix, n)
    w = {"po2": po2, "trace": t, "job": job, "groups": (acc, np.zeros(n, np.uint32), data.to_numpy()),
         "glob": glob.to_numpy(), "mix": mix, "fp": CR.PolyFp(oracle, "rv32im")}
    data.free()
    glob.free()
    return w


def test_rv32im_trace_is_zero_on_every_row(hal, rv):
    """all 8192 rows are compared with the reference (none left out)"""
    import risc0_amd as r
    want = _compare(r, hal, rv["fp"], "rv32im", 13, rv["groups"], rv["mix"], rv["glob"], "rv32im trace")
    assert want == {"bad_rows": 0, "first_row": None, "first_term": None, "rows": []}


RV_CELLS = [("data row 0", 2, 0, 0), ("data row N-1", 2, 10, -1), ("data row N-1024", 2, 70, -1024),
            ("data mid row", 2, 40, 100), ("accum cell", 0, 8, 100)]


@pytest.mark.parametrize("what, g, col, row", RV_CELLS, ids=[c[0].replace(" ", "_") for c in RV_CELLS])
def test_rv32im_one_changed_cell(hal, rv, what, g, col, row):
    """every row is compared again (the changed cell's neighbourhood is re-evaluated by the
    oracle, the other rows' values are the unchanged witness's)"""
    import risc0_amd as r
    n = 1 << 13
    groups = [a.copy() for a in rv["groups"]]
    i = col * n + row % n
    groups[g][i] = _plus_one(groups[g][i])
    want = _compare(r, hal, rv["fp"], "rv32im", 13, groups, rv["mix"], rv["glob"], what)
    assert want["bad_rows"] >= 1 and want["first_row"] == row % n and want["first_term"] is not None, want


# ---- the provers with the mode on -------------------------------------------------------------
def _poke(r, buf, index, word):
    w = np.array([word], np.uint32)
    r.check(r.lib().r0hip_memcpy_h2d(buf.ptr + 4 * index, w.ctypes.data, 4))


def _rec_prove(r, hal, rec, data, accum):
    po2 = 11
    bufs = [hal.copy_from_elem(k, v) for k, v in (("ctrl", rec["w"]["ctrl"]), ("data", data), ("accum", accum),
                                                  ("global", rec["w"]["glob"]))]
    try:
        return r.prove_segment(hal, "recursion", po2, *bufs)
    finally:
        for b in bufs:
            b.free()


def test_fused_recursion_prove_segment(hal, rec):
    """r0hip_prove_segment on the recursion witness: the mix is the transcript's, so the accum
    group is the reference's accumulation under that mix (a first proof returns the mix)"""
    import risc0_amd as r
    po2, n = 11, 2048
    w = rec["w"]
    _, mix = _rec_prove(r, hal, rec, w["data"], rec["groups"][0])
    acc = RP.accumulate(w, mix, po2)
    seal_off, mix_off = _rec_prove(r, hal, rec, w["data"], acc)
    assert r.verify_seal("recursion", hal.suite, seal_off, check_validity=True) == po2
    assert "check_witness" not in r.last_profile()
    r.set_kernel_timing(True)
    _rec_prove(r, hal, rec, w["data"], acc)
    assert not [k for k in r.kernel_times() if "constraint" in k], r.kernel_times().keys()
    with hal.witness_check():
        _rec_prove(r, hal, rec, w["data"], acc)
        assert "constraint_rows" in r.kernel_times()
        r.set_kernel_timing(False)
        seal_on, mix_on = _rec_prove(r, hal, rec, w["data"], acc)
        assert "check_witness" in r.last_profile()
    assert np.array_equal(mix_on, mix_off) and np.array_equal(seal_on, seal_off)
    # one data cell changed: the mix changes with the data commitment, the accum group is the
    # unchanged witness's accumulation under it, and the oracle says which rows that violates
    bad = w["data"].copy()
    bad[0 * n + 7] = _plus_one(bad[7])
    _, mix_b = _rec_prove(r, hal, rec, bad, acc)
    acc_b = RP.accumulate(w, mix_b, po2)
    _, want = _expect(rec["fp"], "recursion", po2, (acc_b, w["ctrl"], bad), mix_b, w["glob"])
    assert want["bad_rows"] >= 1
    with hal.witness_check():
        with pytest.raises(r.R0HipError) as e:
            _rec_prove(r, hal, rec, bad, acc_b)
    assert str(e.value) == MESSAGE.format(k=want["bad_rows"], n=n, r=want["first_row"], t=want["first_term"])
    seal_b, _ = _rec_prove(r, hal, rec, bad, acc_b)  # mode off: a seal, which the receipt check rejects
    with pytest.raises(r.R0HipError):
        r.verify_seal("recursion", hal.suite, seal_b, check_validity=True)


def test_fused_rv32im_trace_and_prove_segment_accum(hal, rv):
    import risc0_amd as r
    po2, n = 13, 1 << 13
    t, job = rv["trace"], rv["job"]

    def trace():
        return r.prove_segment_trace(hal, po2, job.glob, job.index, job.offsets, job.values, job.cycles, job.txns,
                                     t.table_split_cycle, bigint=t.bigint_array(), bigint_records=t.bigint_records())
    seal_off, mix_off = trace()
    assert "check_witness" not in r.last_profile()
    with hal.witness_check():
        seal_on, mix_on = trace()
        assert "check_witness" in r.last_profile()
    assert np.array_equal(mix_on, mix_off) and np.array_equal(seal_on, seal_off)
    assert r.verify_seal("rv32im", hal.suite, seal_on, check_validity=True) == po2

    # r0hip_prove_segment_accum from the device witness with one data cell changed on the device
    acc0, code, data = rv["groups"]
    cell = 40 * n + 100

    def accum_proof(check):
        bufs = [hal.copy_from_elem("code", code), hal.copy_from_elem("data", data),
                hal.alloc_elem_init("accum", 103 * n, INVALID), hal.copy_from_elem("global", rv["glob"])]
        _poke(r, bufs[1], cell, _plus_one(data[cell]))
        try:
            with hal.witness_check(check):
                return r.prove_segment_accum(hal, "rv32im", po2, bufs[0], bufs[1], bufs[2], n, bufs[3], version=2,
                                             bigint=t.bigint_records())
        finally:
            for b in bufs:
                b.free()
    seal_b, mix_b = accum_proof(False)
    with pytest.raises(r.R0HipError):
        r.verify_seal("rv32im", hal.suite, seal_b, check_validity=True)
    bad = data.copy()
    bad[cell] = _plus_one(bad[cell])
    d_data, d_glob = hal.copy_from_elem("data", bad), hal.copy_from_elem("global", rv["glob"])
    acc_b = _rv_accumulate(r, hal, t, d_data, d_glob, mix_b, n)
    d_data.free()
    d_glob.free()
    _, want = _expect(rv["fp"], "rv32im", po2, (acc_b, code, bad), mix_b, rv["glob"])
    assert want["bad_rows"] >= 1
    with pytest.raises(r.R0HipError) as e:
        accum_proof(True)
    assert str(e.value) == MESSAGE.format(k=want["bad_rows"], n=n, r=want["first_row"], t=want["first_term"])


# ---- the worker -------------------------------------------------------------------------------
def _drain(w, count):
    got = {}
    for _ in range(count):
        res = w.wait(WAIT_S)
        assert res is not None, f"no job came back within {WAIT_S} s ({len(got)} of {count} returned)"
        got[res[0]] = res
    return got


def test_worker_switch(hal, oracle, rv):
    """Three jobs with the switch on give the seals of the same jobs with it off. Then a job the
    witness generation accepts and the constraints reject, between two good ones: a recursion
    job whose control group has one word set in a padding row (after the program, before the ZK
    rows). The witness generator and the accumulation run the program's rows only; the oracle,
    on the CPU, finds exactly the padding row violated. It fails alone, with the message."""
    import risc0_amd as r
    if not RP.available():
        pytest.skip("oracle/_ref not built")
    po2 = 11
    n = 1 << po2
    w2 = RP.satisfying_witness(3200, po2, max_rows=300)
    wom, cyc, iops = RP.trace_arrays(w2["preflight"])
    ctrl = w2["ctrl"]
    tjob = rv["job"]

    def submit_three(w, middle_ctrl):
        return [w.submit_trace(tjob, 13), w.submit_recursion(po2, middle_ctrl, wom, cyc, iops), w.submit_trace(tjob, 13)]
    seals = {}
    for on in (False, True):
        with r.Worker(hal, 13, in_flight=2, verify=True, noise_key=KEY) as w:
            w.set_witness_check(on)
            tickets = submit_three(w, ctrl)
            got = _drain(w, 3)
            assert all(got[k][3] is None for k in tickets), [got[k][3] for k in tickets]
            seals[on] = [got[k][1] for k in tickets]
    for a, b in zip(seals[False], seals[True]):
        assert a.size and np.array_equal(a, b)
    # the failing input, confirmed on the CPU with the oracle first
    bad_row = w2["work"] + 5
    bad_ctrl = ctrl.copy()
    bad_ctrl[1 * n + bad_row] = CR.enc(1)
    mix = np.random.default_rng(5).integers(1, P, 20, dtype=np.uint64).astype(np.uint32)
    fp = CR.PolyFp(oracle, "recursion")
    acc = RP.accumulate(w2, mix, po2)
    _, clean = _expect(fp, "recursion", po2, (acc, ctrl, w2["data"]), mix, w2["glob"])
    assert clean["bad_rows"] == 0
    _, want = _expect(fp, "recursion", po2, (acc, bad_ctrl, w2["data"]), mix, w2["glob"])
    assert (want["bad_rows"], want["first_row"]) == (1, bad_row)
    with r.Worker(hal, 13, in_flight=2, verify=True, noise_key=KEY) as w:
        w.set_witness_check(True)
        tickets = submit_three(w, bad_ctrl)
        structs = {int(e[0].ticket): e[0] for e in w._pending.values()}
        got = _drain(w, 3)
        assert got[tickets[1]][3] == MESSAGE.format(k=1, n=n, r=bad_row, t=want["first_term"])
        assert got[tickets[1]][1].size == 0 and structs[tickets[1]].verified == 0
        for k, ref in ((tickets[0], seals[True][0]), (tickets[2], seals[True][2])):
            assert got[k][3] is None and np.array_equal(got[k][1], ref)
        # switched off again, the same input is proved (and its receipt rejected): recorded at submit
        w.set_witness_check(False)
        t3 = w.submit_recursion(po2, bad_ctrl, wom, cyc, iops)
        res = _drain(w, 1)[t3]
        assert res[3] is not None and res[3].startswith("receipt verification failed: "), res[3]
