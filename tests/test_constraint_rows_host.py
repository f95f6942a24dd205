"""The host half of the constraint-rows check, no GPU:
  * r0hip_constraint_term against the Python restatement of its walk (constraint_rows_ref.first_term)
    on rows of satisfying witnesses of both circuits with one tap changed, the reference's own
    compiled poly_fp (oracle.poly_fp_at_taps) confirming first that each changed row violates the
    constraints and the unchanged one does not;
  * the generated rows kernels' arithmetic as a host translation unit (gen_eval_check.py
    --host-rows) against the numpy IR interpreter at stride 1, on the extreme inputs of
    ec_extreme.py;
  * the arguments r0hip_constraint_rows, r0hip_constraint_term and
    r0hip_worker_set_witness_check refuse, each named in the message;
  * the thread mode's default and its return value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_rows_ref as CR
import ir_eval
import recursion_program as RP
import rv32im_witgen_ref as W
from ec_extreme import MODES, enc, extreme_inputs
from test_golden import e_mul, e_pow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = CR.P
u32p = C.POINTER(C.c_uint32)
POLY_MIX = np.array([CR.enc(x) for x in (7, 11, 13, 17)], np.uint32)


@pytest.fixture(scope="module")
def witnesses(oracle):
    """a satisfying witness per circuit (the reference's compiled witness generators and
    accumulations): recursion at po2 11, rv32im's smallest built trace at po2 13"""
    if not (RP.available() and W.RA.available()):
        pytest.skip("oracle/_ref not built")
    return {"recursion": (11, CR.recursion_witness(3100, 11, 3101)),
            "rv32im": (13, CR.rv32im_witness_host(13, 200, 0x5249534330, 3102))}


def _candidates(name, po2, w):
    """(row, tap) pairs in a fixed order: rows of the program's body, its first row, the last
    row (whose taps wrap) and a ZK / padding row, every 7th tap of each"""
    n = 1 << po2
    n_taps = len(CR.circuit(name)["taps"])
    rows = [5, 40, 0, 97, n - 1, n - 600, 150, 33]
    return [(r, t) for k, r in enumerate(rows) for t in range(k % 7, n_taps, 7)]


@pytest.mark.parametrize("name", ["recursion", "rv32im"])
def test_constraint_term_matches_the_restated_walk(oracle, witnesses, name):
    import risc0_amd as r
    po2, w = witnesses[name]
    fp = CR.PolyFp(oracle, name)
    mix, glob = w["mix"], w["glob"]
    byid = {ins[1]: ins for ins in CR.program(name) if ins[0] != "r"}
    top, v = [], [ins for ins in CR.program(name) if ins[0] == "r"][0][1]
    while byid[v][0] in "ab":  # the top-level chain's records
        top.append(byid[v][0])
        v = byid[v][2]
    hit = []  # (row, tap, term, depth)
    clean_rows = set()
    for row, tap in _candidates(name, po2, w):
        taps = CR.gather_taps(name, w["groups"], po2, [row])[0]
        if row not in clean_rows:
            # the unchanged row satisfies the constraints: the oracle, the library, the restatement
            assert not fp.value(taps, mix, glob, POLY_MIX).any(), f"row {row} of the witness is violated"
            assert r.constraint_term(name, taps, mix, glob, POLY_MIX) is None
            assert CR.first_term(name, taps, mix, glob, POLY_MIX) is None
            clean_rows.add(row)
        changed = taps.copy()
        changed[tap] = (int(changed[tap]) + CR.enc(1)) % P
        if not fp.value(changed, mix, glob, POLY_MIX).any():
            continue  # no constraint of this row reads the tap
        want, depth = CR.first_term(name, changed, mix, glob, POLY_MIX, with_depth=True)
        assert want is not None, f"row {row} tap {tap}: the oracle is nonzero, the restatement finds no term"
        got = r.constraint_term(name, changed, mix, glob, POLY_MIX)
        assert got == want, f"row {row} tap {tap}: term {got}, the restated walk gives {want}"
        hit.append((row, tap, want, depth))
        depths = {h[3] for h in hit}
        if len({h[1] for h in hit}) >= 30 and max(depths) >= 1 and ("a" in top) == (0 in depths):
            break  # enough taps, both kinds of answer among them
    assert len({h[1] for h in hit}) >= 20, f"only {len(hit)} changed taps violate a constraint"
    # both kinds of answer are hit: an `a` of the top-level chain (where the circuit has one: the
    # recursion circuit's top-level chain is guarded blocks only) and terms inside `b` blocks
    assert all(byid[h[2]][0] in "ab" for h in hit)
    depths = {h[3] for h in hit}
    assert max(depths) >= 1, f"no term nested in a `b` block was hit: {depths}"
    assert ("a" in top) == (0 in depths), f"top-level chain {set(top)}, depths hit {depths}"
    assert len({h[2] for h in hit}) >= 5, "the changed taps should violate several different terms"


# ---- the generated arithmetic on the CPU ------------------------------------------------------
@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    libs = {}
    d = tmp_path_factory.mktemp("rows_host")
    for circuit in ("rv32im", "recursion"):
        src, so = d / f"rows_{circuit}.cpp", d / f"rows_{circuit}.so"
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_eval_check.py"), "--host-rows", circuit,
                               str(src)], stdout=subprocess.DEVNULL)
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "risc0_amd", "csrc"), str(src), "-o", str(so)])
        libs[circuit] = C.CDLL(str(so))
    return libs


@pytest.mark.parametrize("circuit", ["rv32im", "recursion"])
@pytest.mark.parametrize("mode", MODES)
def test_generated_rows_kernels_extreme_inputs(host_rows, oracle, circuit, mode):
    """every word p - 1, or a mix of 0, 1, 2, p - 2, p - 1, on 16 rows: the kernels' bodies, run
    per row on the host, give poly_fp at stride 1 (taps at row - back, wrapping: every back of
    the circuits exceeds 16 rows somewhere) word for word"""
    d = oracle.load_circuit_json(circuit)
    n = 16
    plain, poly_mix = extreme_inputs(d, mode, 2)  # buffers of 4 << 2 = 16 rows
    args_plain = [plain[a] for a in d["eval_args"]]
    lib = host_rows[circuit]
    combos, npm = C.POINTER(C.c_int)(), C.c_int()
    ncomb = getattr(lib, f"rows_host_{circuit}_combos")(C.byref(combos), C.byref(npm))
    pows = [e_pow(poly_mix, k) for k in d["poly_mix_powers"]]
    table = pows[:npm.value]
    k = 0
    for _ in range(ncomb):
        cnt, prod = combos[k], (1, 0, 0, 0)
        for q in range(cnt):
            prod = e_mul(prod, table[combos[k + 1 + q]])
        k += 1 + cnt
        table.append(prod)
    pm = enc([x for t in table for x in t])
    pmn = enc([x * (P - 11) for t in table for x in t])
    acc, check, vinv = np.zeros(4 * n, np.uint32), np.zeros(4 * n, np.uint32), np.zeros(4, np.uint32)
    mf, me = np.zeros(64 * n, np.uint32), np.zeros(64 * 4 * n, np.uint32)
    arrs = [enc(a) for a in args_plain]
    argv = (u32p * len(arrs))(*[a.ctypes.data_as(u32p) for a in arrs])
    p = lambda a: a.ctypes.data_as(u32p)
    getattr(lib, f"rows_host_{circuit}")(argv, p(pm), p(pmn), p(vinv), p(acc), p(mf), p(me), p(check), C.c_uint32(n))
    ref = np.stack(ir_eval.evaluate(ir_eval.load_ir(circuit), args_plain, n, pows, inv_rate=1))
    assert np.array_equal(acc.reshape(n, 4), enc(ref.T.reshape(-1)).reshape(n, 4))
    assert ref.any(), "the extreme inputs satisfy nothing: the expected values are not all zero"


# ---- refusals ----------------------------------------------------------------------------------
def _message(err):
    import risc0_amd as r
    assert err, "the call was not refused"
    msg = C.cast(err, C.c_char_p).value.decode()
    r.lib().r0hip_free_error(err)
    return msg


def test_constraint_rows_refuses_on_the_host_naming_the_argument():
    """no device call is made before the refusal: this runs without a GPU"""
    import risc0_amd as r
    L = r.lib()
    rep = r.ConstraintReport()
    pm = POLY_MIX.ctypes.data_as(u32p)
    good = dict(circuit=b"recursion", po2=11, d_code=0x1000, d_data=0x2000, d_accum=0x3000, d_mix=0x4000,
                d_global=0x5000, report=C.addressof(rep))

    def call(**kw):
        a = dict(good, **kw)
        return _message(L.r0hip_constraint_rows(a["circuit"], a["po2"], a["d_code"], a["d_data"], a["d_accum"],
                                                a["d_mix"], a["d_global"], pm, None, a["report"]))
    for arg in ("d_code", "d_data", "d_accum", "d_mix", "d_global", "report"):
        msg = call(**{arg: None})
        assert msg.startswith("r0hip: r0hip_constraint_rows: ") and f"{arg} is NULL" in msg, msg
    assert "unknown circuit fibonacci" in call(circuit=b"fibonacci")
    assert "unknown circuit (null)" in call(circuit=None)
    for po2 in (0, 1, 25, 2**31):
        msg = call(po2=po2)
        assert f"po2 {po2} out of range" in msg, msg


def test_constraint_term_refuses_naming_the_argument():
    import risc0_amd as r
    L = r.lib()
    d = CR.circuit("rv32im")
    taps = np.zeros(len(d["taps"]), np.uint32)
    mix, glob = np.zeros(d["mix_size"], np.uint32), np.zeros(d["output_size"], np.uint32)
    term = C.c_int32(0)
    good = dict(circuit=b"rv32im", h_taps=taps.ctypes.data_as(u32p), h_mix=mix.ctypes.data_as(u32p),
                h_global=glob.ctypes.data_as(u32p), h_poly_mix=POLY_MIX.ctypes.data_as(u32p), term=C.pointer(term))

    def call(**kw):
        a = dict(good, **kw)
        return L.r0hip_constraint_term(a["circuit"], a["h_taps"], a["h_mix"], a["h_global"], a["h_poly_mix"], a["term"])
    for arg in ("h_taps", "h_mix", "h_global", "h_poly_mix", "term"):
        msg = _message(call(**{arg: None}))
        assert msg.startswith("r0hip: r0hip_constraint_term: ") and f"{arg} is NULL" in msg, msg
    assert "unknown circuit sha" in _message(call(circuit=b"sha"))
    assert not call()  # all-zero taps of rv32im: accepted, and whatever the term, no error
    assert "w is NULL" in _message(L.r0hip_worker_set_witness_check(None, 1))


def test_witness_check_mode_is_per_thread_and_off_by_default():
    import threading
    import risc0_amd as r
    assert r.set_witness_check(True) is False
    seen = []
    t = threading.Thread(target=lambda: seen.append(r.set_witness_check(False)))
    t.start()
    t.join()
    assert seen == [False], "a new thread starts with the mode off"
    assert r.set_witness_check(False) is True, "another thread's call left this thread's mode alone"
    assert r.set_witness_check(False) is False
