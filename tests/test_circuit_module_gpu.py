"""Circuit modules on the device: a circuit's generated kernels loaded at run time
(r0hip_circuit_load) must give the words the same program compiled into the library gives. The
compiled circuits and the committed fixtures are the oracle; all arithmetic is exact BabyBear, so
every comparison is word for word.
  * eval_check: mod_demo and mod_recursion against the compiled circuits at po2 2 (domain 16, less
    than one wave), 4 (16 rows, fewer than the largest back: taps wrap) and 6, on random words and
    on p - 1 everywhere, into a buffer that starts as 0xFFFFFFFF; mod_recursion also against the
    committed fixtures;
  * one program registered (interpreted) and loaded (module) in one process: both agree with the
    compiled circuit in eval_check and constraint_rows;
  * constraint_rows: values and report against the compiled recursion circuit; the demo witness
    clean and with one word changed;
  * seals: prove_segment_cb under mod_demo equals the compiled circuit's in the three suites and
    the committed seal, verifies on host and device, one changed word is rejected;
  * mod_variant, the circuit no build has: proved, verified in full, rejected as "demo", and a
    plain demo witness reported as violating it;
  * the pipeline: r0hip_prove_segments equals r0hip_prove_segment; the witness check's message;
  * two modules of one generator in one process keep their own kernels;
  * no interpreter kernel runs under a loaded name.
Every negative case is a refusal on the host or a verdict; nothing here can fault the device."""
import json
import os

import numpy as np
import pytest

import circuit_module_util as M
import circuit_rt_util as U
import demo_air as D

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
GOLD = os.path.join(ROOT, "tests", "golden")
P = U.P
INVALID = 0xFFFFFFFF
KEY = np.array([0x64656D6F, 0x9E3779B9, 0x7F4A7C15, 0x0BADC0DE, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x00000001],
               dtype=np.uint32)
NONCE = np.array([0, 0, 0], np.uint32)
SUITE_NAMES = ["poseidon2", "sha-256", "poseidon254"]


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def _rand(rng, n):
    return rng.integers(0, P, n, dtype=np.uint64).astype(np.uint32)  # canonical Montgomery words


def _eval_check(hal, name, po2, groups, mix, glob, pm):
    dom = 4 << po2
    out = hal.alloc_elem_init("check", 4 * dom, INVALID)
    hal.eval_check(name, out, [hal.copy_from_elem("g", g) for g in groups], hal.copy_from_elem("mix", mix),
                   hal.copy_from_elem("glob", glob), pm, po2)
    return out.to_numpy()


def _inputs(name, n, kind, seed):
    """groups (accum, code, data) of n rows, mix, global, poly_mix: random canonical words, or
    the worst-case words of tests/ec_extreme.py's all_pm1 mode (p - 1 everywhere, as Montgomery words)"""
    from risc0_amd import hal as H
    info = H.circuit_info(name)
    sizes = [g * n for g in info["group_sizes"]] + [info["mix_size"], info["output_size"], 4]
    if kind == "random":
        rng = np.random.default_rng(seed)
        arrs = [_rand(rng, k) for k in sizes]
    else:
        import ec_extreme as X
        arrs = [X.enc(np.full(k, P - 1, np.uint64)) for k in sizes]
    return arrs[:3], arrs[3], arrs[4], arrs[5]


# the compiled circuits' eval_check words, computed once per input set and left unchanged
_WANT = {}


def _compiled_eval_check(hal, name, po2, kind):
    key = (name, po2, kind)
    if key not in _WANT:
        ins = _inputs(name, 4 << po2, kind, 0xEC00 + po2)
        _WANT[key] = (ins, _eval_check(hal, name, po2, *ins))
    return _WANT[key]


# ---- 1. eval_check parity ----

@pytest.mark.parametrize("kind", ["random", "all_pm1"])
@pytest.mark.parametrize("po2", [2, 4, 6])
@pytest.mark.parametrize("name", ["demo", "recursion"])
def test_eval_check_equals_the_compiled_circuit(hal, name, po2, kind):
    mod = M.loaded("mod_" + name)
    (groups, mix, glob, pm), want = _compiled_eval_check(hal, name, po2, kind)
    got = _eval_check(hal, mod, po2, groups, mix, glob, pm)
    assert want.max() < P and got.max() < P  # every word written (the buffer starts as 0xFFFFFFFF)
    assert np.array_equal(got, want)


with open(os.path.join(GOLD, "index.json")) as _f:
    _INDEX = json.load(_f)
_REC_FIXTURES = [c for c in _INDEX["eval_check"] if c["circuit"] == "recursion"]


@pytest.mark.parametrize("case", _REC_FIXTURES, ids=lambda c: f"{c['circuit']}-po2{c['po2']}")
def test_eval_check_equals_the_committed_fixture(hal, case):
    import oracle as O  # the seeded input generator only (tests/test_golden.py eval_inputs): nothing is built
    import test_golden as G
    assert sorted(c["po2"] for c in _REC_FIXTURES) == [4, 6]  # the two committed fixtures, both run here
    groups, mix, glob, pm = G.eval_inputs(O, case["circuit"], case["po2"], case["seed"])
    assert G.digest(*groups, mix, glob, pm) == case["inputs_sha256"]
    got = _eval_check(hal, M.loaded("mod_recursion"), case["po2"], groups, mix, glob, pm)
    assert np.array_equal(got, np.load(os.path.join(GOLD, case["file"])))


# ---- 2. one program interpreted and loaded in one process ----

def test_registered_and_loaded_agree_with_the_compiled_circuit(hal):
    from risc0_amd import hal as H
    rt, mod, po2 = U.registered("recursion"), M.loaded("mod_recursion"), 4
    assert [H.circuit_backend(n) for n in ("recursion", rt, mod)] == [0, 1, 2]
    (groups, mix, glob, pm), want = _compiled_eval_check(hal, "recursion", po2, "random")
    for name in (rt, mod):
        assert np.array_equal(_eval_check(hal, name, po2, groups, mix, glob, pm), want), name
    rows = 1 << po2
    groups, mix, glob, pm = _inputs("recursion", rows, "random", 0xC0 + po2)
    acc, code, data = (hal.copy_from_elem("g", g) for g in groups)
    dmix, dglob = hal.copy_from_elem("mix", mix), hal.copy_from_elem("glob", glob)
    res = []
    for circuit in ("recursion", rt, mod):
        out = hal.alloc_extelem("vals", rows)
        rep = H.constraint_rows(circuit, po2, code, data, acc, dmix, dglob, pm, out)
        res.append((rep, out.to_numpy()))
    for rep, vals in res[1:]:
        assert rep == res[0][0] and np.array_equal(vals, res[0][1])


# ---- 3. constraint_rows ----

@pytest.mark.parametrize("po2", [4, 6])
def test_constraint_rows_equal_the_compiled_circuit(hal, po2):
    from risc0_amd import hal as H
    mod, rows = M.loaded("mod_recursion"), 1 << po2
    groups, mix, glob, pm = _inputs("recursion", rows, "random", 0xC0 + po2)
    acc, code, data = (hal.copy_from_elem("g", g) for g in groups)
    dmix, dglob = hal.copy_from_elem("mix", mix), hal.copy_from_elem("glob", glob)
    res = []
    for circuit in ("recursion", mod):
        out = hal.alloc_extelem("vals", rows)
        rep = H.constraint_rows(circuit, po2, code, data, acc, dmix, dglob, pm, out)
        res.append((rep, out.to_numpy()))
    assert res[0][0]["bad_rows"] == rows  # random groups satisfy nothing
    assert res[1][0] == res[0][0]
    assert np.array_equal(res[1][1], res[0][1])


def _demo_witness(hal, po2, a0=3, b0=5):
    """(code, data, global) Buffers and n: noise everywhere in data, then the device witness"""
    from risc0_amd import hal as H
    rows = 1 << po2
    n = rows - max(1, rows // 8)
    code = hal.alloc_elem_init("code", 3 * rows, INVALID)
    data = hal.alloc_elem("data", 3 * rows)
    glob = hal.alloc_elem_init("global", 3, INVALID)
    H.fill_chacha20(data, KEY, NONCE)
    H.demo_witness(po2, n, int(D.enc(a0)), int(D.enc(b0)), code, data, glob)
    return code, data, glob, n


def test_constraint_rows_on_the_demo_witness_clean_and_with_one_word_changed(hal):
    from risc0_amd import hal as H
    mod, po2 = M.loaded("mod_demo"), 8
    rows = 1 << po2
    code, data, glob, n = _demo_witness(hal, po2)
    mix = [7, P - 1, 12345, 1]
    x = D.enc([7, 11, 13, 17])
    acc = hal.alloc_elem("accum", 4 * rows)
    H.fill_chacha20(acc, KEY, np.array([1, 0, 0], np.uint32))
    H.demo_accum(po2, n, data, D.enc(mix), acc)
    dmix = hal.copy_from_elem("mix", D.enc(mix))
    assert H.constraint_rows(mod, po2, code, data, acc, dmix, glob, x) == \
        {"bad_rows": 0, "first_row": None, "first_term": None, "rows": []}
    r = n // 2
    d = data.to_numpy()
    d[r] = D.enc((int(D.dec(d[r])) + 1) % P)  # a[r]: rows r and r + 1 tap it
    data.copy_from(d)
    want = H.constraint_rows("demo", po2, code, data, acc, dmix, glob, x)
    got = H.constraint_rows(mod, po2, code, data, acc, dmix, glob, x)
    assert got["bad_rows"] == 2 and got["rows"] == [r, r + 1] and got["first_row"] == r
    assert got["first_term"] == want["first_term"] and got["first_term"] is not None
    assert got == want


# ---- 4. seals ----

def _prove_cb(h, circuit, po2, witness):
    from risc0_amd import hal as H
    code, data, glob, n = witness
    return H.prove_segment_cb(h, circuit, po2, code, data, lambda mix, accum, stream: H.demo_accum(po2, n, data, mix, accum),
                              glob)


@pytest.mark.parametrize("suite", [0, 1, 2])
def test_seal_under_the_loaded_name_equals_the_compiled_circuits(suite):
    import risc0_amd as r
    from risc0_amd import hal as H
    mod, po2 = M.loaded("mod_demo"), 8
    h = r.HipHal(SUITE_NAMES[suite])
    witness = _demo_witness(h, po2)
    want, want_mix = _prove_cb(h, "demo", po2, witness)
    seal, mix = _prove_cb(h, mod, po2, witness)
    assert np.array_equal(mix, want_mix) and np.array_equal(seal, want)
    if suite == 0:
        with open(os.path.join(GOLD, "demo", "index.json")) as f:
            gold = [e for e in json.load(f)["seals"] if (e["suite"], e["po2"]) == (0, po2)]
        assert len(gold) == 1
        assert np.array_equal(seal, np.load(os.path.join(GOLD, "demo", gold[0]["file"])))
    assert H.verify_seal(mod, suite, seal) == po2
    assert H.verify_seal(mod, suite, seal, where="device") == po2
    bad = seal.copy()
    bad[bad.size // 2] ^= 1
    for where in ("host", "device"):
        with pytest.raises(H.R0HipError):
            H.verify_seal(mod, suite, bad, where=where)


def test_prove_segment_accum_refuses_a_loaded_circuit(hal):
    from risc0_amd import hal as H
    mod, po2 = M.loaded("mod_demo"), 8
    code, data, glob, n = _demo_witness(hal, po2)
    acc = hal.alloc_elem_init("accum", 4 << po2, INVALID)
    msgs = []
    for circuit in ("demo", U.registered("demo"), mod):
        with pytest.raises(H.R0HipError, match="no device accumulation for circuit " + circuit) as e:
            H.prove_segment_accum(hal, circuit, po2, code, data, acc, n, glob)
        msgs.append(str(e.value).replace(circuit, "demo"))
    assert msgs[0] == msgs[1] == msgs[2]


def test_the_version_word_stays_with_rv32im_under_a_loaded_name(hal):
    """the verifier expects a leading version word under the name rv32im only: a demo seal proved
    with one is the same seal under the compiled, registered and loaded names, and each name's
    verifier refuses it with the same words"""
    from risc0_amd import hal as H
    mod, rt, po2 = M.loaded("mod_demo"), U.registered("demo"), 8
    code, data, glob, n = _demo_witness(hal, po2)
    fill = lambda mix, accum, stream: H.demo_accum(po2, n, data, mix, accum)
    plain, _ = H.prove_segment_cb(hal, mod, po2, code, data, fill, glob)
    seals, msgs = [], []
    for circuit in ("demo", rt, mod):
        seal, _ = H.prove_segment_cb(hal, circuit, po2, code, data, fill, glob, version=2)
        seals.append(seal)
        with pytest.raises(H.R0HipError) as e:
            H.verify_seal(circuit, 0, seal)
        msgs.append(str(e.value).replace(circuit, "demo"))
    assert seals[0][0] == 2 and np.array_equal(seals[0][1:], plain)
    assert np.array_equal(seals[1], seals[0]) and np.array_equal(seals[2], seals[0])
    assert msgs[0] == msgs[1] == msgs[2]
    assert H.verify_seal(mod, 0, plain) == po2


# ---- 5. the circuit that is compiled in nowhere ----

def test_the_variant_module_is_proved_and_verified(hal):
    from risc0_amd import hal as H
    mod = M.loaded("mod_variant")
    assert mod in H.circuit_names()[3:] and H.circuit_backend(mod) == 2
    po2 = 8
    rows = 1 << po2
    n = rows - rows // 8
    code, data, glob = (np.array(v, dtype=np.uint64) for v in U.variant_witness(po2, n))
    assert (data[rows + 1], data[rows + 2]) == (13, 31)  # b = a[-1] + 2 b[-1] from (3, 5)
    dcode, ddata, dglob = (hal.copy_from_elem("w", D.enc(v)) for v in (code, data, glob))

    def fill(mix, accum, stream):
        acc = D.accumulate(po2, n, data, [int(v) for v in D.dec(mix)])
        accum.copy_from(D.enc(acc))

    seal, mix = H.prove_segment_cb(hal, mod, po2, dcode, ddata, fill, dglob)
    assert H.verify_seal(mod, 0, seal) == po2  # the validity equation included
    assert H.verify_seal(mod, 0, seal, where="device") == po2
    for other in ("demo", M.loaded("mod_demo")):
        with pytest.raises(H.R0HipError):
            H.verify_seal(other, 0, seal)
    # the rows check: the variant's witness is clean, a witness of the plain demo is not
    x = D.enc([7, 11, 13, 17])
    dmix = hal.copy_from_elem("mix", mix)
    acc = hal.copy_from_elem("accum", D.enc(D.accumulate(po2, n, data, [int(v) for v in D.dec(mix)])))
    assert H.constraint_rows(mod, po2, dcode, ddata, acc, dmix, dglob, x)["bad_rows"] == 0
    pc, pd, pg = D.witness(po2, n, 3, 5)
    pacc = hal.copy_from_elem("accum", D.enc(D.accumulate(po2, n, pd, [int(v) for v in D.dec(mix)])))
    plain = [hal.copy_from_elem("w", D.enc(v)) for v in (pc, pd, pg)]
    assert H.constraint_rows("demo", po2, plain[0], plain[1], pacc, dmix, plain[2], x)["bad_rows"] == 0
    rep = H.constraint_rows(mod, po2, plain[0], plain[1], pacc, dmix, plain[2], x)
    assert rep["bad_rows"] > 0 and rep["first_row"] == 1


# ---- 6. the pipeline and the witness check ----

def test_prove_segments_equals_prove_segment(hal):
    from risc0_amd import hal as H
    mod, po2 = M.loaded("mod_demo"), 8
    rows = 1 << po2
    jobs, want = [], []
    for a0, b0 in ((3, 5), (4, 7)):
        code, data, glob, n = _demo_witness(hal, po2, a0, b0)
        cb_seal, mix = _prove_cb(hal, mod, po2, (code, data, glob, n))  # draws the mix this witness gets
        acc = hal.alloc_elem_init("accum", 4 * rows, INVALID)
        H.demo_accum(po2, n, data, mix, acc)
        hal.eltwise_zeroize_elem(acc)
        seal, mix2 = H.prove_segment(hal, mod, po2, code, data, acc, glob)
        assert np.array_equal(mix2, mix) and np.array_equal(seal, cb_seal)
        want.append(seal)
        jobs.append((code.to_numpy(), data.to_numpy(), acc.to_numpy(), glob.to_numpy()))
    got = H.prove_segments(hal, mod, po2, jobs, in_flight=2)
    assert len(got) == 2
    for (seal, _), w in zip(got, want):
        assert np.array_equal(seal, w)
    assert not np.array_equal(want[0], want[1])


def test_witness_check_message_is_the_compiled_circuits(hal):
    from risc0_amd import hal as H
    mod, po2 = M.loaded("mod_demo"), 8
    code, data, glob, n = _demo_witness(hal, po2)
    d = data.to_numpy()
    r = n // 2
    d[r] = D.enc((int(D.dec(d[r])) + 1) % P)
    data.copy_from(d)
    msgs = []
    with hal.witness_check():
        for circuit in ("demo", mod):
            with pytest.raises(H.R0HipError, match="constraint check failed: 2 of 256 rows, first at cycle " + str(r)) as e:
                _prove_cb(hal, circuit, po2, (code, data, glob, n))
            msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    # off again, the same witness proves (and the seal fails the validity equation)
    seal, _ = _prove_cb(hal, mod, po2, (code, data, glob, n))
    with pytest.raises(H.R0HipError):
        H.verify_seal(mod, 0, seal)


# ---- 7. two modules of one generator in one process ----

def test_two_modules_keep_their_own_kernels(hal):
    """mod_demo and mod_variant come from one generator: their kernels and launchers carry the
    same internal names (k0, launch_k0, ...) in two shared objects. Run alternately, each must
    keep giving its own circuit's words; the programs differ, so equal outputs would mean one
    module's kernels ran for both."""
    a, b, po2 = M.loaded("mod_demo"), M.loaded("mod_variant"), 6
    (groups, mix, glob, pm), want_a = _compiled_eval_check(hal, "demo", po2, "random")
    outs = {a: [], b: []}
    for _ in range(3):
        for name in (a, b):
            outs[name].append(_eval_check(hal, name, po2, groups, mix, glob, pm))
    for name in (a, b):
        assert outs[name][0].max() < P
        assert all(np.array_equal(o, outs[name][0]) for o in outs[name][1:]), name
    assert np.array_equal(outs[a][0], want_a)
    assert not np.array_equal(outs[a][0], outs[b][0])


def test_the_variant_module_equals_the_interpreted_variant(hal, tmp_path):
    """mod_variant has no compiled-in twin; its oracle is the same program interpreted"""
    from risc0_amd import hal as H
    if U.VARIANT not in H.circuit_names():
        U.write_variant(str(tmp_path))
        H.register_circuit(U.VARIANT, str(tmp_path))
    mod = M.loaded("mod_variant")
    for po2 in (2, 6):
        groups, mix, glob, pm = _inputs("demo", 4 << po2, "random", 0xEC40 + po2)
        assert np.array_equal(_eval_check(hal, mod, po2, groups, mix, glob, pm),
                              _eval_check(hal, U.VARIANT, po2, groups, mix, glob, pm))


# ---- 8. no interpreter kernel under a loaded name ----

def test_kernel_times_list_no_interpreter_kernel(hal):
    import risc0_amd as r
    mod, po2 = M.loaded("mod_recursion"), 4
    (groups, mix, glob, pm), want = _compiled_eval_check(hal, "recursion", po2, "random")
    r.set_kernel_timing(True)
    try:
        r.kernel_times()  # start from an empty list
        got = _eval_check(hal, mod, po2, groups, mix, glob, pm)
        times = r.kernel_times()
    finally:
        r.set_kernel_timing(False)
    assert np.array_equal(got, want)
    assert "eval_check" in times and times["eval_check"][1] == 1
    assert not [k for k in times if "interp" in k], times.keys()
