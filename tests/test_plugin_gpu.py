"""The demo circuit, the accumulation by callback and the self-test on the device, against the
demo AIR written down directly (tests/demo_air.py) and the host verifier:
  * r0hip_eval_check("demo") at po2 4 and 6, both tap forms, random and all-(p - 1) groups;
  * r0hip_demo_witness / r0hip_demo_accum against the numpy witness, one and several tiles;
  * r0hip_constraint_rows("demo") on the device witness, clean and with one word of `a` changed;
  * r0hip_prove_segment_cb("demo") in the three suites at po2 8 and 9: the seal passes the full
    check on host and device and equals the committed seal; a wrong mix, a failing callback, the
    memory accounting; and its parity with r0hip_prove_segment on a recursion witness;
  * r0hip_selftest at po2 10.
Sizes: po2 4 and 6 for the ops, 8 (the smallest the synthetic-seal tests prove) and 9 for seals."""
import json
import os

import numpy as np
import pytest

import demo_air as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "demo")
P = D.P
INVALID = 0xFFFFFFFF
KEY = np.array([0x64656D6F, 0x9E3779B9, 0x7F4A7C15, 0x0BADC0DE, 0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x00000001],
               dtype=np.uint32)
NONCE = np.array([0, 0, 0], np.uint32)
A0, B0 = 3, 5
SUITE_NAMES = ["poseidon2", "sha-256", "poseidon254"]


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def _active(po2):
    rows = 1 << po2
    return rows - max(1, rows // 8)


def _device_witness(hal, po2, n=None):
    """(code, data, global) Buffers: noise everywhere in data, then the device witness"""
    from risc0_amd import hal as H
    rows = 1 << po2
    n = _active(po2) if n is None else n
    code = hal.alloc_elem_init("code", 3 * rows, INVALID)
    data = hal.alloc_elem("data", 3 * rows)
    glob = hal.alloc_elem_init("global", 3, INVALID)
    H.fill_chacha20(data, KEY, NONCE)
    H.demo_witness(po2, n, int(D.enc(A0)), int(D.enc(B0)), code, data, glob)
    return code, data, glob


# ---- eval_check ----

def _eval_check_ref(po2, groups, mix, glob, x):
    """check[k * D + c] = (poly(c) / ((3 w^c)^N - 1))[k] on the 4N domain, taps 4 * back points up"""
    N, dom = 1 << po2, 4 << po2
    acc, code, data = groups
    vals = D.poly(D.taps_on_rows(code, data, acc, dom, step=4), glob, mix, x)
    w = _rou(po2 + 2)
    c = np.arange(dom)
    shift = pow(3, N, P)
    i4 = pow(w, N, P)
    vinv = np.array([pow((shift * pow(i4, k, P) - 1) % P, P - 2, P) for k in range(4)], np.uint64)
    return np.concatenate([np.asarray(v, np.uint64) * vinv[c % 4] % P for v in vals])


def _rou(lg):
    # baby_bear.rs:184-197 (risc0_amd/csrc/bb31.h kRouFwd): the root of unity of order 2^lg
    fwd = [1, 2013265920, 284861408, 1801542727, 567209306, 740045640, 918899846, 1881002012, 1453957774, 65325759,
           1538055801, 515192888, 483885487]
    assert pow(fwd[lg], 1 << lg, P) == 1 and pow(fwd[lg], 1 << (lg - 1), P) == P - 1
    return fwd[lg]


@pytest.mark.parametrize("wide", ["0", "0xffffffff"])
@pytest.mark.parametrize("po2", [4, 6])
def test_eval_check_equals_the_air(hal, po2, wide, monkeypatch):
    monkeypatch.setenv("R0_EC_WIDE", wide)
    dom = 4 << po2
    rng = np.random.default_rng(0xE0 + po2)
    for kind in ("random", "all p - 1"):
        draw = (lambda k: rng.integers(0, P, k).astype(np.uint64)) if kind == "random" else \
            (lambda k: np.full(k, P - 1, np.uint64))
        groups = [draw(4 * dom), draw(3 * dom), draw(3 * dom)]  # accum, code, data
        mix, glob, x = [int(v) for v in draw(4)], [int(v) for v in draw(3)], tuple(int(v) for v in draw(4))
        want = _eval_check_ref(po2, groups, mix, glob, x)
        assert want.any()
        out = hal.alloc_elem_init("check", 4 * dom, INVALID)
        hal.eval_check("demo", out, [hal.copy_from_elem("g", D.enc(g)) for g in groups],
                       hal.copy_from_elem("mix", D.enc(mix)), hal.copy_from_elem("glob", D.enc(glob)), D.enc(x), po2)
        assert np.array_equal(out.to_numpy(), D.enc(want)), kind


# ---- the witness and accumulation kernels ----

@pytest.mark.parametrize("po2,n", [(2, 1), (4, 13), (6, 64), (11, 1025), (12, 4001)])
def test_demo_witness_and_accum_equal_numpy(hal, po2, n):
    """one row, a partial wave, a full group, a tile and one row, four tiles less a few"""
    from risc0_amd import hal as H
    rows = 1 << po2
    code, data, glob = _device_witness(hal, po2, n)
    noise = hal.alloc_elem("noise", 3 * rows)
    H.fill_chacha20(noise, KEY, NONCE)
    wc, wd, wg = D.witness(po2, n, A0, B0)
    wd = D.enc(wd)
    for col in range(3):  # the rows above n keep the caller's noise
        wd[col * rows + n:(col + 1) * rows] = noise.to_numpy()[col * rows + n:(col + 1) * rows]
    assert np.array_equal(code.to_numpy(), D.enc(wc))
    assert np.array_equal(data.to_numpy(), wd)
    assert np.array_equal(glob.to_numpy(), D.enc(wg))
    mix = [P - 1, 1, 0, 123456789]
    acc = hal.alloc_elem_init("accum", 4 * rows, INVALID)
    H.demo_accum(po2, n, data, D.enc(mix), acc)
    want = D.enc(D.accumulate(po2, n, D.dec(wd), mix))
    for k in range(4):
        want[k * rows + n:(k + 1) * rows] = INVALID  # untouched
    assert np.array_equal(acc.to_numpy(), want)


def test_demo_kernels_refuse_bad_shapes(hal):
    from risc0_amd import hal as H
    b = hal.alloc_elem("b", 64)
    for po2, n in ((1, 1), (25, 1), (4, 0), (4, 17)):
        with pytest.raises(H.R0HipError, match="po2|n_active"):
            H.demo_witness(po2, n, 1, 1, b, b, b)
        with pytest.raises(H.R0HipError, match="po2|n_active"):
            H.demo_accum(po2, n, b, np.zeros(4, np.uint32), b)
    with pytest.raises(H.R0HipError, match="canonical"):
        H.demo_witness(4, 4, P, 1, b, b, b)


# ---- constraint_rows ----

@pytest.mark.parametrize("po2", [4, 6])
def test_constraint_rows_on_the_device_witness(hal, po2):
    from risc0_amd import hal as H
    rows, n = 1 << po2, _active(po2)
    code, data, glob = _device_witness(hal, po2)
    mix = [7, P - 1, 12345, 1]
    x = D.enc([7, 11, 13, 17])
    acc = hal.alloc_elem("accum", 4 * rows)
    H.fill_chacha20(acc, KEY, np.array([1, 0, 0], np.uint32))  # noise above n here too
    H.demo_accum(po2, n, data, D.enc(mix), acc)
    dmix = hal.copy_from_elem("mix", D.enc(mix))
    rep = H.constraint_rows("demo", po2, code, data, acc, dmix, glob, x)
    assert rep == {"bad_rows": 0, "first_row": None, "first_term": None, "rows": []}
    r = n // 2
    d = data.to_numpy()
    d[r] = D.enc((int(D.dec(d[r])) + 1) % P)  # a[r]
    data.copy_from(d)
    out = hal.alloc_extelem("vals", rows)
    rep = H.constraint_rows("demo", po2, code, data, acc, dmix, glob, x, out)
    taps = D.taps_on_rows(D.dec(code.to_numpy()), D.dec(d), D.dec(acc.to_numpy()), rows)
    row_taps = [int(t[r]) for t in taps]
    host_term = H.constraint_term("demo", D.enc(row_taps), D.enc(mix), glob.to_numpy(), x)
    assert rep == {"bad_rows": 2, "first_row": r, "first_term": host_term, "rows": [r, r + 1]}
    want = D.poly(taps, [int(v) for v in D.dec(glob.to_numpy())], mix, tuple(int(v) for v in D.dec(x)))
    assert np.array_equal(out.to_numpy().reshape(rows, 4), D.enc(np.stack([np.asarray(v) for v in want], axis=1)))


# ---- prove_segment_cb ----

def _prove_demo(hal, po2, accum_fn=None, witness=None):
    from risc0_amd import hal as H
    n = _active(po2)
    code, data, glob = witness or _device_witness(hal, po2)
    seen = {}

    def fill(mix, accum, stream):
        seen["mix"] = mix.copy()
        H.demo_accum(po2, n, data, mix, accum)

    seal, mix = H.prove_segment_cb(hal, "demo", po2, code, data, accum_fn or fill, glob)
    return seal, mix, seen


@pytest.mark.parametrize("po2", [8, 9])
@pytest.mark.parametrize("suite", [0, 1, 2])
def test_prove_segment_cb_demo_seal_is_valid_and_golden(suite, po2):
    import risc0_amd as r
    from risc0_amd import hal as H
    h = r.HipHal(SUITE_NAMES[suite])
    seal, mix, seen = _prove_demo(h, po2)
    assert np.array_equal(seen["mix"], mix) and mix.size == 4
    assert H.verify_seal("demo", suite, seal) == po2
    assert H.verify_seal("demo", suite, seal, where="device") == po2
    with open(os.path.join(GOLD, "index.json")) as f:
        gold = [e for e in json.load(f)["seals"] if (e["suite"], e["po2"]) == (suite, po2)]
    for e in gold:  # committed at the smaller size
        assert np.array_equal(seal, np.load(os.path.join(GOLD, e["file"]))), e
    assert gold or po2 != 8 or suite != 0


def test_prove_segment_cb_wrong_mix_proves_but_is_rejected(hal):
    from risc0_amd import hal as H
    po2, n = 8, _active(8)
    witness = _device_witness(hal, po2)

    def wrong(mix, accum, stream):
        other = mix.copy()
        other[1] = D.enc((int(D.dec(other[1])) + 1) % P)
        H.demo_accum(po2, n, witness[1], other, accum)

    seal, mix, _ = _prove_demo(hal, po2, wrong, witness)
    assert H.verify_seal("demo", 0, seal, check_validity=False) == po2
    with pytest.raises(H.R0HipError):
        H.verify_seal("demo", 0, seal)
    with pytest.raises(H.R0HipError):
        H.verify_seal("demo", 0, seal, where="device")
    # the witness check, when on, refuses it before the commit
    with hal.witness_check():
        with pytest.raises(H.R0HipError, match="constraint check failed"):
            _prove_demo(hal, po2, wrong, witness)
        seal2, _, _ = _prove_demo(hal, po2, None, witness)
    assert H.verify_seal("demo", 0, seal2) == po2


def test_prove_segment_cb_message_fails_the_call_and_memory_returns(hal):
    from risc0_amd import hal as H
    po2 = 8
    witness = _device_witness(hal, po2)
    _prove_demo(hal, po2, None, witness)  # pools warm
    live = H.mem_stats()["live"]
    with pytest.raises(H.R0HipError, match="accum callback: no accumulation today"):
        _prove_demo(hal, po2, lambda mix, accum, stream: "no accumulation today", witness)
    assert H.mem_stats()["live"] == live

    def raises(mix, accum, stream):
        raise ValueError("broken")

    with pytest.raises(H.R0HipError, match="accum callback: ValueError: broken"):
        _prove_demo(hal, po2, raises, witness)
    assert H.mem_stats()["live"] == live
    seal, _, _ = _prove_demo(hal, po2, None, witness)
    assert H.mem_stats()["live"] == live
    assert H.verify_seal("demo", 0, seal) == po2


def test_prove_segment_cb_under_proof_streams_and_deferred_mode(hal):
    from risc0_amd import hal as H
    po2 = 8
    witness = _device_witness(hal, po2)
    seal, _, _ = _prove_demo(hal, po2, None, witness)
    with hal.proof_streams(2):
        seal2, _, _ = _prove_demo(hal, po2, None, witness)
    with hal.deferred():
        seal3, _, _ = _prove_demo(hal, po2, None, witness)
    assert np.array_equal(seal, seal2) and np.array_equal(seal, seal3)


def test_prove_segment_cb_parity_with_prove_segment_recursion(hal):
    from risc0_amd import hal as H
    po2 = 8
    rows = 1 << po2
    info = H.circuit_info("recursion")
    rng = np.random.default_rng(0xCB)
    gs = info["group_sizes"]
    acc, code, data = (D.enc(rng.integers(0, P, g * rows)) for g in gs)
    glob = D.enc(rng.integers(0, P, info["output_size"]))
    dev = lambda a: hal.copy_from_elem("w", a)
    dacc = dev(acc)
    want, want_mix = H.prove_segment(hal, "recursion", po2, dev(code), dev(data), dacc, dev(glob))

    def copy_in(mix, accum, stream):
        assert accum.to_numpy().min() == INVALID  # the library's fill
        H.check(H.lib().r0hip_memcpy_d2d(accum.ptr, dacc.ptr, accum.nwords * 4))

    seal, mix = H.prove_segment_cb(hal, "recursion", po2, dev(code), dev(data), copy_in, dev(glob))
    assert np.array_equal(mix, want_mix) and np.array_equal(seal, want)


# ---- selftest ----

def test_selftest_passes_every_check(hal):
    from risc0_amd import hal as H
    H.trim()
    live = H.mem_stats()["live"]
    err, rep = H.selftest(0b111, 10)
    assert err is None, err
    assert sorted(rep) == [0, 1, 2]
    for s, e in rep.items():
        assert e["passed"] == 0b111 and e["seal_len"] > 0 and all(ms > 0 for ms in e["ms"]), (s, e)
        print(f"selftest suite {s}: seal {e['seal_len']} words, ms a/b/c = {e['ms']}")
    assert H.mem_stats()["live"] == live
    err, rep = H.selftest(0b010, 10)
    assert err is None and list(rep) == [1] and rep[1]["passed"] == 0b111
    with pytest.raises(H.R0HipError, match="suites_mask 0"):
        H.selftest(0, 10)
    with pytest.raises(H.R0HipError, match="out_size"):
        H.selftest(0b111, 10, out_size=4)
