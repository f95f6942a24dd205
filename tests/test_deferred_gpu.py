"""Deferred completion mode of the per-op C ABI (r0hip_set_deferred, r0hip_call_stats).

In the mode, the device-only entry points return with their work queued on the calling thread's
stream; the entry points that hand data or a verdict to the host drain first. Everything here
compares a deferred run with the same calls in the default (synchronous) mode, bit for bit, and
reads r0hip_call_stats to tell that the calls really were left queued. The ordering rules the
runtime keeps (pool reuse in stream order, the copy stream behind queued kernels, the pool
hand-back only at a drain) each have a test that fails when the rule is dropped.

Not reachable here, checked by reading runtime.cpp (stage_take): the staging arena's overflow
path (a proof stages a few hundred 256-byte slots between drains, against 64 MiB).
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import rv32im_trace as T

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration"))

P = 15 * 2**27 + 1
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def r():
    import risc0_amd
    return risc0_amd


@pytest.fixture(scope="module")
def hal(r):
    return r.HipHal("poseidon2")


@pytest.fixture(autouse=True)
def default_mode_after(r):
    """no test leaves its thread in deferred mode"""
    yield
    r.check(r.lib().r0hip_set_deferred(0, None))


def alloc(r, words):
    p = C.c_void_p()
    r.check(r.lib().r0hip_alloc(C.byref(p), max(1, words) * 4))
    return p.value


def free(r, *ptrs):
    for p in ptrs:
        r.check(r.lib().r0hip_free(p))


def read(r, ptr, words):
    out = np.empty(words, np.uint32)
    r.check(r.lib().r0hip_memcpy_d2h(out.ctypes.data, ptr, words * 4))
    return out


def delta(r, before):
    now = r.call_stats()
    return {k: now[k] - before[k] for k in now}


# ---- the chain of tests 1, 5 and 7: one Merkle commitment, per op ---------------------------------
CHAIN_COLS, CHAIN_LG = 8, 12
CHAIN_ROWS = 1 << (CHAIN_LG + 2)
# 3 alloc, 8 memset32, interpolate, expand + evaluate, hash_rows, one hash_fold per layer, 2 free
CHAIN_CALLS = 3 + CHAIN_COLS + 3 + (CHAIN_LG + 2) + 2


def chain(r, suite=0):
    """alloc, memset32 (one value per column), batch_interpolate_ntt, batch_expand_into_evaluate_ntt,
    hash_rows, hash_fold per layer, free: CHAIN_CALLS device-only calls and no read. Returns the
    node heap, whose root the caller reads (and which the caller frees)."""
    L = r.lib()
    n = 1 << CHAIN_LG
    coeffs, evaluated, nodes = alloc(r, CHAIN_COLS * n), alloc(r, CHAIN_COLS * CHAIN_ROWS), alloc(r, 2 * CHAIN_ROWS * 8)
    for c in range(CHAIN_COLS):
        r.check(L.r0hip_memset32(coeffs + c * n * 4, 1000003 * (c + 1), n))
    r.check(L.r0hip_batch_interpolate_ntt(coeffs, CHAIN_COLS, CHAIN_LG))
    r.check(L.r0hip_batch_expand_into_evaluate_ntt(evaluated, coeffs, CHAIN_COLS, CHAIN_LG + 2, 2))
    r.check(L.r0hip_hash_rows(suite, nodes + CHAIN_ROWS * 32, evaluated, CHAIN_ROWS, CHAIN_COLS))
    for i in reversed(range(CHAIN_LG + 2)):
        r.check(L.r0hip_hash_fold(suite, nodes, (1 << i) * 2, 1 << i))
    free(r, coeffs, evaluated)
    return nodes


def chain_root(r):
    nodes = chain(r)
    root = read(r, nodes + 32, 8)
    free(r, nodes)
    return root


@pytest.fixture(scope="module")
def sync_root(r, hal):
    return chain_root(r)


def test_calls_really_defer(r, hal, sync_root):
    """the chain leaves every one of its calls queued in deferred mode and drains every one in the
    default mode; the root read afterwards is the same"""
    s0 = r.call_stats()
    nodes = chain(r)
    assert delta(r, s0) == {"calls": CHAIN_CALLS, "drained": CHAIN_CALLS, "queued": 0}
    free(r, nodes)
    with hal.deferred():
        s0 = r.call_stats()
        nodes = chain(r)
        assert delta(r, s0) == {"calls": CHAIN_CALLS, "drained": 0, "queued": CHAIN_CALLS}
        root = read(r, nodes + 32, 8)  # a read drains
        assert delta(r, s0) == {"calls": CHAIN_CALLS + 1, "drained": 1, "queued": CHAIN_CALLS}
        free(r, nodes)
    assert np.array_equal(root, sync_root)
    assert len(set(sync_root.tolist())) > 1


def test_constructor_and_set_deferred_report_the_mode(r):
    h = r.HipHal("poseidon2", deferred=True)
    assert h.set_deferred(True) is True
    assert h.set_deferred(False) is True
    assert h.set_deferred(False) is False
    with h.deferred():
        assert h.set_deferred(True) is True
    assert h.set_deferred(False) is False


# ---- op parity ------------------------------------------------------------------------------------
MIX_ROWS = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 13}  # as test_gpu_op_edges.py


def op_inputs(oracle):
    """host inputs of run_ops, drawn once"""
    import accum_ir as A
    import bigint_records as G
    import rv32im_accum_ref as R
    from test_rv32im_accum_ir import rows_for_arms
    rng = np.random.default_rng(0xDEFE44ED)
    d = A.circuit()
    rec_po2 = 4
    ctrl, rglob, rdata, rmix = A.synthetic(rng, oracle, rec_po2, d["group_sizes"], d["output_size"], d["mix_size"])
    rows = 1 << 10
    draw = lambda n: rng.integers(0, P, n, dtype=np.uint64).astype(np.uint32)
    cycles = 300
    offsets = rng.permutation(3 << 13)[:cycles].astype(np.uint32)
    return dict(
        which=np.array([0, 2, 1, 1, 0, 2, 2, 0, 1], np.uint32), xs=oracle.rand_elems(rng, 4 * 9),
        combos=rng.permutation(np.repeat(list(MIX_ROWS), list(MIX_ROWS.values()))).astype(np.uint32),
        mix_start=oracle.rand_elems(rng, 4), mix=oracle.rand_elems(rng, 4),
        reg_sizes=np.array([1, 2, 3, 2, 1, 6, 1], np.uint32), reg_ids=np.array([0, 1, 2, 3, 0, 2, 1], np.uint32),
        coeff_u=oracle.rand_elems(rng, 4 * (16 + 16)),
        index=np.arange(cycles + 1, dtype=np.uint32), offsets=offsets, values=oracle.rand_elems(rng, cycles),
        key=draw(8) | np.uint32(1 << 31), nonce=np.array([1, 2, 3], np.uint32),
        rv_rows=rows, rv_data=rows_for_arms(rng, rows, list(rng.integers(0, 13, rows))), rv_glob=draw(R.GLOBAL_WORDS),
        rv_mix=draw(R.MIX_WORDS), rv_cols=R.ACCUM_COLS,
        recs_small=G.valid_stream(rng, 100, 1 << 13), recs_large=G.valid_stream(rng, 5000, 1 << 13),
        rec_n=1 << rec_po2, rec_accum_cols=d["group_sizes"][0], ctrl=ctrl, rglob=rglob, rdata=rdata, rmix=rmix)


def run_ops(r, hal, inp, deferred):
    """Every device-only entry point, inputs and outputs chained where the op allows it, with no
    read between the first and the last op. Returns the final buffers as host arrays, and the
    call counters' change over the ops."""
    L = r.lib()
    u32p = C.POINTER(C.c_uint32)
    hp = lambda a: np.ascontiguousarray(a, np.uint32).ctypes.data_as(u32p)
    up = lambda a: hal.copy_from_elem("in", a)  # synchronous uploads, all before the ops
    d_which, d_xs = up(inp["which"]), up(inp["xs"])
    d_index, d_offsets, d_values = up(inp["index"]), up(inp["offsets"]), up(inp["values"])
    d_rvdata, d_rvglob, d_rvmix = up(inp["rv_data"]), up(inp["rv_glob"]), up(inp["rv_mix"])
    d_ctrl, d_rglob, d_rdata, d_rmix = up(inp["ctrl"]), up(inp["rglob"]), up(inp["rdata"]), up(inp["rmix"])
    keep = [np.ascontiguousarray(inp[k], np.uint32) for k in ("combos", "mix_start", "mix", "reg_sizes", "reg_ids",
                                                                "coeff_u", "key", "nonce")]
    combos, mix_start, mix, reg_sizes, reg_ids, coeff_u, key, nonce = keep
    backs = {k: r.bigint_backs(inp[k]) for k in ("recs_small", "recs_large")}
    n13, count = 1 << 13, 257
    chunks = max(MIX_ROWS) + 1
    out = {}
    was = hal.set_deferred(deferred)
    s0 = r.call_stats()
    ck = r.check
    try:
        # NTT family: lg 13 is one row pass, lg 14 and 15 add a column pass (ntt.hip plan())
        x = alloc(r, 3 * n13)
        ck(L.r0hip_fill_uniform(x, 3 * n13, 11))
        ck(L.r0hip_batch_interpolate_ntt(x, 3, 13))
        ck(L.r0hip_zk_shift(x, 3, 13))
        e15, e13 = alloc(r, 3 << 15), alloc(r, 12 << 13)
        ck(L.r0hip_batch_expand_into_evaluate_ntt(e15, x, 3, 15, 2))
        ck(L.r0hip_batch_expand_into_evaluate_ntt(e13, x, 12, 13, 2))
        ck(L.r0hip_batch_bit_reverse(x, 3, 13))
        y = alloc(r, 1 << 14)
        ck(L.r0hip_memcpy_d2d(y, e15 + 4 * 12345, 4 << 14))
        ck(L.r0hip_batch_interpolate_ntt(y, 1, 14))
        # hashing: 17 columns (one past the 16-column sponge rate), per layer and fused
        rows = 4096
        nodes, nodes2 = alloc(r, 2 * rows * 8), alloc(r, 2 * rows * 8)
        ck(L.r0hip_memset32(nodes, 0, 8))  # node 0 is written by neither form
        ck(L.r0hip_memset32(nodes2, 0, 8))
        ck(L.r0hip_hash_rows(0, nodes + rows * 32, e13, rows, 17))
        for i in reversed(range(12)):
            ck(L.r0hip_hash_fold(0, nodes, (1 << i) * 2, 1 << i))
        ck(L.r0hip_merkle_tree(0, nodes2, e13, rows, 17))
        # element-wise
        s, c, z = alloc(r, 3 * n13), alloc(r, 3 * n13), alloc(r, 3 * n13)
        ck(L.r0hip_eltwise_add_elem(s, x, e13, 3 * n13))
        ck(L.r0hip_eltwise_copy_elem(c, s, 3 * n13))
        ck(L.r0hip_memset32(z, INVALID, 3 * n13))
        ck(L.r0hip_eltwise_copy_elem_slice(z, s, 3, 100, 5, n13, 7, n13))
        ck(L.r0hip_scatter(z, d_index.ptr, d_offsets.ptr, d_values.ptr, inp["index"].size - 1))
        ck(L.r0hip_eltwise_zeroize_elem(z, 3 * n13))
        summed, folded, sample = alloc(r, 4 * count), alloc(r, 4 * count), alloc(r, 17)
        ck(L.r0hip_eltwise_sum_extelem(summed, s, 3, count))
        ck(L.r0hip_fri_fold(folded, c, hp(mix), count))
        ck(L.r0hip_gather_sample(sample, e13, 5, 17, rows))
        ck(L.r0hip_prefix_products(c, 300))
        # polynomial ops: evaluation at lg 13 (two waves of a chunk empty) and lg 2 (ragged piece)
        ev13, ev2 = alloc(r, 4 * 9), alloc(r, 4 * 9)
        ck(L.r0hip_batch_evaluate_any(ev13, x, 3, 13, d_which.ptr, d_xs.ptr, 9))
        ck(L.r0hip_batch_evaluate_any(ev2, s, 3, 2, d_which.ptr, d_xs.ptr, 9))
        mixed = alloc(r, 4 * count * chunks)
        ck(L.r0hip_fill_uniform(mixed, 4 * count * chunks, 12))
        ck(L.r0hip_mix_poly_coeffs(mixed, e15, hp(combos), hp(mix_start), hp(mix), combos.size, count))
        ck(L.r0hip_combos_prepare(mixed, hp(coeff_u), 4, 8, hp(reg_sizes), hp(reg_ids), reg_sizes.size, hp(mix)))
        cha = alloc(r, 1000)
        ck(L.r0hip_fill_chacha20(cha, 1000, hp(key), hp(nonce)))
        # accumulation
        rv_rows, rv_cols = inp["rv_rows"], inp["rv_cols"]
        fin, acc = alloc(r, rv_cols * rv_rows), alloc(r, rv_cols * rv_rows)
        ck(L.r0hip_fill_uniform(fin, rv_cols * rv_rows, 13))
        ck(L.r0hip_rv32im_accum_finalize(fin, rv_rows, rv_cols, 1000))
        ck(L.r0hip_memset32(acc, INVALID, rv_cols * rv_rows))
        ck(L.r0hip_rv32im_accum(d_rvdata.ptr, acc, d_rvglob.ptr, d_rvmix.ptr, rv_rows, rv_cols, rv_rows))
        big = alloc(r, 2 * 12 << 13)
        ck(L.r0hip_memset32(big, INVALID, 2 * 12 << 13))
        for k, name in enumerate(("recs_small", "recs_large")):  # the host loop, the device scans
            ck(L.r0hip_rv32im_bigint_accum_inject(big + k * (12 << 13) * 4, 1 << 13, hp(inp["rv_mix"]),
                                                   C.cast(backs[name], C.c_void_p), len(backs[name])))
        rec_n = inp["rec_n"]
        racc = alloc(r, inp["rec_accum_cols"] * rec_n)
        ck(L.r0hip_memset32(racc, INVALID, inp["rec_accum_cols"] * rec_n))
        ck(L.r0hip_recursion_accum(d_ctrl.ptr, d_rglob.ptr, d_rdata.ptr, d_rmix.ptr, racc, rec_n - 3, rec_n))
        # a freed block is taken again while the ops above may still be queued on it
        free(r, e15, y)
        y2 = alloc(r, 1 << 14)
        ck(L.r0hip_memset32(y2, 7, 1 << 14))
        stats = delta(r, s0)
    finally:
        hal.set_deferred(was)
    sizes = dict(x=3 * n13, e13=12 << 13, nodes=2 * rows * 8, nodes2=2 * rows * 8, s=3 * n13, c=3 * n13, z=3 * n13,
                 summed=4 * count, folded=4 * count, sample=17, ev13=36, ev2=36, mixed=4 * count * chunks, cha=1000,
                 fin=rv_cols * rv_rows, acc=rv_cols * rv_rows, big=2 * 12 << 13, racc=inp["rec_accum_cols"] * rec_n,
                 y2=1 << 14)
    ptrs = dict(x=x, e13=e13, nodes=nodes, nodes2=nodes2, s=s, c=c, z=z, summed=summed, folded=folded, sample=sample,
                ev13=ev13, ev2=ev2, mixed=mixed, cha=cha, fin=fin, acc=acc, big=big, racc=racc, y2=y2)
    for k, p in ptrs.items():
        out[k] = read(r, p, sizes[k])
    free(r, *ptrs.values())
    return out, stats


def test_op_parity(r, hal, oracle):
    """more than 20 ops back to back, every device-only entry point among them, none drained in
    deferred mode: the final buffers equal the synchronous run's bit for bit"""
    inp = op_inputs(oracle)
    want, sync_stats = run_ops(r, hal, inp, False)
    got, stats = run_ops(r, hal, inp, True)
    assert sync_stats["queued"] == 0 and sync_stats["drained"] == sync_stats["calls"]
    assert stats["calls"] == sync_stats["calls"] > 20
    assert stats["queued"] == stats["calls"] and stats["drained"] == 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # the results are not trivial, and the two Merkle forms agree
    assert np.array_equal(want["nodes"][8:], want["nodes2"][8:])
    assert np.all(want["y2"] == 7) and np.any(want["acc"] != INVALID) and np.any(want["big"] != INVALID)
    assert np.any(want["racc"] != INVALID) and len(set(want["ev13"].tolist())) > 30


# ---- ordering rules -------------------------------------------------------------------------------
def test_pool_reuse_in_stream_order(r, hal):
    """A deferred thread frees the input of an NTT that is still queued and takes the block again
    for a fill: the fill runs after the NTT (same stream), so the NTT's output is the
    synchronous run's. Another thread that allocates the same size meanwhile must not get that
    block: it is on the deferred thread's own pool until that thread drains."""
    L = r.lib()
    count, lg_out = 16, 20
    n_in, n_out = count << (lg_out - 2), count << lg_out

    def ntt(after_free=None):
        a, out = alloc(r, n_in), alloc(r, n_out)
        r.check(L.r0hip_fill_uniform(a, n_in, 77))
        r.check(L.r0hip_synchronize())
        r.check(L.r0hip_batch_expand_into_evaluate_ntt(out, a, count, lg_out, 2))
        free(r, a)
        b = None
        if after_free:
            b = after_free(a)
        got = read(r, out, n_out)
        free(r, out)
        return got, b

    want, _ = ntt()
    r.trim()  # no idle block of any size is left for thread 2 to find
    freed, checked = threading.Barrier(2), threading.Barrier(2)
    res = {}

    def thread1():
        try:
            hal.set_deferred(True)
            s0 = r.call_stats()

            def after_free(a):
                freed.wait(30)
                b = alloc(r, n_in)
                r.check(L.r0hip_memset32(b, 0x5A5A5A5, n_in))
                res["queued"] = delta(r, s0)
                checked.wait(30)  # thread 2 allocates before this thread drains
                res["a"], res["b"] = a, b
                return b
            res["out"], b = ntt(after_free)
            free(r, b)
            hal.set_deferred(False)
        except BaseException as e:  # noqa: BLE001
            res["err1"] = e
            freed.abort()
            checked.abort()

    def thread2():
        try:
            freed.wait(30)
            m0 = r.mem_stats()["mallocs"]
            p = alloc(r, n_in)
            r.check(L.r0hip_memset32(p, 0x3C3C3C3, n_in))
            res["p"], res["mallocs"] = p, r.mem_stats()["mallocs"] - m0
            checked.wait(30)
            free(r, p)
        except BaseException as e:  # noqa: BLE001
            res["err2"] = e
            freed.abort()
            checked.abort()

    ts = [threading.Thread(target=f) for f in (thread1, thread2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert "err1" not in res and "err2" not in res, res
    # alloc, alloc, fill | synchronize | expand + evaluate, free, alloc, memset32
    assert res["queued"] == {"calls": 8, "drained": 1, "queued": 7}
    assert res["b"] == res["a"], "the deferred thread's next allocation of that size takes the freed block"
    assert res["p"] != res["a"] and res["mallocs"] == 1, "thread 2 got fresh memory, not the block still in use"
    assert np.array_equal(res["out"], want)


def test_d2h_start_waits_for_queued_work(r, hal):
    """r0hip_memcpy_d2h_start copies on the copy stream; after a deferred fill of 2^26 words it
    must see the fill's last words, not what the buffer held before"""
    L = r.lib()
    n, tail = 1 << 26, 1024
    v1, v2 = 0x11111111, 0x22222222
    h = C.c_void_p()
    r.check(L.r0hip_host_alloc(C.byref(h), tail * 4))
    host = np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_uint32)), shape=(tail,))
    host[:] = 0
    d = alloc(r, n)
    try:
        r.check(L.r0hip_memset32(d, v1, n))
        r.check(L.r0hip_synchronize())
        with hal.deferred():
            s0 = r.call_stats()
            r.check(L.r0hip_memset32(d, v2, n))
            copy = C.c_void_p()
            r.check(L.r0hip_memcpy_d2h_start(h, d + (n - tail) * 4, tail * 4, C.byref(copy)))
            assert delta(r, s0) == {"calls": 2, "drained": 0, "queued": 2}
            done = C.c_int(0)
            r.check(L.r0hip_copy_finish(copy, 1, C.byref(done)))
            assert done.value == 1
            got = host.copy()
        assert np.all(got == v2), np.unique(got)
    finally:
        free(r, d)
        r.check(L.r0hip_host_free(h))


def test_validation_error_comes_from_the_failing_call(r, hal, sync_root):
    """a host-side check that fails in deferred mode is reported by that call, which drains; the
    mode stays on and later calls work (no device fault is involved: the size is rejected
    before anything is launched)"""
    L = r.lib()
    with hal.deferred():
        d = alloc(r, 16)
        s0 = r.call_stats()
        with pytest.raises(r.R0HipError, match="bad NTT size"):
            r.check(L.r0hip_batch_interpolate_ntt(d, 1, 28))
        assert delta(r, s0) == {"calls": 1, "drained": 1, "queued": 0}
        assert hal.set_deferred(True) is True
        free(r, d)
        s0 = r.call_stats()
        nodes = chain(r)
        assert delta(r, s0)["queued"] == CHAIN_CALLS
        root = read(r, nodes + 32, 8)
        free(r, nodes)
    assert np.array_equal(root, sync_root)


def test_memory_goes_back_at_the_drain(r, hal, sync_root):
    """Leaving the mode returns the thread's blocks: live bytes are what they were. A thread that
    runs the chain deferred, synchronises and exits leaves its blocks to the shared lists: the
    main thread's next chain allocates nothing new."""
    r.check(r.lib().r0hip_synchronize())
    live = r.mem_stats()["live"]
    with hal.deferred():
        free(r, chain(r))
    assert r.mem_stats()["live"] == live
    res = {}

    def worker():
        try:
            hal.set_deferred(True)
            res["root"] = chain_root(r)
            free(r, chain(r))  # leaves work queued
            r.check(r.lib().r0hip_synchronize())
        except BaseException as e:  # noqa: BLE001
            res["err"] = e

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "err" not in res, res
    assert np.array_equal(res["root"], sync_root)
    mallocs = r.mem_stats()["mallocs"]
    assert np.array_equal(chain_root(r), sync_root)
    assert r.mem_stats()["mallocs"] == mallocs
    assert r.mem_stats()["live"] == live


# ---- whole proofs ---------------------------------------------------------------------------------
def merkle_calls(po2):
    """hash_rows + hash_fold calls of one proof: log2(rows) + 1 per Merkle tree, over the three
    register groups and the check group (4 * 2^po2 rows each) and the FRI rounds (fri.rs:86-126)"""
    total = 4 * (po2 + 2 + 1)
    size = 1 << po2
    while size > 256:
        total += (size * 4 // 16).bit_length() - 1 + 1
        size //= 16
    return total


def _trace_job(r, t):
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    return r.TraceJob(t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                      bigint_records=t.bigint_records())


def test_rv32im_proof_deferred_matches_fused(r, oracle):
    """the loop guest at the smallest po2 its trace builds (14): the per-op path in deferred mode,
    natively and from Python, gives r0hip_prove_segment_trace's seal and mix, and the seal verifies"""
    import halprover
    import hal_prover
    po2 = 14
    hal = r.HipHal("poseidon2")
    t = T.loop_s_trace(po2, 64, seed=914)
    job = _trace_job(r, t)
    fused_seal, fused_mix = r.prove_segment_trace(hal, po2, job.glob, job.index, job.offsets, job.values, job.cycles,
                                                  job.txns, t.table_split_cycle, bigint=t.bigint_array(),
                                                  bigint_records=t.bigint_records())
    s0 = r.call_stats()
    seal, mix = halprover.prove_trace(hal, po2, job, deferred=True)
    assert delta(r, s0)["queued"] >= merkle_calls(po2)
    assert hal.set_deferred(False) is False  # the driver restored the caller's mode
    assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
    n = 1 << po2
    with hal.deferred():
        s0 = r.call_stats()
        data = hal.alloc_elem_init("data", 211 * n, INVALID)
        glob = hal.copy_from_elem("global", job.glob)
        hal.scatter(data, job.index, job.offsets, job.values)
        r.rv32im_witgen(data, glob, job.cycles, job.txns, t.table_split_cycle, bigint=t.bigint_array())
        hal.eltwise_zeroize_elem(data)
        hal.eltwise_zeroize_elem(glob)
        code = hal.alloc_elem_init("code", n, 0)
        accum = hal.alloc_elem("accum", 103 * n)

        def accumulate(mix_buf, mix_words):  # WitnessGenerator::accum (witgen/mod.rs:178-221)
            r.check(r.lib().r0hip_memset32(accum.ptr, INVALID, accum.size))
            r.bigint_accum_inject(accum, n, mix_words, t.bigint_records())
            r.check(r.lib().r0hip_rv32im_accum(data.ptr, accum.ptr, glob.ptr, mix_buf.ptr, n, 103, n))
            hal.eltwise_zeroize_elem(accum)
        pseal, pmix = hal_prover.prove_segment(oracle, hal, "rv32im", po2, code, data, accum, glob,
                                               accumulate=accumulate)
        assert delta(r, s0)["queued"] >= merkle_calls(po2)
        for b in (data, glob, code, accum):
            b.free()
    assert np.array_equal(pmix, fused_mix) and np.array_equal(pseal, fused_seal)
    assert r.verify_seal("rv32im", hal.suite, seal, check_validity=True) == po2


@pytest.mark.parametrize("suite", ["poseidon2", "sha-256"])
def test_recursion_proof_deferred_matches_fused(r, oracle, suite):
    """a random recursion program at po2 12: the per-op path in deferred mode, natively and from
    Python, gives r0hip_prove_recursion's seal and mix, and the seal verifies"""
    import halprover
    import hal_prover
    import recursion_program as RP
    if not RP.available():
        pytest.skip("oracle/_ref not built")
    hal = r.HipHal(suite)
    po2 = 12
    n, zk = 1 << po2, RP.ZK_CYCLES
    rng = np.random.default_rng(1212)
    prog, inp = RP.random_program(rng, n - zk - 1)
    pf = RP.preflight(prog, inp)
    wom, cyc, iops = RP.trace_arrays(pf)
    ctrl = hal.copy_from_elem("ctrl", RP.ctrl_group(prog, po2))
    seed = 0x5EED12
    fused_seal, fused_mix = r.prove_recursion(hal, po2, ctrl, wom, cyc, iops, seed)
    lib = r.lib()

    def witness():  # WitnessGenerator::new (circuit/recursion/src/prove/witgen.rs:44-133), per op
        data = hal.alloc_elem_init("data", RP.DATA * n, INVALID)
        glob = hal.alloc_elem_init("global", RP.OUT, INVALID)
        r.recursion_witgen(ctrl, data, glob, n, wom, cyc, iops)
        noise = hal.alloc_elem("noise", max(RP.DATA, RP.ACCUM) * zk)
        r.check(lib.r0hip_fill_uniform(noise.ptr, RP.DATA * zk, seed))
        r.check(lib.r0hip_eltwise_copy_elem_slice(data.ptr, noise.ptr, RP.DATA, zk, 0, zk, n - zk, n))
        hal.eltwise_zeroize_elem(data)
        accum = hal.alloc_elem_init("accum", RP.ACCUM * n, INVALID)
        r.check(lib.r0hip_fill_uniform(noise.ptr, RP.ACCUM * zk, seed + 1))
        r.check(lib.r0hip_eltwise_copy_elem_slice(accum.ptr, noise.ptr, RP.ACCUM, zk, 0, zk, n - zk, n))
        noise.free()
        return data, glob, accum

    with hal.deferred():
        data, glob, accum = witness()
        s0 = r.call_stats()
        seal, mix = halprover.prove_segment(hal, "recursion", po2, ctrl, data, accum, glob, accum_mode=2,
                                            work_cycles=len(prog.rows), deferred=True)
        assert delta(r, s0)["queued"] >= merkle_calls(po2)
        assert hal.set_deferred(True) is True  # the driver restored the caller's mode: still on
        for b in (data, glob, accum):
            b.free()
        data, glob, accum = witness()

        def accumulate(mix_buf, mix_words):  # prove/witgen.rs:162-177
            r.check(lib.r0hip_recursion_accum(ctrl.ptr, glob.ptr, data.ptr, mix_buf.ptr, accum.ptr, len(prog.rows), n))
            hal.eltwise_zeroize_elem(accum)
        s0 = r.call_stats()
        pseal, pmix = hal_prover.prove_segment(oracle, hal, "recursion", po2, ctrl, data, accum, glob,
                                               accumulate=accumulate)
        assert delta(r, s0)["queued"] >= merkle_calls(po2)
        for b in (data, glob, accum):
            b.free()
    ctrl.free()
    assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
    assert np.array_equal(pmix, fused_mix) and np.array_equal(pseal, fused_seal)
    assert r.verify_seal("recursion", hal.suite, seal, check_validity=True) == po2
