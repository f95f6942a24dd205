"""The per-op driver's node-heap mirrors under a budget (halp_set_mirror_budget), with one
r0hip_merkle_paths_host call per opening as the fallback (integration/hal_prover.cpp Buf::at,
integration/node_reads.h): whatever the budget, the seal and the mix are the fused prover's, and
halp_mirror_stats tells which way the node reads went.

A node heap is 256 * 2^po2 bytes. Budgets: 0 (no mirror at all), exactly one heap (the code tree,
built first and alive to the end, takes it; every later tree falls back) and the default 4 GiB
(at these sizes every tree mirrors; at po2 22 the four big heaps fill it to the byte and the FRI
trees fall back)."""
import os
import sys
import time

import numpy as np
import pytest

import rv32im_trace as T

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration"))

P = 15 * 2**27 + 1
QUERIES = 50
COLS = {"code": 1, "data": 211, "accum": 103}


@pytest.fixture(scope="module")
def r():
    import risc0_amd
    return risc0_amd


@pytest.fixture(scope="module")
def hal(r):
    return r.HipHal("poseidon2")


@pytest.fixture(scope="module")
def hp():
    import halprover
    return halprover


@pytest.fixture(autouse=True)
def default_budget_after(r, hp):
    yield
    hp.set_mirror_budget(hp.DEFAULT_MIRROR_BUDGET)
    r.check(r.lib().r0hip_set_deferred(0, None))


def trees(po2):
    """the code, data, accum and check trees and one per FRI round (fri.rs:86-126)"""
    n, size = 4, 1 << po2
    while size > 256:
        n, size = n + 1, size // 16
    return n


def output_size(hp):
    return hp.CircuitTaps("rv32im").struct.output_size


@pytest.fixture(scope="module", params=[10, 13])
def random_groups(request, r, hal, hp):
    """seeded random witness groups on the device, and the fused prover's seal and mix of them"""
    po2 = request.param
    rng = np.random.default_rng(0xB0D6E7 + po2)
    n = 1 << po2
    dev = {k: hal.copy_from_elem(k, rng.integers(0, P, size=c * n, dtype=np.uint32)) for k, c in COLS.items()}
    glob = rng.integers(0, P, size=output_size(hp), dtype=np.uint32)
    seal, mix = r.prove_segment(hal, "rv32im", po2, dev["code"], dev["data"], dev["accum"],
                                hal.copy_from_elem("global", glob))
    return po2, dev, glob, seal, mix


def per_op(hal, hp, po2, dev, glob, budget):
    hp.set_mirror_budget(budget)
    hp.mirror_stats(reset=True)
    seal, mix = hp.prove_segment(hal, "rv32im", po2, dev["code"], dev["data"], dev["accum"],
                                 hal.copy_from_elem("global", glob), accum_mode=0)
    return seal, mix, hp.mirror_stats()


def test_seal_is_the_fused_seal_under_every_budget(hal, hp, random_groups):
    po2, dev, glob, fused_seal, fused_mix = random_groups
    heap = 256 << po2
    # budget 0: no mirror, one device call per opening
    seal, mix, s = per_op(hal, hp, po2, dev, glob, 0)
    print(f"po2={po2} budget 0: {s}")
    assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
    assert s["mirrors_started"] == 0 and s["peak_mirror_bytes"] == 0
    assert s["mirrors_refused"] == trees(po2)
    assert 0 < s["path_fetches"] <= QUERIES * trees(po2)
    # exactly one heap: the first tree mirrors, the rest fetch
    seal, mix, s = per_op(hal, hp, po2, dev, glob, heap)
    print(f"po2={po2} budget {heap}: {s}")
    assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
    assert s["mirrors_started"] > 0 and s["path_fetches"] > 0 and s["mirrors_refused"] > 0
    assert 0 < s["peak_mirror_bytes"] <= heap
    # the default: as before the budget existed
    seal, mix, s = per_op(hal, hp, po2, dev, glob, hp.DEFAULT_MIRROR_BUDGET)
    print(f"po2={po2} default budget: {s}")
    assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
    assert s["path_fetches"] == 0 and s["mirrors_refused"] == 0 and s["path_cache_hits"] == 0
    assert s["mirrors_started"] == trees(po2)


def test_loop_guest_trace_without_mirrors_sync_and_deferred(r, hal, hp):
    """prove_core from the loop guest's trace at po2 16 with budget 0, in the default and the
    deferred completion mode: the fused seal, and a valid one"""
    po2 = 16
    t = T.loop_s_trace(po2, T.loop_s_iterations(po2) - 11, seed=900 + po2)
    cyc, tx = t.arrays()
    idx, off, val = t.injector_arrays()
    job = r.TraceJob(t.global_words(), idx, off, val, cyc, tx, t.table_split_cycle, bigint=t.bigint_array(),
                     bigint_records=t.bigint_records())
    fused_seal, fused_mix = r.prove_segment_trace(hal, po2, job.glob, job.index, job.offsets, job.values, job.cycles,
                                                  job.txns, t.table_split_cycle, bigint=t.bigint_array(),
                                                  bigint_records=t.bigint_records())
    hp.set_mirror_budget(0)
    for deferred in (False, True):
        hp.mirror_stats(reset=True)
        seal, mix = hp.prove_trace(hal, po2, job, deferred=deferred)
        s = hp.mirror_stats()
        assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal), deferred
        assert s["mirrors_started"] == 0 and 0 < s["path_fetches"] <= QUERIES * trees(po2), (deferred, s)
        assert r.verify_seal("rv32im", r.POSEIDON2, seal, check_validity=True) == po2


def test_po2_22_under_the_default_budget(r, hal, hp):
    """the size the budget exists for: the four 1 GiB heaps fill the default 4 GiB, the FRI
    trees are refused and fetch paths, and the seal is still the fused one"""
    po2 = 22
    n = 1 << po2
    dev = {k: hal.alloc_elem(k, c * n) for k, c in COLS.items()}
    for i, b in enumerate(dev.values()):
        r.check(r.lib().r0hip_fill_uniform(b.ptr, b.size, 0x2200 + i))
    glob = np.random.default_rng(22).integers(0, P, size=output_size(hp), dtype=np.uint32)
    try:
        t0 = time.perf_counter()
        fused_seal, fused_mix = r.prove_segment(hal, "rv32im", po2, dev["code"], dev["data"], dev["accum"],
                                                hal.copy_from_elem("global", glob))
        t1 = time.perf_counter()
        seal, mix, s = per_op(hal, hp, po2, dev, glob, hp.DEFAULT_MIRROR_BUDGET)
        t2 = time.perf_counter()
        print(f"po2=22: fused {t1 - t0:.2f} s, per-op {t2 - t1:.2f} s, {s}")
        assert np.array_equal(mix, fused_mix) and np.array_equal(seal, fused_seal)
        assert s["mirrors_refused"] >= 1 and s["path_fetches"] > 0
        assert 0 < s["peak_mirror_bytes"] <= 4 << 30
    finally:
        for b in dev.values():
            b.free()
        r.trim()
