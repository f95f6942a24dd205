"""r0hip_merkle_paths_host: the nodes MerkleTreeProver::prove reads for an opening
(prove/merkle.rs:108-140), fetched from a device node heap in one call.

The kernel only gathers, so the heaps here are random u32 words uploaded as they are and the
reference is numpy indexing of the same words: out[i, 0] = heap[j], out[i, k] = heap[(j >> k) ^ 1]
for j = idx[i]. The sizes are the smallest heaps (4 and 8 digests: every node and every legal
depth), one of more than a block of path words with the deepest legal path (2^11), and a tree of
2^20 rows (2^21 digests) with the 15 levels its openings read under top_size 32 and the deepest
20. Errors are host-side validation and name the index; deferred mode drains."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    import risc0_amd
    return risc0_amd


@pytest.fixture(scope="module")
def hal(r):
    return r.HipHal("poseidon2")


@pytest.fixture(autouse=True)
def default_mode_after(r):
    yield
    r.check(r.lib().r0hip_set_deferred(0, None))


def expected(heap, idx, levels):
    """heap: (digests, 8) host words; the paths as the header defines them"""
    out = np.zeros((len(idx), levels, 8), np.uint32)
    for i, j in enumerate(idx):
        j = int(j)
        for k in range(levels):
            out[i, k] = heap[j if k == 0 else (j >> k) ^ 1]
    return out


def make_heap(hal, digests, seed):
    host = np.random.default_rng(seed).integers(0, 1 << 32, size=(digests, 8), dtype=np.uint64).astype(np.uint32)
    return host, hal.copy_from_digest("nodes", host)


@pytest.fixture(scope="module")
def big(hal):
    """a heap of 2^21 digests (a tree of 2^20 rows), shared and never written"""
    return make_heap(hal, 1 << 21, 21)


@pytest.mark.parametrize("digests,idx,levels", [
    (4, [1, 2, 3], 1),
    (8, [4, 5, 6, 7], 1),
    (8, [4, 5, 6, 7], 2),
    (8, [1], 1),
    (1 << 11, [1 << 10, (1 << 11) - 1], 10),
])
def test_small_heaps_match_numpy(hal, digests, idx, levels):
    host, dev = make_heap(hal, digests, digests + levels)
    got = hal.merkle_paths_host(dev, idx, levels)
    assert got.shape == (len(idx), levels, 8)
    assert np.array_equal(got, expected(host, idx, levels))
    dev.free()


def test_tree_of_2_20_rows(hal, big):
    """50 seeded leaves, one pair duplicated, at the 15 levels an opening of 2^20 rows reads
    down to top_size 32; the last leaf at the deepest legal path of 20"""
    host, dev = big
    rows = 1 << 20
    idx = rows + np.random.default_rng(50).integers(0, rows, size=50)
    idx[37] = idx[3]
    assert np.array_equal(hal.merkle_paths_host(dev, idx, 15), expected(host, idx, 15))
    last = [2 * rows - 1]
    assert np.array_equal(hal.merkle_paths_host(dev, last, 20), expected(host, last, 20))


def test_no_indices_is_a_no_op(r, hal, big):
    _, dev = big
    assert hal.merkle_paths_host(dev, [], 15).shape == (0, 15, 8)
    # nothing is dereferenced: null pointers pass
    r.check(r.lib().r0hip_merkle_paths_host(None, None, 0, None, 0, 0))


def test_pageable_and_page_locked_destinations(r, hal, big):
    """the same words land in numpy (pageable) memory and in an r0hip_host_alloc block"""
    host, dev = big
    L = r.lib()
    idx = np.array([(1 << 20) + 12345, (1 << 21) - 2, 1 << 20], np.uint64)
    want = expected(host, idx, 15)
    pageable = np.zeros(want.shape, np.uint32)
    r.check(L.r0hip_merkle_paths_host(pageable.ctypes.data, dev.ptr, dev.size, idx.ctypes.data, idx.size, 15))
    assert np.array_equal(pageable, want)
    block = C.c_void_p()
    r.check(L.r0hip_host_alloc(C.byref(block), want.nbytes))
    try:
        r.check(L.r0hip_merkle_paths_host(block.value, dev.ptr, dev.size, idx.ctypes.data, idx.size, 15))
        pinned = np.ctypeslib.as_array(C.cast(block.value, C.POINTER(C.c_uint32)), shape=(want.size,)).copy()
    finally:
        r.check(L.r0hip_host_free(block.value))
    assert np.array_equal(pinned.reshape(want.shape), want)


@pytest.mark.parametrize("idx,levels,names", [
    ([5, 0, 6], 1, "index 0 (h_idx[1])"),          # node 0 is not a node
    ([4, 8], 2, "index 8 (h_idx[1])"),             # == heap_digests
    ([5], 0, "levels = 0"),
    ([6, 5], 3, "index 6 (h_idx[0])"),             # one too deep: (6 >> 2) = 1 is the root, it has no sibling
])
def test_errors_name_the_index_and_leave_the_library_usable(r, hal, idx, levels, names):
    host, dev = make_heap(hal, 8, 8)
    with pytest.raises(r.R0HipError) as e:
        hal.merkle_paths_host(dev, idx, levels)
    assert names in str(e.value), str(e.value)
    assert np.array_equal(hal.merkle_paths_host(dev, [4, 7], 2), expected(host, [4, 7], 2))
    dev.free()


def test_deferred_mode_drains_and_sees_queued_work(r, hal):
    """a hash_fold layer queued onto a heap, then the path fetch straight after it: the fetch
    drains (one more drained call, the fold stays counted as queued) and returns the digests the
    same two calls give in the default mode"""
    L = r.lib()
    digests = 1 << 9
    host = np.random.default_rng(9).integers(0, 15 * 2**27 + 1, size=(digests, 8), dtype=np.uint64).astype(np.uint32)
    idx = np.array([128, 200, 255], np.uint64)  # the layer the fold writes: nodes [128, 256)

    def run():
        dev = hal.copy_from_digest("nodes", host)
        s0 = r.call_stats()
        r.check(L.r0hip_hash_fold(hal.suite, dev.ptr, 256, 128))
        s1 = r.call_stats()
        out = hal.merkle_paths_host(dev, idx, 7)
        s2 = r.call_stats()
        dev.free()
        return out, {k: s1[k] - s0[k] for k in s0}, {k: s2[k] - s1[k] for k in s0}

    sync, fold_sync, fetch_sync = run()
    assert fold_sync == {"calls": 1, "drained": 1, "queued": 0} and fetch_sync == fold_sync
    assert not np.array_equal(sync[:, 0], host[idx.astype(np.int64)])  # the fold really wrote these nodes
    assert np.array_equal(sync[:, 1:], expected(host, idx, 7)[:, 1:])  # and nothing above them
    with hal.deferred():
        deferred, fold_def, fetch_def = run()
    assert fold_def == {"calls": 1, "drained": 0, "queued": 1}
    assert fetch_def == {"calls": 1, "drained": 1, "queued": 0}
    assert np.array_equal(deferred, sync)
