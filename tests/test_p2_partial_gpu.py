"""Poseidon2 on the GPU against the CPU oracle at the shapes where the permutation's callers
differ (risc0_amd/csrc/hash.hip): row hashing over one block, a padded block and the
multi-block sponge; a Merkle tree whose first fold layers take the two-nodes-per-lane kernel;
odd fold sizes. Bit-exact words, as in test_gpu_parity.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 15 * 2**27 + 1


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def words(oracle, rng, n, kind):
    """n stored words: all 0, all p - 1 (the largest canonical word), or random elements"""
    if kind == "random":
        return oracle.rand_elems(rng, n)
    return np.full(n, {"zero": 0, "max": P - 1}[kind], np.uint32)


def digests(rng, n):
    """digest words as test_hash_fold draws them (reduced words, some of them in [p, 2^31))"""
    return (rng.integers(0, 2**32, n * 8, dtype=np.uint64) // 3).astype(np.uint32)


@pytest.mark.parametrize("kind", ["random", "zero", "max", "mixed"])
@pytest.mark.parametrize("cols", [1, 15, 16, 17, 48, 211])
def test_hash_rows(hal, oracle, cols, kind):
    rows = 321  # five waves and a ragged one
    rng = np.random.default_rng(cols * 7 + len(kind))
    if kind == "mixed":
        pick = rng.integers(0, 3, rows * cols)
        m = np.choose(pick, [words(oracle, rng, rows * cols, k) for k in ("zero", "max", "random")]).astype(np.uint32)
    else:
        m = words(oracle, rng, rows * cols, kind)
    out = hal.alloc_digest("out", rows)
    hal.hash_rows(out, hal.copy_from_elem("m", m))
    ref = np.zeros(rows * 8, np.uint32)
    oracle.hash_rows(oracle.POSEIDON2, ref, m)
    assert np.array_equal(out.to_numpy(), ref)


def test_merkle_tree_two_node_layers(hal, oracle):
    """2^17 rows: the first fold layer (65536 nodes) is the smallest above the 32768-node
    quad threshold, so it runs two nodes per lane; the layers below run one quad per node"""
    rows, cols = 1 << 17, 3
    rng = np.random.default_rng(17)
    m = oracle.rand_elems(rng, rows * cols)
    nodes = hal.alloc_digest("nodes", rows * 2)
    hal.merkle_tree(nodes, hal.copy_from_elem("m", m), rows)
    io = np.zeros(rows * 2 * 8, np.uint32)
    leaves = np.zeros(rows * 8, np.uint32)
    oracle.hash_rows(oracle.POSEIDON2, leaves, m)
    io[rows * 8:] = leaves
    layer = rows
    while layer > 1:
        oracle.hash_fold(oracle.POSEIDON2, io, layer, layer // 2)
        layer //= 2
    assert np.array_equal(nodes.to_numpy()[8:], io[8:])


# 3 and 2049: odd counts below the quad threshold; 32771: an odd count above it (two nodes
# per lane with a lone last node)
@pytest.mark.parametrize("outputs", [3, 2049, 32771])
def test_hash_fold_odd(hal, oracle, outputs):
    rng = np.random.default_rng(outputs)
    io = np.zeros(outputs * 4 * 8, np.uint32)
    io[outputs * 2 * 8:] = digests(rng, outputs * 2)
    d = hal.copy_from_digest("io", io)
    hal.hash_fold(d, outputs * 2, outputs)
    oracle.hash_fold(oracle.POSEIDON2, io, outputs * 2, outputs)
    assert np.array_equal(d.to_numpy(), io)


_ONE_PER_LANE = """
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/oracle")
import oracle, risc0_amd as r
outputs = 32771
rng = np.random.default_rng(5)
io = np.zeros(outputs * 4 * 8, np.uint32)
io[outputs * 2 * 8:] = (rng.integers(0, 2**32, outputs * 2 * 8, dtype=np.uint64) // 3).astype(np.uint32)
hal = r.HipHal("poseidon2")
d = hal.copy_from_digest("io", io)
hal.hash_fold(d, outputs * 2, outputs)
oracle.hash_fold(oracle.POSEIDON2, io, outputs * 2, outputs)
assert np.array_equal(d.to_numpy(), io)
print("ONE_PER_LANE_OK")
"""


def test_hash_fold_one_node_per_lane(oracle):
    """The one-node-per-lane fold kernel is chosen by R0_P2_FOLD_TWO=0, which the library reads
    once per process: a child process runs an odd layer above the quad threshold through it."""
    env = dict(os.environ, R0_P2_FOLD_TWO="0")
    out = subprocess.run([sys.executable, "-c", _ONE_PER_LANE.format(root=ROOT)], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "ONE_PER_LANE_OK" in out.stdout, out.stdout + out.stderr
