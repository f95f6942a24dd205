"""NTT register groups with unreduced multiplied operands (risc0_amd/csrc/ntt_bfly.h) against
the CPU oracle, word for word: batch_expand_into_evaluate_ntt at expand bits 0, 1, 2 and
batch_interpolate_ntt.

Sizes: log 1..14 are every row pass B = 1..13, hence every split of its stages into register
groups of 1..3 stages (with the first group's skipped twiddles), and the smallest two-pass size
(13-bit row pass + 1-bit column pass); 16 adds a column pass that runs its twiddles as running
products (B = 3); 22 is the workload's plan, a 13-bit row pass and a 9-bit column pass. Three
polynomials up to log 14 (ragged row-pass workgroups), two at 16 and 22.

Inputs, as stored Montgomery words, the same in every polynomial of a batch: all p - 1 (every
sum and difference at the top of its range), (p - 1, 0) alternating, zeros with one nonzero
word at the last index, and uniform random canonical words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 15 * 2**27 + 1
SIZES = list(range(1, 15)) + [16, 22]
KINDS = ("max", "alternating", "last", "random")


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def count_for(lg):
    return 3 if lg <= 14 else 2


def column(oracle, n, kind, seed):
    if kind == "max":
        return np.full(n, P - 1, np.uint32)
    if kind == "alternating":
        c = np.zeros(n, np.uint32)
        c[0::2] = P - 1
        return c
    if kind == "last":
        c = np.zeros(n, np.uint32)
        c[-1] = P - 1
        return c
    assert kind == "random", kind
    return oracle.rand_elems(np.random.default_rng(seed), n)


def batch(oracle, lg, count, kind, seed):
    return np.ascontiguousarray(np.tile(column(oracle, 1 << lg, kind, seed), count))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("expand_bits,lg_out", [(eb, lg) for eb in (0, 1, 2) for lg in SIZES if lg >= eb])
def test_expand_evaluate(hal, oracle, expand_bits, lg_out, kind):
    count = count_for(lg_out)
    a = batch(oracle, lg_out - expand_bits, count, kind, 7000 + 100 * expand_bits + lg_out)
    out = hal.alloc_elem("out", count << lg_out)
    src = hal.copy_from_elem("in", a)
    hal.batch_expand_into_evaluate_ntt(out, src, count, expand_bits)
    got = out.to_numpy()
    out.free()
    src.free()
    ref = np.zeros(count << lg_out, np.uint32)
    oracle.batch_expand_into_evaluate_ntt(ref, a, count, expand_bits)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", SIZES)
def test_interpolate(hal, oracle, lg, kind):
    count = count_for(lg)
    a = batch(oracle, lg, count, kind, 8000 + lg)
    d = hal.copy_from_elem("io", a)
    hal.batch_interpolate_ntt(d, count)
    got = d.to_numpy()
    d.free()
    oracle.batch_interpolate_ntt(a, count)
    assert np.array_equal(got, a)
