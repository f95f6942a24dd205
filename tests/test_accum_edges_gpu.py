"""The accumulation kernels at worst-case words, ragged tiles and scan carries.

test_gpu_parity.py runs r0hip_rv32im_accum, r0hip_recursion_accum and r0hip_demo_accum on
uniformly random words at a few power-of-two sizes, mostly against oracle/_ref. This module
closes what that leaves, with the bar of test_gpu_op_edges.py: np.array_equal on the whole
buffer of u32 words, the INVALID cells no kernel may touch included, against references that
need no oracle/_ref (one case excepted, below). Inputs and references: tests/accum_edges.py.

Which shape reaches which branch:

rv32im step (gen/rvaccum, four arm-sorted kernels of 256-lane tiles; tile_sort_lane<256>):
  * words `max` (every word p - 1): a fused sum over loaded words has every product at
    (p - 1)^2 and runs at the bound tools/gen_accum.py:fuse_sums folds by; `mixed` adds 0, 1,
    p - 2 and the words of +-1 (zero factors, carries of fp_add / fp_sub at both ends). Of
    the 1783 fold64 steps of the build's settings, deleting any one of 495 (each the fold in
    front of a REDC) changes a stored word on the `max` cases, and none does on random words.
    Sums over derived values (products, powers of the mix) cannot be driven to the bound by
    any stored words; the 72 folds inside a sum are all of that sort (the BigInt arm), and
    rest on the exact bound tests/test_accum_fuse.py checks.
  * mix `holes`: every second FpExt of the mix is zero, so a row's fp_inv_batch gets zero and
    non-zero inputs together (asserted on the CPU side of test_rv32im_step_zeros_in_inverse_batches).
  * rows 4, 8, 16: less than a wave; 64: one wave of a 256-lane tile, the other lanes sort
    behind every arm (key K) and return. last = rows - 1 and 1: lanes past `last` inside the
    only wave. rows 512 with last 63, 64, 65 (one lane either side of a wave), 255, 256, 257
    (of a tile; 257 is a second workgroup with one live lane), 511.
  * arm patterns at 512 rows: each tile one arm (every other `if (arm)` block skipped by all
    four waves; arm 12 then arm 0: the last and the first key), descending arms (the counting
    sort reverses the tile), 64-row runs per arm (already sorted: the identity permutation),
    two arms alternating (two keys, 128 lanes each).
  * 256 rows of one arm alone, for each of the 13: that arm's cone on worst-case words with
    nothing else stored; every accum cell its arm does not store stays INVALID through the
    step, and phases 2-3 then add to it as raw words exactly as the oracle does.
recursion step (gen/accum) and its product scan (recursion_accum.hip, tiles of 1024 steps):
  * po2 4 and 10 with steps n and n - 3 on `max` / `mixed` words, mix same or `holes`: one
    tile, ragged lanes; po2 11 with steps 1023, 1024, 1025: one lane short of a tile, a whole
    tile, a second tile of one step (scan_products_kernel with ntiles 2).
  * po2 19 with steps 2^18 + 1: 257 tiles, scan_products_kernel's second batch of 256.
scans over tile sums, second and third batch (`for (b = 0; b < ntiles; b += 256)` with carry):
  * r0hip_rv32im_accum_finalize (tiles of 4096 rows), last 2^20, 2^20 + 1, 2^20 + 4097,
    2^21 + 1: 256 tiles (one batch), 257 and 258 (second batch, one and two live lanes),
    513 (third batch: the first whose incoming carry is not zero-plus-one-term).
  * r0hip_demo_accum (tiles of 1024 rows) at po2 19, n 2^18, 2^18 + 1, 2^18 + 1025, 2^19:
    256, 257, 258 and 512 tiles, and at po2 20 with n 2^19 + 1: 513 tiles, the third batch.
  * combos_divide, three rows of 2^20 + 16 cycles: 257 blocks per row, so div_top_kernel
    runs two segments per row at offsets row * nblocks.

A failure here that tests/test_gen_accum_source.py::test_generated_source_worst_case_words
does not show on the same words is the device code's, not the generator's.
"""
import os
import time

import numpy as np
import pytest

import accum_edges as E
import accum_ir as A

pytestmark = pytest.mark.gpu

P, INVALID = E.P, E.INVALID


@pytest.fixture(scope="module")
def hal():
    import risc0_amd as r
    return r.HipHal("poseidon2")


def test_constants(oracle):
    assert P == oracle.P and E.R_MONT == int(oracle.encode(1))


def assert_same_words(got, ref, rows):
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{bad.size} words differ, first at column {bad[0] // rows} row {bad[0] % rows}: " \
                          f"{got[bad[0]]:#x}, expected {ref[bad[0]]:#x}"
    assert np.array_equal(got, ref)


# ---- rv32im: the generated step, then phases 2-3 ----------------------------------------------
def check_rv32im(hal, oracle, seed, rows, last, arms, kind, mix_kind):
    data, glob, mix = E.rv_case(seed, rows, arms, kind, mix_kind)
    ref = E.rv_reference(oracle, data, glob, mix, rows, last)
    assert (ref[(E.RV_ACCUM_COLS - 4) * rows:].reshape(4, rows)[:, :last] < P).all()  # the scanned columns are all stored
    d_acc = hal.alloc_elem_init("accum", E.RV_ACCUM_COLS * rows, INVALID)
    hal.rv32im_accum(hal.copy_from_elem("data", data), d_acc, hal.copy_from_elem("global", glob),
                     hal.copy_from_elem("mix", mix), rows, last)
    assert_same_words(d_acc.to_numpy(), ref, rows)


RV_WORST_SHAPES = [("all13", 512)] + [(a, 256) for a in range(E.RV_ARMS)]


@pytest.mark.parametrize("mix_kind", ["same", "holes"])
@pytest.mark.parametrize("kind", ["max", "mixed"])
@pytest.mark.parametrize("arm,rows", RV_WORST_SHAPES)
def test_rv32im_step_worst_case_words(hal, oracle, arm, rows, kind, mix_kind):
    """A1: 512 rows over arms r % 13, and 256 rows of each arm alone"""
    arms = np.arange(rows) % 13 if arm == "all13" else np.full(rows, arm)
    check_rv32im(hal, oracle, 1000 + rows + len(kind), rows, rows, arms, kind, mix_kind)


RV_SHAPES = [(rows, last) for rows in (4, 8, 16, 64) for last in (rows, rows - 1, 1)] + \
            [(512, last) for last in (63, 64, 65, 255, 256, 257, 511)]


@pytest.mark.parametrize("rows,last", RV_SHAPES)
def test_rv32im_step_shapes(hal, oracle, rows, last):
    """A2: below a wave, below a tile, `last` one either side of a wave and of a tile; random
    words, random arms"""
    rng = np.random.default_rng(2000 + 7 * rows + last)
    check_rv32im(hal, oracle, 2000 + rows + last, rows, last, rng.integers(0, E.RV_ARMS, rows), "random", "same")


def arm_pattern(name, rows):
    r = np.arange(rows)
    return {"tile_per_arm": np.where(r < 256, 12, 0),  # tile 0 on arm 12, tile 1 on arm 0
            "descending": 12 - r % 13,
            "runs_of_64": (r // 64) % 13,
            "alternating": np.where(r % 2 == 0, 3, 9)}[name]


@pytest.mark.parametrize("pattern", ["tile_per_arm", "descending", "runs_of_64", "alternating"])
def test_rv32im_step_arm_patterns(hal, oracle, pattern):
    """A2: what the tile's counting sort sees, two tiles of 256 rows"""
    rows = 512
    check_rv32im(hal, oracle, 2100 + len(pattern), rows, rows, arm_pattern(pattern, rows), "random", "same")


def test_rv32im_step_zeros_in_inverse_batches(hal, oracle):
    """A3: 64 `mixed` rows over arms r % 13 with the `holes` mix, default_rng(5). First the
    condition that gives every `holes` case its meaning, on the CPU: rows hand the step's
    inverses zero and non-zero inputs together (and with the mix of the rows' kind no inverse
    sees a zero). Then the same inputs on the card."""
    rows, arms = 64, np.arange(64) % 13
    for mix_kind, want_both in (("holes", True), ("same", False)):
        data, glob, mix = E.rv_case(5, rows, arms, "mixed", mix_kind)
        seen = E.InverseInputs(rows)
        E.rv_step_reference(data, glob, mix, rows, rows, on_inv=seen)
        print(f"{mix_kind}: {seen.ops_with_zero} of {seen.ops} inverses see a zero on some row, "
              f"{seen.rows_with_both()} of {rows} rows hold both")
        assert seen.ops > 0
        assert (seen.rows_with_both() >= 1) == want_both
    check_rv32im(hal, oracle, 5, rows, rows, arms, "mixed", "holes")


# ---- recursion ---------------------------------------------------------------------------------
def check_recursion(hal, oracle, seed, po2, steps, kind, mix_kind, reference):
    d = A.circuit()
    gs, n = d["group_sizes"], 1 << po2
    ctrl, glob, data, mix = E.recursion_case(seed, oracle, po2, gs, d["output_size"], d["mix_size"], kind, mix_kind)
    acc0 = np.full(gs[0] * n, INVALID, np.uint32)
    ref = reference(ctrl, glob, data, mix, acc0, steps, n)
    dacc = hal.copy_from_elem("accum", acc0)
    hal.recursion_accum(hal.copy_from_elem("ctrl", ctrl), hal.copy_from_elem("global", glob),
                        hal.copy_from_elem("data", data), hal.copy_from_elem("mix", mix), dacc, steps, n)
    assert_same_words(dacc.to_numpy(), ref, n)


@pytest.mark.parametrize("mix_kind", ["same", "holes"])
@pytest.mark.parametrize("kind", ["max", "mixed"])
@pytest.mark.parametrize("po2,short", [(4, 0), (4, 3), (10, 0), (10, 3)])
def test_recursion_accum_worst_case_words(hal, oracle, po2, short, kind, mix_kind):
    """A4, against the numpy IR with the Python prefix product"""
    check_recursion(hal, oracle, 3000 + po2 + short, po2, (1 << po2) - short, kind, mix_kind, A.accum)


@pytest.mark.parametrize("steps", [1023, 1024, 1025])
def test_recursion_accum_tile_boundary(hal, oracle, steps):
    check_recursion(hal, oracle, 3100 + steps, 11, steps, "random", "same", A.accum)


def test_recursion_accum_second_scan_batch(hal, oracle):
    """A5: 257 tile products. Against the compiled reference (the Python prefix product and the
    interpreter's per-op arrays are too large here): the one case of this module that needs
    oracle/_ref"""
    if not os.path.exists(os.path.join(A.ROOT, "oracle", "_ref", "libref_recursion.so")):
        pytest.skip("oracle/_ref/libref_recursion.so not built")

    def compiled(ctrl, glob, data, mix, acc0, steps, n):
        ref = acc0.copy()
        A.ref_accum(ctrl, glob, data, mix, ref, steps, n)
        return ref

    t0 = time.time()
    check_recursion(hal, oracle, 3200, 19, (1 << 18) + 1, "random", "same", compiled)
    print(f"recursion po2 19, 2^18 + 1 steps: {time.time() - t0:.1f} s with its reference")


# ---- scans over tile sums: second and third batch -------------------------------------------
FINALIZE_COLS = 31  # 0..22 not touched, 23..26 the one machine group, 27..30 the prefix columns


def check_finalize(hal, oracle, rows, last, kind):
    t0 = time.time()
    a = E.words(np.random.default_rng(4000 + last % 9973), rows * FINALIZE_COLS, kind)
    d = hal.copy_from_elem("accum", a)
    t1 = time.time()
    hal.rv32im_accum_finalize(d, rows, FINALIZE_COLS, last)
    got = d.to_numpy()
    t2 = time.time()
    d.free()
    ref = a.copy()
    oracle.rv32im_accum_finalize(ref, rows, FINALIZE_COLS, E.RV_SPLIT, last)
    print(f"finalize rows {rows} last {last} {kind}: device call and download {t2 - t1:.2f} s, all {time.time() - t0:.2f} s")
    g, r0 = got.reshape(FINALIZE_COLS, rows), a.reshape(FINALIZE_COLS, rows)
    assert np.array_equal(g[:E.RV_SPLIT], r0[:E.RV_SPLIT])
    assert np.array_equal(g[:, last:], r0[:, last:])
    assert_same_words(got, ref, rows)


@pytest.mark.parametrize("kind", ["random", "max"])
@pytest.mark.parametrize("last", [1 << 20, (1 << 20) + 1, (1 << 20) + 4097, (1 << 21) + 1])
def test_rv32im_accum_finalize_scan_batches(hal, oracle, last, kind):
    """A5: 256, 257, 258 and 513 tiles of 4096 rows; rows = last, no power of two"""
    check_finalize(hal, oracle, last, last, kind)


def test_rv32im_accum_finalize_rows_past_last(hal, oracle):
    check_finalize(hal, oracle, (1 << 21) + 64, (1 << 21) + 1, "random")


@pytest.mark.parametrize("kind", ["random", "max"])
@pytest.mark.parametrize("po2,n", [(19, 1 << 18), (19, (1 << 18) + 1), (19, (1 << 18) + 1025), (19, 1 << 19),
                                   (20, (1 << 19) + 1)])
def test_demo_accum_scan_batches(hal, po2, n, kind):
    """A5: 256, 257, 258, 512 and 513 tiles of 1024 rows; column `a` uploaded, no witness
    kernel. demo_scan_sums_kernel's carry is zero until the second batch has been added, so only
    513 tiles tell `carry + total` from `total`."""
    import demo_air as D
    from risc0_amd import hal as H
    rows = 1 << po2
    data = E.words(np.random.default_rng(5000 + n % 9973), 3 * rows, kind)
    mix = [P - 1, 1, 0, 123456789]
    acc = hal.alloc_elem_init("accum", 4 * rows, INVALID)
    H.demo_accum(po2, n, hal.copy_from_elem("data", data), D.enc(mix), acc)
    want = D.enc(D.accumulate(po2, n, D.dec(data), mix))
    for k in range(4):
        want[k * rows + n:(k + 1) * rows] = INVALID  # untouched
    assert_same_words(acc.to_numpy(), want, rows)


@pytest.mark.parametrize("kind", ["random", "max"])
def test_combos_divide_three_rows_two_segments(hal, oracle, kind):
    """A5: three chunks of one row each, 2^20 + 16 cycles = 65537 lanes = 257 blocks per row"""
    cycles = (1 << 20) + 16
    rng = np.random.default_rng(6000)
    combos = E.words(rng, 3 * 4 * cycles, kind)
    z = E.words(rng, 3 * 4, "random")
    begin = np.array([0, 1, 2, 3], np.uint32)
    d = hal.copy_from_extelem("combos", combos)
    bad_gpu = hal.combos_divide(d, z, begin, cycles)
    got = d.to_numpy()
    d.free()
    bad_ref = oracle.combos_divide(combos, z, begin, cycles)
    assert bad_gpu == bad_ref
    assert_same_words(got, combos, 4 * cycles)
