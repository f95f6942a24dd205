"""Hand-encoded recursion programs for the native preflight (r0hip_recursion_preflight): small
programs that each pin one corner of Preflight::step (prove/preflight.rs:181-627), and programs
whose run must fail with a given message at a given cycle. Test infrastructure only.

`CASES` maps a name to (program, input); `ERRORS` maps a name to (program, input, po2, message
pattern with the cycle). `write_cases(path)` dumps both for tests/native/recursion_preflight_host.cpp:
per case one line `name po2 n_code n_input` and one line of code words then input words.
"""
import numpy as np

import recursion_program as RP
from recursion_program import (ADD, CONST, EQ, EXTRACT, INV, MIX_RNG, MUL, P, READ_IOP_BODY, READ_IOP_HEADER, SELECT,
                               SUB, Program)

ZK = RP.ZK_CYCLES


def _consts(p, wa, vals):
    """CONST rows from address wa: three (lo, hi) pairs per row"""
    for i in range(0, len(vals), 3):
        p.micro(wa + i, [(CONST, a, b, 0) for a, b in vals[i:i + 3]])


def one_row():
    p = Program()
    p.micro(0, [(CONST, 5, 6, 0)])
    return p, []


def full_po2_11():
    """exactly 2^11 - 1024 rows: wom_init, CONST rows over a contiguous WOM, wom_fini"""
    p = Program()
    p.macro("wom_init")
    for r in range((1 << 11) - ZK - 2):
        p.micro(1 + 3 * r, [(CONST, r + 1, r, 0), (CONST, 2 * r, 1, 0), (CONST, 7, 7, 0)])
    p.macro("wom_fini", 1 + 3 * ((1 << 11) - ZK - 2))
    assert len(p.rows) == (1 << 11) - ZK
    return p, []


def iop_headers():
    """READ_IOP_HEADER with k = 0, 1, 2, 3, 4 and 5 (a poly longer than an FpExt is cut), flip 0
    and 1, count 1 and 3; bodies with and without do_mont; every body value read"""
    rng = np.random.default_rng(1)
    p, inp, wa = Program(), [], 0
    for k in (1, 2, 3, 4, 5, 0):
        for flip in (0, 1):
            for count in (1, 3):
                n = count if k == 2 else k * count
                words = rng.integers(0, 1 << 32, n) if k == 2 else rng.integers(0, P, n)
                inp += [int(x) for x in words]
                p.micro(wa, [(READ_IOP_HEADER, count, 2 * k + flip, 0)])
                wa += 3
                for i in range(count):
                    p.micro(wa, [(READ_IOP_BODY, 0, 0, (i + flip) % 2)])
                    wa += 3
    return p, inp


def iop_raw_words():
    """input words at and above p enter as Fp::new_raw does: the element of the word mod p"""
    p = Program()
    p.micro(0, [(READ_IOP_HEADER, 2, 2 * 4, 0)])
    p.micro(3, [(READ_IOP_BODY, 0, 0, 1), (READ_IOP_BODY, 0, 0, 0)])
    return p, [P, P + 1, 2**32 - 1, 2**31, 0, 1, P - 1, 5]


def select_corners():
    """SELECT landing on index 0 (a[2] * x = 0) and on a non-zero index"""
    p = Program()
    _consts(p, 0, [(11, 1), (22, 2), (33, 3), (0, 0), (2, 0), (1, 9)])
    p.micro(6, [(SELECT, 3, 0, 1), (SELECT, 4, 0, 1), (SELECT, 5, 0, 2)])  # cells 0, 2, 2
    p.micro(9, [(SELECT, 4, 1, 0), (SELECT, 3, 5, 7), (CONST, 0, 0, 0)])   # cells 1, 5
    return p, []


def extract_corners():
    p = Program()
    _consts(p, 0, [(3, 4)])
    p.micro(3, [(MUL, 0, 0, 0), (MUL, 3, 0, 0), (CONST, 0, 0, 0)])  # 4: all four limbs set
    p.micro(6, [(EXTRACT, 4, 0, 0), (EXTRACT, 4, 0, 1), (EXTRACT, 4, 1, 0)])
    p.micro(9, [(EXTRACT, 4, 1, 1), (EXTRACT, 4, 2, 3), (EXTRACT, 4, P - 1, 5)])  # and off the corners
    return p, []


def inv_modes():
    """INV as is_zero (mode 0) of zero, of a non-zero element and of (0, x); as the inverse
    (mode 1, and any other non-zero mode) of an element, an extension element and zero"""
    p = Program()
    _consts(p, 0, [(0, 0), (7, 0), (0, 5), (3, 4), (P - 1, 0), (1, 0)])
    p.micro(6, [(INV, 0, 0, 0), (INV, 1, 0, 0), (INV, 2, 0, 0)])
    p.micro(9, [(INV, 1, 1, 0), (INV, 3, 1, 0), (INV, 0, 1, 0)])
    p.micro(12, [(INV, 4, 2, 0), (INV, 5, P - 1, 0), (INV, 2, 1, 0)])
    p.micro(15, [(MUL, 3, 10, 0), (EQ, 15, 5, 0), (SUB, 1, 3, 0)])  # x * x^-1 == 1
    return p, []


def mix_rng():
    """a MIX_RNG start (a[2] = 0), continuations (a[2] != 0 multiplies the cell before), a
    continuation whose previous cell was written by another row"""
    p = Program()
    _consts(p, 0, [(0x1234, 0xFFFF), (0xFFFF, 0xFFFF), (1, 0)])
    p.micro(3, [(MIX_RNG, 0, 1, 0), (MIX_RNG, 1, 2, 1), (MIX_RNG, 2, 0, 1)])
    p.micro(6, [(MIX_RNG, 1, 1, 7), (MIX_RNG, 0, 0, 0), (MIX_RNG, 1, 0, P - 1)])
    return p, []


def poseidon2_flags():
    """every p2_load flag and group, p2_store with and without do_mont, a second permutation
    that keeps the state and one that keeps only the upper state"""
    p = Program()
    _consts(p, 0, [(i + 1, 0) for i in range(24)])
    a = list(range(24))
    p.p2_load(0, a[0:8])
    p.p2_load(1, a[8:16], keep_state=1)
    p.p2_load(2, a[16:24], keep_state=1, do_mont=1, prep_full=1)
    for k in range(4):
        p.p2_full(k)
    p.p2_partial()
    for k in range(4):
        p.p2_full(k)
    for g in range(3):
        p.p2_store(g, 24 + 8 * g, do_mont=g % 2)
    # keep_upper_state: groups 0 and 1 cleared, group 2 kept; then add into group 1 with keep_state
    p.p2_load(0, a[8:16], keep_upper_state=1)
    p.p2_load(1, a[0:8], keep_state=1, keep_upper_state=1, do_mont=1)
    p.p2_partial()
    for g in range(3):
        p.p2_store(g, 48 + 8 * g, do_mont=1 - g % 2)
    # no flag: everything cleared
    p.p2_load(2, a[0:8])
    p.p2_partial()
    p.p2_store(2, 72)
    p.p2_store(0, 80, do_mont=1)
    return p, []


def bit_macros():
    p = Program()
    p.macro("wom_init")
    _consts(p, 1, [(0xF0F0, 0x00FF), (0x3C3C, 0x0F0F), (P - 1, 0), (0x7FFFFFF, 0), (0xFFFF, 0xFFFF), (0, 0)])
    p.macro("bit_and_elem", 7, (1, 2, 0))
    p.macro("bit_and_elem", 8, (3, 4, 0))
    p.macro("bit_op_shorts", 9, (1, 2, 1))   # and
    p.macro("bit_op_shorts", 10, (1, 2, 0))  # xor
    p.macro("bit_op_shorts", 11, (5, 1, 0))
    p.macro("bit_op_shorts", 12, (5, 6, 5))
    p.macro("nop")
    p.macro("set_global", 0, (1, 2, 0))
    p.macro("wom_fini", 13)
    return p, []


def rewrite_same_value():
    """a WOM cell rewritten with the same value is legal; a zero cell may be written over"""
    p = Program()
    p.micro(0, [(CONST, 9, 8, 0), (CONST, 0, 0, 0), (CONST, 1, 0, 0)])
    p.micro(0, [(CONST, 9, 8, 0), (CONST, 4, 0, 0), (CONST, 1, 0, 0)])
    return p, []


def outputs():
    p = Program()
    _consts(p, 0, [(10, 1), (20, 2), (30, 3)])
    p.micro(3, [(ADD, 0, 1, 1), (ADD, 1, 2, 0), (ADD, 2, 0, P - 1)])
    p.micro(6, [(SUB, 0, 1, 1), (ADD, 5, 5, 2), (CONST, 0, 0, 0)])
    return p, []


def two_selectors():
    """rows with two selectors set take the first in Preflight::step's order (macro, micro,
    checked_bytes, p2_load, p2_full, p2_partial, p2_store): a p2_full row that is also a p2_store
    row stores nothing, a macro row that is also a micro row runs no micro op"""
    p = Program()
    p.micro(0, [(CONST, 1, 2, 0)])
    p.p2_full(0)[RP.SEL["p2_store"]] = 1
    p.p2_partial()[RP.SEL["p2_store"]] = 1
    r = p.micro(3, [(CONST, 4, 5, 0)])
    r[RP.SEL["macro"]] = 1
    p.p2_load(0, [0] * 8)[RP.SEL["p2_store"]] = 1
    p.p2_store(0, 6)
    return p, []


def _sha(subtype):
    import recursion_sha_program as S
    b = S.ShaBuilder(np.random.default_rng(40 + subtype))
    out = b.block_sha(subtype)
    for i in range(0, 8, 2):  # the digest is read back: a wrong word would break the memory argument
        b.micro([(ADD, out + i, out + i + 1, 0), (SUB, out + i, out + i + 1, 0)])
    out2 = b.block_sha(1 - subtype)
    b.micro([(MUL, out2, out2 + 7, 0)])
    return b.finish()


def sha_shorts():
    """two SHA-256 compressions: block words as two shorts each (subtype 1), then as Montgomery
    words (subtype 0)"""
    return _sha(1)


def sha_montgomery():
    return _sha(0)


CASES = dict(one_row=one_row, full_po2_11=full_po2_11, iop_headers=iop_headers, iop_raw_words=iop_raw_words,
             select_corners=select_corners, extract_corners=extract_corners, inv_modes=inv_modes, mix_rng=mix_rng,
             poseidon2_flags=poseidon2_flags, bit_macros=bit_macros, rewrite_same_value=rewrite_same_value,
             outputs=outputs, two_selectors=two_selectors, sha_shorts=sha_shorts, sha_montgomery=sha_montgomery)


# ---- programs whose run must fail ----
def _pad(p, rows):
    """`rows` harmless rows first, so that the failing cycle is not 0"""
    for r in range(rows):
        p.macro("nop")
    return p


def err_eq():
    p = _pad(Program(), 3)
    p.micro(0, [(CONST, 1, 2, 0), (CONST, 1, 3, 0), (EQ, 0, 0, 0)])
    p.micro(3, [(CONST, 0, 0, 0), (EQ, 0, 1, 0), (CONST, 0, 0, 0)])
    return p, [], 11, r"Equality check failed: Expecting \[1, 2, 0, 0\] == \[1, 3, 0, 0\] \(cycle 4\)$"


def err_overwrite():
    p = _pad(Program(), 2)
    p.micro(0, [(CONST, 1, 0, 0)])
    p.micro(0, [(CONST, 2, 0, 0)])
    return p, [], 11, r"WOM 0 overwritten with \[2, 0, 0, 0\] from \[1, 0, 0, 0\] \(cycle 3\)$"


def err_input_exhausted():
    p = _pad(Program(), 1)
    p.micro(0, [(READ_IOP_HEADER, 2, 2 * 4, 0)])
    return p, [1, 2, 3, 4, 5, 6, 7], 11, r"input exhausted: READ_IOP_HEADER reads 8 words, 7 left \(cycle 1\)$"


def err_input_exhausted_shorts():
    p = Program()
    p.micro(0, [(READ_IOP_HEADER, 1, 2 * 2, 0)])
    p.micro(3, [(READ_IOP_BODY, 0, 0, 0)])
    p.micro(6, [(READ_IOP_HEADER, P - 1, 2 * 2 + 1, 0)])
    return p, [9], 11, r"input exhausted: READ_IOP_HEADER reads 2013265920 words, 0 left \(cycle 2\)$"


def err_empty_body():
    p = _pad(Program(), 5)
    p.micro(0, [(READ_IOP_HEADER, 1, 2 * 1, 0), (READ_IOP_BODY, 0, 0, 0), (READ_IOP_BODY, 0, 0, 0)])
    return p, [4], 11, r"READ_IOP_BODY on an empty IOP body \(cycle 5\)$"


def err_unread_body():
    p = Program()
    p.micro(0, [(READ_IOP_HEADER, 2, 2 * 1, 0), (READ_IOP_BODY, 0, 0, 0), (READ_IOP_HEADER, 1, 2 * 1, 0)])
    return p, [4, 5, 6], 11, r"READ_IOP_HEADER while the IOP body has 1 unread values \(cycle 0\)$"


def err_illegal_row():
    p = _pad(Program(), 6)
    p.rows.append([0] * RP.CTRL)
    return p, [], 11, r"Illegal recursion op \(cycle 6\)$"


def err_selector_two():
    """a selector that is not exactly one selects nothing"""
    p = _pad(Program(), 1)
    p.micro(0, [(CONST, 1, 0, 0)])[RP.SEL["micro"]] = 2
    return p, [], 11, r"Illegal recursion op \(cycle 1\)$"


def err_unknown_opcode():
    p = _pad(Program(), 2)
    p.micro(0, [(CONST, 1, 0, 0), (11, 0, 0, 0)])
    return p, [], 11, r"Unknown opcode \(cycle 2\)$"


def err_read_past_memory():
    p = _pad(Program(), 1)
    p.micro(0, [(ADD, 0, 1, 0)])
    return p, [], 11, r"WOM read of address 0 past the memory's 0 cells \(cycle 1\)$"


def err_cap_write():
    p = _pad(Program(), 1)
    p.micro(16 << 11, [(CONST, 1, 0, 0)])
    return p, [], 11, r"WOM address 32768 at or above the library's cap of 16 \* 2\^po2 = 32768 cells \(cycle 1\)$"


def err_cap_write_below_is_fine_at_po2_12():
    """the same write is legal one size up, and the cap moves with po2"""
    p = _pad(Program(), 1)
    p.micro(16 << 11, [(CONST, 1, 0, 0)])
    p.micro((16 << 12) - 2, [(CONST, 1, 0, 0)])
    return p, [], 12, r"WOM address 65536 at or above the library's cap of 16 \* 2\^po2 = 65536 cells \(cycle 2\)$"


def err_cap_read():
    p = Program()
    p.micro(0, [(CONST, 1, 0, 0), (CONST, P - 1, 0, 0), (SELECT, 1, 0, 1)])  # reads cell p - 1
    return p, [], 11, r"WOM address 2013265920 at or above the library's cap .* \(cycle 0\)$"


def err_cap_p2_store():
    p = Program()
    p.p2_store(0, (16 << 11) - 3)
    return p, [], 11, r"WOM address 32768 at or above the library's cap .* \(cycle 0\)$"


def err_p2_group():
    p = Program()
    p.micro(0, [(CONST, 1, 0, 0)])
    r = p.p2_load(1, [0] * 8)
    r[14] = 1  # g1 + 2 * g2 = 3
    return p, [], 11, r"Poseidon2 load: group out of range \(cycle 1\)$"


def err_sha_fini_address():
    p = _pad(Program(), 2)
    p.macro("sha_fini", 0, (2, 6, 0))
    return p, [], 11, r"sha_fini: the output address args\[0\] - 3 is below zero \(cycle 2\)$"


ERRORS = dict(eq=err_eq, overwrite=err_overwrite, input_exhausted=err_input_exhausted,
              input_exhausted_shorts=err_input_exhausted_shorts, empty_body=err_empty_body,
              unread_body=err_unread_body, illegal_row=err_illegal_row, selector_two=err_selector_two,
              unknown_opcode=err_unknown_opcode, read_past_memory=err_read_past_memory, cap_write=err_cap_write,
              cap_po2_12=err_cap_write_below_is_fine_at_po2_12, cap_read=err_cap_read, cap_p2_store=err_cap_p2_store,
              p2_group=err_p2_group, sha_fini_address=err_sha_fini_address)


# ---- programs the decoder refuses (no run) ----
def refused_checked_bytes():
    p = _pad(Program(), 4)
    p._row("checked_bytes")
    return p, r"row 4 is a checked_bytes row"


def write_cases(path):
    """every CASES and ERRORS program for the stand-alone native check"""
    with open(path, "w") as fh:
        items = [(n, *f(), 11) for n, f in CASES.items()]
        items += [("err_" + n, *f()[:3]) for n, f in ERRORS.items()]
        for name, prog, inp, po2 in items:
            code = prog.encoded()
            fh.write(f"{name} {po2} {code.size} {len(inp)}\n")
            fh.write(" ".join(str(int(x)) for x in code) + " " + " ".join(str(int(x)) for x in inp) + "\n")
