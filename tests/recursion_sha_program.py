"""The recursion circuit's SHA macro ops, restated (test infrastructure only): Preflight's
sha_init, sha_load, sha_mix and sha_fini (prove/preflight.rs:411-500) on top of
recursion_program.Preflight, and the row sequence one SHA-256 compression takes in a program:

    sha_init x 4    operands (address of H[3 - i], address of H[7 - i]): the initial state, read
                    from the write-once memory as two shorts per word
    sha_load x 16   operands (address of the block word, address of K[i], subtype): subtype 0
                    takes the cell's first element as its Montgomery word, any other subtype the
                    cell's two shorts
    sha_mix x 48    operands (0, address of K[16 + i])
    sha_fini x 4    operands (out + 3 - i, out + 7 - i): the digest's eight words, two shorts each,
                    written at out .. out + 7

Words travel as the digest holds them (the bytes of a big-endian word read as a little-endian
u32), which is how Preflight swaps them around sha2::compress256.
"""
import struct

import recursion_program as RP

H0 = [0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19]
K = [0x428A2F98, 0x71374491, 0xB5C0FBCF, 0xE9B5DBA5, 0x3956C25B, 0x59F111F1, 0x923F82A4, 0xAB1C5ED5, 0xD807AA98,
     0x12835B01, 0x243185BE, 0x550C7DC3, 0x72BE5D74, 0x80DEB1FE, 0x9BDC06A7, 0xC19BF174, 0xE49B69C1, 0xEFBE4786,
     0x0FC19DC6, 0x240CA1CC, 0x2DE92C6F, 0x4A7484AA, 0x5CB0A9DC, 0x76F988DA, 0x983E5152, 0xA831C66D, 0xB00327C8,
     0xBF597FC7, 0xC6E00BF3, 0xD5A79147, 0x06CA6351, 0x14292967, 0x27B70A85, 0x2E1B2138, 0x4D2C6DFC, 0x53380D13,
     0x650A7354, 0x766A0ABB, 0x81C2C92E, 0x92722C85, 0xA2BFE8A1, 0xA81A664B, 0xC24B8B70, 0xC76C51A3, 0xD192E819,
     0xD6990624, 0xF40E3585, 0x106AA070, 0x19A4C116, 0x1E376C08, 0x2748774C, 0x34B0BCB5, 0x391C0CB3, 0x4ED8AA4A,
     0x5B9CCA4F, 0x682E6FF3, 0x748F82EE, 0x78A5636F, 0x84C87814, 0x8CC70208, 0x90BEFFFA, 0xA4506CEB, 0xBEF9A3F7,
     0xC67178F2]
M32 = 0xFFFFFFFF


def bswap(x):
    return struct.unpack("<I", struct.pack(">I", x & M32))[0]


def compress(state, block):
    """SHA-256's compression function on numeric words (FIPS 180-4 6.2.2)"""
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    w = list(block)
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = state
    for t in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & M32 & g)) + K[t] + w[t]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        a, b, c, d, e, f, g, h = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
    return [(x + y) & M32 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


class ShaPreflight(RP.Preflight):
    """recursion_program.Preflight with the SHA macro ops"""

    def __init__(self, inp=()):
        super().__init__(inp)
        self.sha_state, self.sha_words = [0] * 8, [0] * 16
        self.init_pos = self.load_pos = self.fini_pos = 0

    def step(self, row):
        g = lambda i: row[i] % RP.P
        if g(RP.SEL["macro"]) == 1 and not (g(RP.MACRO["bit_and_elem"]) == 1 or g(RP.MACRO["bit_op_shorts"]) == 1):
            a = [g(RP.MACRO_OPERAND + i) for i in range(3)]
            sha = True
            if g(RP.MACRO["sha_init"]) == 1:
                if self.init_pos == 0:
                    self.sha_state = list(H0)
                self.init_pos = (self.init_pos + 1) % 4
            elif g(RP.MACRO["sha_load"]) == 1:
                x = self.wom_read(a[0])
                self.sha_words[self.load_pos] = RP.enc(x[0]) if a[2] == 0 else (x[0] + (x[1] << 16)) & M32
                self.load_pos = (self.load_pos + 1) % 16
            elif g(RP.MACRO["sha_mix"]) == 1:
                pass
            elif g(RP.MACRO["sha_fini"]) == 1:
                if self.fini_pos == 0:
                    self.sha_state = compress(self.sha_state, [bswap(w) for w in self.sha_words])
                    for i in range(8):
                        out = bswap(self.sha_state[i])
                        self.wom_write(a[0] - 3 + i, (out & 0xFFFF, out >> 16, 0, 0))
                self.fini_pos = (self.fini_pos + 1) % 4
            else:
                sha = False
            if sha:
                self.cycles.append((self.iop_idx, 0))
                self.iop_idx = len(self.iops)
                return
        super().step(row)


def preflight(program, inp=()):
    pf = ShaPreflight(inp)
    for row in program.rows:
        pf.step(row)
    return pf


def shorts(x):
    return (x & 0xFFFF, x >> 16)


class ShaBuilder(RP.Builder):
    """recursion_program.Builder with the constants of SHA-256 in the write-once memory (after
    wom_init) and a block for one compression"""

    def __init__(self, rng, const_form=lambda x: x):
        super().__init__(rng)
        self.h = self.consts([shorts(const_form(x)) for x in H0])
        self.k = self.consts([shorts(const_form(x)) for x in K])

    def block_sha(self, subtype=1):
        """one compression of 16 random words; returns the address of the digest's first word"""
        if subtype:
            ins = self.shorts(16)
        else:
            ins = self.elems(16)
        for i in range(4):
            self.p.macro("sha_init", 0, (self.h[3 - i], self.h[7 - i], 0))
        for i in range(16):
            self.p.macro("sha_load", 0, (ins[i], self.k[i], subtype))
        for i in range(48):
            self.p.macro("sha_mix", 0, (0, self.k[16 + i], 0))
        out = self.next
        for i in range(4):
            self.p.macro("sha_fini", 0, (out + 3 - i, out + 7 - i, 0))
        self.next += 8
        return out
