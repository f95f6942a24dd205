"""A plain-Python ChaCha20 (RFC 8439 section 2.3) and the field elements r0hip_fill_chacha20
makes of its keystream: element i is the 128-bit little-endian integer of keystream words
4i..4i+3 (block counter from 0) reduced mod p = 15 * 2^27 + 1. The model of the device kernel
for tests/test_worker_host.py and tests/test_worker_gpu.py; numpy only vectorises it over
blocks."""
import numpy as np

P = 15 * (1 << 27) + 1
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)

#: RFC 8439 section 2.3.2: key bytes 00..1f, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
RFC_KEY = np.frombuffer(bytes(range(32)), dtype="<u4").copy()
RFC_NONCE = np.array([0x09000000, 0x4A000000, 0], dtype=np.uint32)


def _rotl(v, c):
    return ((v << c) & 0xFFFFFFFF) | (v >> (32 - c))


def block(key, counter, nonce):
    """one 64-byte block as its 16 little-endian state words (Python ints; RFC 8439 2.3.1)"""
    init = list(SIGMA) + [int(k) for k in key] + [int(counter) & 0xFFFFFFFF] + [int(w) for w in nonce]
    assert len(init) == 16
    x = list(init)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return [(a + b) & 0xFFFFFFFF for a, b in zip(x, init)]


def block_elements(words):
    """the four field elements of one block's 16 words"""
    return [sum(int(words[4 * j + k]) << (32 * k) for k in range(4)) % P for j in range(4)]


def blocks(key, nonce, first, count):
    """keystream blocks first .. first + count - 1 as a (count, 16) uint32 array (the block
    function above, on arrays of blocks)"""
    ctr = np.arange(first, first + count, dtype=np.uint64).astype(np.uint32)
    init = [np.full(count, v, np.uint32) for v in SIGMA] + [np.full(count, int(k), np.uint32) for k in key] + [ctr] + \
        [np.full(count, int(w), np.uint32) for w in nonce]
    x = [v.copy() for v in init]

    def rotl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        x[a] = x[a] + x[b]
        x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = x[c] + x[d]
        x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = x[a] + x[b]
        x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = x[c] + x[d]
        x[b] = rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
            qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(x, init)], axis=1)


def elements(key, nonce, count):
    """elements 0 .. count - 1 of the stream (uint32, each below P)"""
    nb = (count + 3) // 4
    if nb == 0:
        return np.zeros(0, np.uint32)
    w = blocks(key, nonce, 0, nb).reshape(nb * 4, 4).astype(np.uint64)
    v = w[:, 3] % P
    for k in (2, 1, 0):
        v = ((v << np.uint64(32)) | w[:, k]) % np.uint64(P)
    return v[:count].astype(np.uint32)
