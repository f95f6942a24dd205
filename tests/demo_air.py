"""The demo circuit (risc0_amd/circuits/demo.*) written down a second time, straight from its
AIR's formulas and not from the constraint program: test infrastructure for the plug-in tests.

Values are plain integers mod P (numpy uint64 arrays or Python ints); an FpExt is a 4-tuple of
them. enc/dec convert to and from the library's Montgomery words.

Columns: code first, on, last; data a, b, s; accum z0..z3; global g0..g2; mix m0..m3.
  C0          on * (s - a * b)
  first  *  { a - g0, b - g1, z_k - m_k a }
  (on - first) * { a - b', b - (a' + b'), z_k - (z_k' + m_k a) }      (x' = the row before)
  last * (b - g2)
poly = C0 + x * first * sum_j F_j x^j + x^7 * (on - first) * sum_j S_j x^j + x^13 * last * (b - g2)
with x the poly_mix (each guarded block's six constraints restart at power 0).
"""
import numpy as np

P = 15 * 2**27 + 1
NB = P - 11
R = 2**32 % P
RINV = pow(R, P - 2, P)
N_TAPS = 16
# tap order of demo.taps.json: accum z_k (back 0, 1) x 4, code first/on/last, data a (0, 1), b (0, 1), s
TAP_Z, TAP_Z1 = [0, 2, 4, 6], [1, 3, 5, 7]
TAP_FIRST, TAP_ON, TAP_LAST, TAP_A, TAP_A1, TAP_B, TAP_B1, TAP_S = 8, 9, 10, 11, 12, 13, 14, 15
POWERS = [0, 1, 2, 3, 4, 5, 7, 13]  # the distinct poly_mix powers (demo.taps.json)


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % P * R % P).astype(np.uint32)


def dec(w):
    return (np.asarray(w, dtype=np.uint64) * RINV % P).astype(np.uint64)


def ext(v):
    return v if isinstance(v, tuple) else (v, v * 0, v * 0, v * 0)


def eadd(a, b):
    return tuple((x + y) % P for x, y in zip(ext(a), ext(b)))


def esub(a, b):
    return tuple((x + P - y) % P for x, y in zip(ext(a), ext(b)))


def emul(a, b):
    a0, a1, a2, a3 = ext(a)
    b0, b1, b2, b3 = ext(b)
    m = lambda x, y: (x * y) % P
    return ((m(a0, b0) + NB * ((m(a1, b3) + m(a2, b2) + m(a3, b1)) % P)) % P,
            (m(a0, b1) + m(a1, b0) + NB * ((m(a2, b3) + m(a3, b2)) % P)) % P,
            (m(a0, b2) + m(a1, b1) + m(a2, b0) + NB * m(a3, b3)) % P,
            (m(a0, b3) + m(a1, b2) + m(a2, b1) + m(a3, b0)) % P)


def epow(x, n):
    r = (1, 0, 0, 0)
    for _ in range(n):
        r = emul(r, x)
    return r


def constraints(t, g, m):
    """The 14 constraint values in chain order from the 16 tap values t (tap order; Fp or FpExt),
    the globals g[3] and the mix m[4] (Fp), each with its selector applied."""
    z, z1 = [t[i] for i in TAP_Z], [t[i] for i in TAP_Z1]
    first, on, last = t[TAP_FIRST], t[TAP_ON], t[TAP_LAST]
    a, a1, b, b1, s = t[TAP_A], t[TAP_A1], t[TAP_B], t[TAP_B1], t[TAP_S]
    ma = [emul(a, m[k]) for k in range(4)]
    head = [esub(a, g[0]), esub(b, g[1])] + [esub(z[k], ma[k]) for k in range(4)]
    step = [esub(a, b1), esub(b, eadd(a1, b1))] + [esub(z[k], eadd(z1[k], ma[k])) for k in range(4)]
    rest = esub(on, first)
    return ([emul(on, esub(s, emul(a, b)))] + [emul(first, c) for c in head] + [emul(rest, c) for c in step] +
            [emul(last, esub(b, g[2]))])


def poly(t, g, m, x):
    """The constraint polynomial: sum of constraint j times x^power_j."""
    powers = [0] + [1 + j for j in range(6)] + [7 + j for j in range(6)] + [13]
    tot = (0, 0, 0, 0)
    for c, p in zip(constraints(t, g, m), powers):
        tot = eadd(tot, emul(c, epow(x, p)))
    return tot


def taps_on_rows(code, data, accum, rows, step=1):
    """The 16 tap values of every row of column-major groups (plain), a tap `back` rows * step up."""
    cyc = np.arange(rows)
    at = lambda grp, col, back: grp[col * rows + ((cyc - back * step) % rows)]
    t = []
    for k in range(4):
        t += [at(accum, k, 0), at(accum, k, 1)]
    t += [at(code, 0, 0), at(code, 1, 0), at(code, 2, 0)]
    t += [at(data, 0, 0), at(data, 0, 1), at(data, 1, 0), at(data, 1, 1), at(data, 2, 0)]
    return t


def witness(po2, n, a0=1, b0=1, noise=None):
    """code, data, global (plain, column-major) of n active rows; rows above n: `noise` (a
    generator) or zero in data."""
    rows = 1 << po2
    code = np.zeros(3 * rows, np.uint64)
    data = np.zeros(3 * rows, np.uint64) if noise is None else noise.integers(0, P, 3 * rows).astype(np.uint64)
    a, b = a0 % P, b0 % P
    for i in range(n):
        data[i], data[rows + i], data[2 * rows + i] = a, b, a * b % P
        a, b = b, (a + b) % P
    code[0] = 1
    code[rows:rows + n] = 1
    code[2 * rows + n - 1] = 1
    glob = np.array([data[0], data[rows], data[rows + n - 1]], np.uint64)
    return code, data, glob


def accumulate(po2, n, data, mix, fill=0):
    """accum (plain, column-major): z_i = sum_{j <= i} m * a_j on the rows below n, `fill` above."""
    rows = 1 << po2
    acc = np.full(4 * rows, fill, np.uint64)
    run = np.cumsum(data[:n].astype(object)) % P
    for k in range(4):
        acc[k * rows:k * rows + n] = (run * int(mix[k]) % P).astype(np.uint64)
    return acc
