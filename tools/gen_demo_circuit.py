#!/usr/bin/env python3
"""Write the demo circuit: risc0_amd/circuits/demo.poly.ir and demo.taps.json.

A small AIR of this project's own design (nothing in it comes from another code base): the
library can make a valid witness for it (risc0_amd/csrc/demo_circuit.hip), prove it and verify the
seal in full, so it serves r0hip_selftest and is the in-tree example of a plugged-in circuit.

Columns (a row is a cycle; x[-1] is the row before):
  code   first, on, last     selectors; `on` is 1 on the n active rows and 0 on every other row
                             (padding and ZK noise), `first` on row 0, `last` on row n - 1
  data   a, b, s             a Fibonacci-like pair and its product
  accum  z0..z3              one FpExt: the running sum of m * a, m = the four mix words
  global g0, g1, g2          a[0], b[0] and b[n - 1]

Constraints, in chain order (poly_mix power in brackets; a guarded block's inner chain starts
again at power 0):
  [0]    on * (s - a * b)                                    degree 3
  [1..6] first * { a - g0, b - g1, z_k - m_k * a  (k = 0..3) }
  [7..12] (on - first) * { a - b[-1], b - (a[-1] + b[-1]), z_k - (z_k[-1] + m_k * a) }
  [13]   last * (b - g2)
Every constraint carries a selector that is 0 where `on` is 0, so the rows outside the active
range may hold anything, and row 0 never reads row N - 1.

Usage: gen_demo_circuit.py [OUTDIR]      (default risc0_amd/circuits)
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAME = "demo"
INFO = "R0HIPDEMO:rev1v1"  # 16 bytes
EVAL_ARGS = ["code", "global", "data", "mix", "accum"]
CODE, GLOBAL, DATA, MIX, ACCUM = range(5)
FIRST, ON, LAST = range(3)
A, B, S = range(3)


class Builder:
    def __init__(self, powers=None):
        self.lines, self.memo = [], {}
        self.powers = powers  # None: collect into self.seen
        self.seen = set()

    def node(self, *n):
        if n not in self.memo:
            self.memo[n] = len(self.lines)
            self.lines.append(" ".join(str(x) for x in (n[0], len(self.lines)) + n[1:]))
        return self.memo[n]

    def tap(self, arg, col, back=0):
        return self.node("l", arg, col, back)

    def k(self, power):
        self.seen.add(power)
        return self.powers.index(power) if self.powers else 0

    def chain(self, items):
        """items: ("eqz", value) | ("cond", condition, items). Returns (id, powers consumed)."""
        acc, p = self.node("e", 0, 0, 0, 0), 0
        for it in items:
            if it[0] == "eqz":
                acc = self.node("a", acc, it[1](self), self.k(p))
                p += 1
            else:
                inner, n = self.chain(it[2])
                acc = self.node("b", acc, it[1](self), inner, self.k(p))
                p += n
        return acc, p


def constraints():
    sub = lambda x, y: lambda b: b.node("-", x(b), y(b))
    add = lambda x, y: lambda b: b.node("+", x(b), y(b))
    mul = lambda x, y: lambda b: b.node("*", x(b), y(b))
    t = lambda arg, col, back=0: lambda b: b.tap(arg, col, back)
    g = lambda arg, i: lambda b: b.node("g", arg, i)
    first, on, last = t(CODE, FIRST), t(CODE, ON), t(CODE, LAST)
    a, bb, s = t(DATA, A), t(DATA, B), t(DATA, S)
    a1, b1 = t(DATA, A, 1), t(DATA, B, 1)
    z = [t(ACCUM, k) for k in range(4)]
    z1 = [t(ACCUM, k, 1) for k in range(4)]
    ma = [mul(g(MIX, k), a) for k in range(4)]
    return [
        ("eqz", mul(on, sub(s, mul(a, bb)))),
        ("cond", first, [("eqz", sub(a, g(GLOBAL, 0))), ("eqz", sub(bb, g(GLOBAL, 1)))] +
         [("eqz", sub(z[k], ma[k])) for k in range(4)]),
        ("cond", sub(on, first), [("eqz", sub(a, b1)), ("eqz", sub(bb, add(a1, b1)))] +
         [("eqz", sub(z[k], add(z1[k], ma[k]))) for k in range(4)]),
        ("eqz", mul(last, sub(bb, g(GLOBAL, 2)))),
    ]


def program():
    probe = Builder()
    probe.chain(constraints())
    powers = sorted(probe.seen)
    b = Builder(powers)
    res, _ = b.chain(constraints())
    return b.lines + [f"r {res}"], powers


def taps():
    # [offset, back, group, combo, skip], sorted by group, offset, back; combo 0 = {0}, 1 = {0, 1}
    out = []
    for k in range(4):  # accum z0..z3
        out += [[k, 0, 0, 1, 2], [k, 1, 0, 1, 2]]
    for k in range(3):  # code first, on, last
        out.append([k, 0, 1, 0, 1])
    for k in (A, B):
        out += [[k, 0, 2, 1, 2], [k, 1, 2, 1, 2]]
    out.append([S, 0, 2, 0, 1])
    return out


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "risc0_amd", "circuits")
    lines, powers = program()
    tp = taps()
    d = {
        "taps": tp,
        "combo_taps": [0, 0, 1],
        "combo_begin": [0, 1, 3],
        "group_begin": [0, 8, 11, 16],
        "combos_count": 2,
        "reg_count": 10,
        "tot_combo_backs": 3,
        "group_names": ["accum", "code", "data"],
        "name": NAME,
        "circuit_info": INFO,
        "output_size": 3,
        "mix_size": 4,
        "poly_mix_powers": powers,
        "group_sizes": [4, 3, 3],
        "eval_args": EVAL_ARGS,
    }
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, NAME + ".taps.json"), "w") as f:
        json.dump(d, f, separators=(",", ":"))
        f.write("\n")
    with open(os.path.join(outdir, NAME + ".poly.ir"), "w") as f:
        f.write(f"# {NAME} constraint program (written by tools/gen_demo_circuit.py)\n")
        f.write("\n".join(lines) + "\n")
    print(f"{NAME}: {len(lines)} records, {len(tp)} taps, poly_mix powers {powers}")


if __name__ == "__main__":
    main()
