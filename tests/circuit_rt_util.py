"""Shared by the run-time circuit tests (test_circuit_rt_host.py, test_circuit_rt_gpu.py): the
committed circuits registered under another name, once per process, and a variant of the demo
circuit that no build has."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCUITS = os.path.join(ROOT, "risc0_amd", "circuits")
P = 15 * 2**27 + 1


def tables(name):
    """circuit_tables.load() of a committed circuit"""
    from risc0_amd import circuit_tables
    return circuit_tables.load(os.path.join(CIRCUITS, name + ".taps.json"), os.path.join(CIRCUITS, name + ".poly.ir"))


def registered(name):
    """"rt_<name>": the committed <name> files registered at run time (the registry has no way
    out, so a process registers each once)"""
    from risc0_amd import hal
    rt = "rt_" + name
    if rt not in hal.circuit_names():
        hal.register_circuit(rt, CIRCUITS, files=name)
    return rt


def register_tables(t, name):
    """r0hip_circuit_register on a tables dict; raises R0HipError with the library's message"""
    from risc0_amd import hal
    import ctypes as C
    s, keep = hal.circuit_tables_struct(t, name)
    hal.check(hal.lib().r0hip_circuit_register(C.byref(s), C.sizeof(s)))


# ---- a circuit that is compiled in nowhere: the demo AIR with the step (a, b) -> (b, a + 2b) ----

VARIANT = "demo_2b"


def write_variant(directory):
    """<directory>/demo_2b.poly.ir and .taps.json, from tools/gen_demo_circuit.py's builder with
    one constraint changed: b = a[-1] + 2 * b[-1]"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_demo_circuit as G
    sub = lambda x, y: lambda b: b.node("-", x(b), y(b))
    add = lambda x, y: lambda b: b.node("+", x(b), y(b))
    mul = lambda x, y: lambda b: b.node("*", x(b), y(b))
    t = lambda arg, col, back=0: lambda b: b.tap(arg, col, back)
    g = lambda arg, i: lambda b: b.node("g", arg, i)
    first, on, last = t(G.CODE, G.FIRST), t(G.CODE, G.ON), t(G.CODE, G.LAST)
    a, bb, s = t(G.DATA, G.A), t(G.DATA, G.B), t(G.DATA, G.S)
    a1, b1 = t(G.DATA, G.A, 1), t(G.DATA, G.B, 1)
    z = [t(G.ACCUM, k) for k in range(4)]
    z1 = [t(G.ACCUM, k, 1) for k in range(4)]
    ma = [mul(g(G.MIX, k), a) for k in range(4)]
    items = [
        ("eqz", mul(on, sub(s, mul(a, bb)))),
        ("cond", first, [("eqz", sub(a, g(G.GLOBAL, 0))), ("eqz", sub(bb, g(G.GLOBAL, 1)))] +
         [("eqz", sub(z[k], ma[k])) for k in range(4)]),
        ("cond", sub(on, first), [("eqz", sub(a, b1)), ("eqz", sub(bb, add(a1, add(b1, b1))))] +
         [("eqz", sub(z[k], add(z1[k], ma[k]))) for k in range(4)]),
        ("eqz", mul(last, sub(bb, g(G.GLOBAL, 2)))),
    ]
    probe = G.Builder()
    probe.chain(items)
    powers = sorted(probe.seen)
    b = G.Builder(powers)
    res, _ = b.chain(items)
    with open(os.path.join(CIRCUITS, "demo.taps.json")) as f:
        d = json.load(f)
    d["name"] = VARIANT
    d["circuit_info"] = "R0HIPDEMO:2b__v1"
    d["poly_mix_powers"] = powers
    with open(os.path.join(directory, VARIANT + ".taps.json"), "w") as f:
        json.dump(d, f)
    with open(os.path.join(directory, VARIANT + ".poly.ir"), "w") as f:
        f.write("\n".join(b.lines + [f"r {res}"]) + "\n")


def variant_witness(po2, n, a0=3, b0=5):
    """(code, data, global) of the variant as plain values, column-major: demo_air.witness with the
    variant's step; rows from n on are zero"""
    rows = 1 << po2
    code = [[0] * rows for _ in range(3)]
    data = [[0] * rows for _ in range(3)]
    a, b = a0 % P, b0 % P
    for i in range(n):
        code[0][i], code[1][i], code[2][i] = int(i == 0), 1, int(i == n - 1)
        data[0][i], data[1][i], data[2][i] = a, b, a * b % P
        a, b = b, (a + 2 * b) % P
    glob = [data[0][0], data[1][0], data[1][n - 1]]
    flat = lambda cols: [v for c in cols for v in c]
    return flat(code), flat(data), glob
