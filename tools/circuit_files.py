#!/usr/bin/env python3
"""The list of circuits compiled into libr0hip.so, and where each one's files are.

The list is the two shipped circuits, then the demo circuit (tools/gen_demo_circuit.py), then
every circuit found in the directories named by EXTRA_CIRCUIT_DIRS (space-separated; the make
variable of the same name is handed on through the environment). A directory holds
<name>.poly.ir (tools/gen_poly_ir.py) and <name>.taps.json (tools/extract_circuits.py), and may
hold <name>.ectune.json; without it tools/gen_eval_check.py uses its untuned defaults.

Every plugged-in circuit, and the demo circuit, is validated here before anything is generated
from it (validate); a refusal names the file and the field. The shipped rv32im and recursion
files are trusted as they are.

  circuit_files.py --names          the names, space-separated (the Makefile's CIRCUITS)
  circuit_files.py --check          validate, print one line per circuit
"""
import glob
import json
import os
import re
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
BUILTIN_DIR = os.path.join(ROOT, "risc0_amd", "circuits")
SHIPPED = ["rv32im", "recursion"]
DEMO = "demo"
# directories under risc0_amd/csrc/gen that other generators own, and words the build uses
RESERVED = {"accum", "rvaccum", "rwitgen", "rvwitgen", "circuits"}
GROUPS = {"accum": 0, "code": 1, "data": 2}


class CircuitError(Exception):
    pass


def extra_dirs():
    return os.environ.get("EXTRA_CIRCUIT_DIRS", "").split()


def circuits(validated=True):
    """[(name, directory)] in build order. Plugged-in circuits are validated unless told not to."""
    out = [(n, BUILTIN_DIR) for n in SHIPPED + [DEMO]]
    where = {n: os.path.join(d, n + ".taps.json") for n, d in out}
    for d in extra_dirs():
        if not os.path.isdir(d):
            raise CircuitError(f"{d}: EXTRA_CIRCUIT_DIRS: not a directory")
        for path in sorted(glob.glob(os.path.join(d, "*.taps.json"))):
            name = os.path.basename(path)[:-len(".taps.json")]
            if not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", name):
                raise CircuitError(f"{path}: name: {name!r} is not a C identifier")
            if name in RESERVED:
                raise CircuitError(f"{path}: name: {name!r} is reserved by the build")
            if name in where:
                raise CircuitError(f"{path}: name: {name!r} collides with the circuit of {where[name]}")
            where[name] = path
            out.append((name, d))
    if validated:
        for name, d in out:
            if name not in SHIPPED:
                validate(name, d)
    return out


def find(name, suffix, must=True):
    """Path of <name>.<suffix> in the circuit's directory (None if absent and not `must`)."""
    for n, d in circuits(validated=False):
        if n == name:
            path = os.path.join(d, f"{name}.{suffix}")
            if os.path.exists(path):
                return path
            if must:
                raise CircuitError(f"{path}: missing")
            return None
    raise CircuitError(f"unknown circuit {name!r}; known: {' '.join(n for n, _ in circuits(validated=False))}")


def read_ir(path):
    """[(line number, op, [ints])] of a constraint program."""
    recs = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            if line.startswith("#") or not line.strip():
                continue
            t = line.split()
            try:
                recs.append((ln, t[0], [int(x) for x in t[1:]]))
            except ValueError:
                raise CircuitError(f"{path}: line {ln}: not a record: {line.strip()!r}")
    return recs


def validate(name, d):
    """Refuse a circuit whose taps.json is inconsistent or whose program reads what it lacks."""
    tpath = os.path.join(d, name + ".taps.json")
    ipath = os.path.join(d, name + ".poly.ir")
    if not os.path.exists(ipath):
        raise CircuitError(f"{ipath}: missing (a circuit is <name>.poly.ir and <name>.taps.json)")
    try:
        with open(tpath) as f:
            t = json.load(f)
    except ValueError as e:
        raise CircuitError(f"{tpath}: not JSON: {e}")

    def bad(field, why):
        raise CircuitError(f"{tpath}: {field}: {why}")

    for k in ("taps", "combo_taps", "combo_begin", "group_begin", "combos_count", "group_names", "name",
              "circuit_info", "output_size", "mix_size", "poly_mix_powers", "group_sizes", "eval_args"):
        if k not in t:
            bad(k, "missing")
    if t["name"] != name:
        bad("name", f"{t['name']!r} is not the file's name {name!r}")
    if t["group_names"] != ["accum", "code", "data"]:
        bad("group_names", 'must be ["accum", "code", "data"]')
    taps = t["taps"]
    if not taps or any(not isinstance(x, list) or len(x) != 5 for x in taps):
        bad("taps", "every tap is [offset, back, group, combo, skip]")
    keys = [(x[2], x[0], x[1]) for x in taps]
    for i in range(1, len(keys)):
        if keys[i - 1] >= keys[i]:
            bad("taps", f"entry {i} is not sorted by group, offset and back after entry {i - 1}")
    # skip: the taps of one register are adjacent and carry the register's tap count
    regs, cur = [], 0
    while cur < len(taps):
        sk = taps[cur][4]
        if sk < 1 or cur + sk > len(taps):
            bad("taps", f"entry {cur}: skip {sk} does not tile the registers")
        for j in range(cur, cur + sk):
            if taps[j][4] != sk or keys[j][:2] != keys[cur][:2]:
                bad("taps", f"entry {j}: skip {taps[j][4]} does not tile the registers (register of entry {cur})")
        if cur + sk < len(taps) and keys[cur + sk][:2] == keys[cur][:2]:
            bad("taps", f"entry {cur + sk}: skip {sk} of entry {cur} does not tile the registers")
        regs.append((cur, sk))
        cur += sk
    # combos
    cb, ct = t["combo_begin"], t["combo_taps"]
    if (len(cb) != t["combos_count"] + 1 or cb[0] != 0 or cb[-1] != len(ct)
            or any(cb[i] >= cb[i + 1] for i in range(len(cb) - 1))):
        bad("combo_begin", f"is not {t['combos_count']} + 1 rising offsets into the {len(ct)} combo_taps")
    for cur, sk in regs:
        c = taps[cur][3]
        if any(taps[j][3] != c for j in range(cur, cur + sk)) or not 0 <= c < t["combos_count"]:
            bad("combo_begin", f"register of tap {cur}: combo {c} is not one of {t['combos_count']}")
        if ct[cb[c]:cb[c + 1]] != [taps[j][1] for j in range(cur, cur + sk)]:
            bad("combo_begin", f"combo {c} disagrees with the backs of the register of tap {cur}")
    # groups
    want_gb = [0]
    for g in range(3):
        want_gb.append(sum(1 for x in taps if x[2] <= g))
    if t["group_begin"] != want_gb:
        bad("group_begin", f"{t['group_begin']} disagrees with the taps ({want_gb})")
    sizes = []
    for g in range(3):
        cols = sorted({x[0] for x in taps if x[2] == g})
        if cols != list(range(len(cols))) or not cols:
            bad("group_sizes", f"group {g}: the taps' offsets are not 0..{len(cols) - 1}")
        sizes.append(len(cols))
    if t["group_sizes"] != sizes:
        bad("group_sizes", f"{t['group_sizes']} disagrees with the taps ({sizes})")
    if any(x[2] not in (0, 1, 2) for x in taps):
        bad("taps", "a group is not 0, 1 or 2")
    info = t["circuit_info"]
    if not isinstance(info, str) or len(info.encode()) != 16 or not info.isascii() or '"' in info or "\\" in info:
        bad("circuit_info", f"{info!r} is not 16 plain bytes")
    for k in ("output_size", "mix_size"):
        if not isinstance(t[k], int) or t[k] < 0:
            bad(k, "not a size")
    args = t["eval_args"]
    if any(a not in ("accum", "code", "data", "mix", "global") for a in args):
        bad("eval_args", f"{args}: each is accum, code, data, mix or global")
    pm = t["poly_mix_powers"]
    # the program
    have = set(keys)
    ids = 0
    for ln, op, a in read_ir(ipath):
        def ibad(why):
            raise CircuitError(f"{ipath}: line {ln}: {op} record: {why}")
        n_op = {"c": 2, "e": 5, "l": 4, "g": 3, "+": 3, "-": 3, "*": 3, "a": 4, "b": 5, "r": 1}.get(op)
        if n_op is None or len(a) != n_op:
            ibad("not a record of the constraint program")
        if op == "r":
            if a[0] >= ids:
                ibad(f"names value {a[0]} before it is made")
            continue
        if a[0] != ids:
            ibad(f"id {a[0]} is not the next dense id {ids}")
        ids += 1
        if op == "l":
            if not 0 <= a[1] < len(args) or args[a[1]] not in GROUPS:
                ibad(f"names argument {a[1]}, which {os.path.basename(tpath)} (eval_args) does not have as a group")
            if (GROUPS[args[a[1]]], a[2], a[3]) not in have:
                ibad(f"names tap ({args[a[1]]}, column {a[2]}, back {a[3]}), which {os.path.basename(tpath)} "
                     "(taps) does not have")
        elif op == "g":
            if not 0 <= a[1] < len(args) or args[a[1]] not in ("mix", "global"):
                ibad(f"names argument {a[1]}, which {os.path.basename(tpath)} (eval_args) does not have as "
                     "mix or global")
            lim = t["mix_size"] if args[a[1]] == "mix" else t["output_size"]
            if not 0 <= a[2] < lim:
                ibad(f"names word {a[2]} of {args[a[1]]}, which {os.path.basename(tpath)} sizes at {lim}")
        elif op in "+-*":
            if max(a[1:]) >= a[0]:
                ibad("an operand is not an earlier id")
        elif op in "ab":
            if max(a[1:-1]) >= a[0]:
                ibad("an operand is not an earlier id")
            if not 0 <= a[-1] < len(pm):
                ibad(f"names poly_mix power {a[-1]}, which {os.path.basename(tpath)} (poly_mix_powers) does not have")
    return t


def main():
    try:
        if sys.argv[1:] == ["--names"]:
            print(" ".join(n for n, _ in circuits()))
        elif sys.argv[1:] == ["--check"]:
            for n, d in circuits():
                print(n, d)
        else:
            sys.exit(__doc__)
    except CircuitError as e:
        sys.exit(f"circuit_files.py: {e}")


if __name__ == "__main__":
    main()
