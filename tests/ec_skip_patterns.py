"""Shared by test_ec_skip_host.py and test_ec_skip_gpu.py: the patterns of selector columns set to
zero, and for each pattern how many kernels of the generated program are then not launched, per
circuit and family ("ec": eval_check on the 4N domain, "rows": the constraint-rows family on the N
trace rows). The numbers hold for the committed tuning files (the rows family reads none); the
host test derives them from the generated plan() on the CPU, the device test from
r0hip_eval_check_launched, and both must agree with this table."""

# rv32im data columns: 1 + major are the one-hot major selectors, 22..28 the minor selectors
MAJORS = list(range(1, 14))
MINORS = list(range(22, 29))
LOOP_MIDDLE = [2, 4, 5, 6, 7, 9, 12, 13]  # zero in a middle segment of the loop guest
# recursion's selectors are code columns
REC_GATES = [1, 2, 3, 4, 5, 6, 7, 17]

KERNELS = {("rv32im", "ec"): 30, ("rv32im", "rows"): 34, ("recursion", "ec"): 7, ("recursion", "rows"): 7}


def patterns(circuit):
    """name -> the (group, column) pairs set to zero"""
    if circuit == "rv32im":
        pats = {"none": [], "loop_middle": [("data", c) for c in LOOP_MIDDLE],
                "all_majors": [("data", c) for c in MAJORS], "minors": [("data", c) for c in MINORS]}
        pats.update({f"major_col{c}": [("data", c)] for c in MAJORS})
        return pats
    pats = {"none": [], "all_gates": [("code", c) for c in REC_GATES]}
    pats.update({f"code_col{c}": [("code", c)] for c in REC_GATES})
    return pats


def _rv(none, loop_middle, all_majors, minors, singles):
    out = {"none": none, "loop_middle": loop_middle, "all_majors": all_majors, "minors": minors}
    out.update({f"major_col{c}": n for c, n in zip(MAJORS, singles)})
    return out


def _rec(all_gates, singles):
    out = {"none": 0, "all_gates": all_gates}
    out.update({f"code_col{c}": n for c, n in zip(REC_GATES, singles)})
    return out


# kernels not launched, by pattern
SKIPPED = {
    ("rv32im", "ec"): _rv(0, 14, 26, 9, [0, 1, 0, 2, 3, 0, 0, 4, 2, 4, 1, 3, 0]),
    ("rv32im", "rows"): _rv(0, 13, 31, 11, [1, 0, 0, 2, 3, 0, 0, 4, 1, 6, 1, 4, 1]),
    ("recursion", "ec"): _rec(4, [0, 1, 0, 0, 0, 0, 0, 0]),
    ("recursion", "rows"): _rec(4, [0, 1, 0, 0, 0, 0, 0, 0]),
}


def zeroed(plain, cols, n):
    """plain: buffer name -> flat column-major array of n points per column"""
    out = {k: v.copy() for k, v in plain.items()}
    for g, c in cols:
        out[g][c * n:(c + 1) * n] = 0
    return out
