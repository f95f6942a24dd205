"""Load-time refusals of a circuit module's gate view (circuit_module.cpp check_kernel_view, no GPU):
EvalCheckInfo's ngates, gate_col and plan, which eval_check's zero scan and launch plan read. A
stub module (circuit_module_util.stub_source: plain C++, empty kernels) is wrong in the one thing
each case changes; the sound variant with one gate is the control."""
import re

import pytest

import circuit_module_util as M
import circuit_rt_util as U

PLAN = "static uint64_t plan(uint64_t) { return 1; }\nstatic const int gate_col[] = {%d};\nstatic void info("
# the demo's eval_args are code, global, data, mix, accum: argument 0 is code, argument 1 is global
CASES = [
    ("ngates_out_of_range", (0, 0), "o->ngates = 65; o->gate_col = gate_col; o->plan = plan;", 0,
     r"info\(\): ngates: 65 is not 0 to 64$"),
    ("ngates_negative", (0, 0), "o->ngates = -1;", 0, r"info\(\): ngates: -1 is not 0 to 64$"),
    ("gate_col_null", (0, 0), "o->ngates = 1; o->plan = plan;", 0, r"info\(\): gate_col, plan: NULL with ngates 1$"),
    ("plan_null", (0, 0), "o->ngates = 1; o->gate_col = gate_col;", 0, r"info\(\): gate_col, plan: NULL with ngates 1$"),
    ("gate_outside_the_columns", (0, 0), "o->ngates = 1; o->gate_col = gate_col; o->plan = plan;", 1,
     r"info\(\): gate_col: gate 0 names column 1 of 1$"),
    ("gate_on_global", (1, 0), "o->ngates = 1; o->gate_col = gate_col; o->plan = plan;", 0,
     r"info\(\): gate_col: gate 0 is a column of mix or global, not of a witness group$"),
]


def stub(name, col, fields, gate):
    src = M.stub_source(U.tables("demo"), name, col=col)
    assert src.count("static void info(") == 1 and src.count("o->ncols = 1;") == 1
    return src.replace("static void info(", PLAN % gate).replace("o->ncols = 1;", "o->ncols = 1; " + fields)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_malformed_gate_view_is_refused(case, tmp_path):
    from risc0_amd import hal
    cid, col, fields, gate, want = case
    t = U.tables("demo")
    assert t["eval_args"] == [1, -2, 2, -1, 0]
    path = M.build_stub(tmp_path, cid, stub("gates_refused", col, fields, gate))
    before = hal.circuit_names()
    with pytest.raises(hal.R0HipError, match=r"^r0hip: r0hip_circuit_load: " + re.escape(str(path)) + ": " + want):
        hal.load_circuit_module(str(path))
    assert hal.circuit_names() == before


def test_a_sound_gate_view_loads(tmp_path):
    from risc0_amd import hal
    path = M.build_stub(tmp_path, "gates_ok", stub("gates_ok", (0, 0), "o->ngates = 1; o->gate_col = gate_col; o->plan = plan;", 0))
    if "gates_ok" not in hal.circuit_names():
        assert hal.load_circuit_module(str(path)) == "gates_ok"
    assert "gates_ok" in hal.circuit_names()
