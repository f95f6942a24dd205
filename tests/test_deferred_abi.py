"""The deferred completion mode's two entry points are part of the declared C ABI (no GPU):
the header, the Python binding and the Rust binding all name them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("r0hip_set_deferred", "r0hip_call_stats")


def test_exported_symbols_contain_the_deferred_entry_points():
    from risc0_amd import hal
    syms = hal.exported_symbols()
    for n in NAMES:
        assert n in syms, n


def test_python_and_rust_bindings_declare_them():
    py = open(os.path.join(ROOT, "risc0_amd", "hal.py")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    for n in NAMES:
        assert f'"{n}"' in py, n
        assert re.search(r"pub fn " + n + r"\(", rs), n
    hal_rs = open(os.path.join(ROOT, "integration", "rust", "hal_hip.rs")).read()
    assert re.search(r"pub fn with_deferred\(deferred: bool\) -> Self", hal_rs)


def test_every_prototype_states_its_completion_kind():
    """include/r0hip.h tags each entry point [queues], [drains] or [host-only]; the per-op
    calls that hand data or a verdict to the host are [drains]"""
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    kinds = dict((name, kind) for kind, name in
                 re.findall(r"/\* \[(queues|drains|host-only)\] \*/\nconst char\* (r0hip_\w+)\(", hdr))
    protos = set(re.findall(r"^const char\* (r0hip_\w+)\(", hdr, flags=re.M))
    assert protos == set(kinds)
    for n in ("memcpy_d2h", "memcpy_h2d", "gather_sample_host", "poly_divide", "combos_divide", "synchronize",
              "eval_check", "rv32im_witgen", "recursion_witgen", "prove_segment", "prove_segment_trace",
              "prove_recursion", "trim", "kernel_times"):
        assert kinds["r0hip_" + n] == "drains", n
    for n in ("alloc", "free", "memset32", "memcpy_d2d", "batch_interpolate_ntt", "hash_rows", "hash_fold",
              "merkle_tree", "mix_poly_coeffs", "fri_fold", "combos_prepare", "recursion_accum", "rv32im_accum"):
        assert kinds["r0hip_" + n] == "queues", n
    assert kinds["r0hip_set_deferred"] == kinds["r0hip_call_stats"] == kinds["r0hip_verify_seal"] == "host-only"
