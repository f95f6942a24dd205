"""Shared by the circuit-module tests (test_circuit_module_host.py, test_circuit_module_gpu.py):
the modules the default build makes (risc0_amd/modules/), loaded once per process, and stub
modules, plain C++ with no kernels, for the refusals that need a malformed module."""
import os
import subprocess

import circuit_rt_util as U

ROOT = U.ROOT
CSRC = os.path.join(ROOT, "risc0_amd", "csrc")
# name -> the compiled-in circuit with the same program (None: compiled in nowhere)
MODULES = {"mod_demo": "demo", "mod_recursion": "recursion", "mod_variant": None}


def module_path(name):
    from risc0_amd import hal
    return os.path.join(hal.MODULE_DIR, name + ".r0mod.so")


def loaded(name):
    """the module's circuit name, loading it on first use (the registry has no way out, so a
    process loads each once)"""
    from risc0_amd import hal
    assert name in MODULES
    if name not in hal.circuit_names():
        assert hal.load_circuit_module(module_path(name)) == name
    return name


def stub_source(t, name, abi="R0HIP_MODULE_ABI", args_size="sizeof(EvalCheckArgs)", arch="gfx950", nargs=None,
                col=(0, 0), entry="r0hip_circuit_module"):
    """A module of the tables dict `t` (circuit_tables.load) whose "kernels" are empty functions:
    good as it stands, and wrong in the one thing a keyword changes. col: the one (argument,
    column) pair its info() names."""
    arr = lambda xs: ", ".join(str(int(x)) for x in xs) or "0"
    nargs = len(t["eval_args"]) if nargs is None else nargs
    info = t["circuit_info"].encode()
    return f"""
#include "r0hip_module.h"
#include "evalcheck_types.h"
using namespace r0;
static const uint32_t taps[] = {{{arr(t['taps'])}}}, combo_taps[] = {{{arr(t['combo_taps'])}}},
    combo_begin[] = {{{arr(t['combo_begin'])}}}, group_begin[] = {{{arr(t['group_begin'])}}},
    group_sizes[] = {{{arr(t['group_sizes'])}}}, pm[] = {{{arr(t['poly_mix_powers'])}}}, ir[] = {{{arr(t['ir'])}}};
static const int32_t args[] = {{{arr(t['eval_args'])}}};
static const int col_arg[] = {{{col[0]}}}, col_idx[] = {{{col[1]}}};
static void info(EvalCheckInfo* o) {{
  *o = EvalCheckInfo{{}};
  o->nargs = {nargs}; o->npm = {len(t['poly_mix_powers'])}; o->kernels = 1;
  o->ncols = 1; o->col_arg = col_arg; o->col_idx = col_idx;
}}
static void never_launched() {{}}
static const r0hip_module_desc desc = {{
  {abi}, sizeof(r0hip_module_desc), {args_size}, sizeof(EvalCheckInfo), "{arch}",
  {{"{name}", taps, {t['n_taps']}, combo_taps, {len(t['combo_taps'])}, combo_begin, {t['combos_count']}, group_begin,
   {t['n_groups']}, group_sizes, pm, {len(t['poly_mix_powers'])}, {{{arr(info)}}}, {t['mix_size']}, {t['output_size']},
   args, {len(t['eval_args'])}, ir, {t['n_ir']}}},
  never_launched, reinterpret_cast<r0hip_module_fn>(&info), never_launched, reinterpret_cast<r0hip_module_fn>(&info)}};
extern "C" const r0hip_module_desc* {entry}(void) {{ return &desc; }}
"""


def build_stub(directory, stem, source):
    """g++ -shared of a stub's source; the path of the shared object"""
    src, out = os.path.join(str(directory), stem + ".cpp"), os.path.join(str(directory), stem + ".r0mod.so")
    with open(src, "w") as f:
        f.write(source)
    cc = subprocess.run(["g++", "-std=c++17", "-O0", "-shared", "-fPIC", "-Wall", "-I", os.path.join(ROOT, "include"),
                         "-I", CSRC, src, "-o", out], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return out
