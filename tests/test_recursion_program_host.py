"""Host-side checks of the resident recursion programs (r0hip_recursion_program_*), no device
needed: every refusal of r0hip_recursion_program_create comes back as an error string that names
the argument (and for a word its index) before any device call; the other entry points refuse a
NULL handle; r0hip_worker_job keeps its layout and r0hip_worker_program_job appends `program` to
it; the header is still C11; the ctypes and Rust mirrors list the header's fields in order."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 15 * 2**27 + 1
u32p = C.POINTER(C.c_uint32)


def _create(code, po2=11, suite=0, form=0, n_words=None, out=True, null_code=False):
    """r0hip_recursion_program_create's error text (None on success) and the handle value"""
    import risc0_amd as r
    L = r.lib()
    c = np.ascontiguousarray(code, dtype=np.uint32)
    h = C.c_void_p(1)
    err = L.r0hip_recursion_program_create(C.byref(h) if out else None, suite, po2,
                                           None if null_code else c.ctypes.data_as(u32p),
                                           c.size if n_words is None else n_words, form)
    msg = None
    if err:
        msg = C.cast(err, C.c_char_p).value.decode()
        L.r0hip_free_error(err)
    return msg, h.value


ROW = np.zeros(23, dtype=np.uint32)


@pytest.mark.parametrize("kwargs, needles", [
    (dict(out=False), ["out is NULL"]),
    (dict(null_code=True), ["h_code is NULL"]),
    (dict(suite=3), ["suite 3"]),
    (dict(suite=-1), ["suite -1"]),
    (dict(form=2), ["form 2"]),
    (dict(po2=10), ["po2 10"]),
    (dict(po2=25), ["po2 25"]),
    (dict(n_words=0), ["n_words is 0"]),
    (dict(n_words=22), ["n_words 22", "multiple of 23"]),
    (dict(n_words=24), ["n_words 24", "multiple of 23"]),
])
def test_create_refuses_bad_arguments_on_the_host(kwargs, needles):
    msg, handle = _create(ROW, **kwargs)
    assert msg is not None and msg.startswith("r0hip: r0hip_recursion_program_create: "), msg
    for n in needles:
        assert n in msg, msg
    if kwargs.get("out", True):
        assert not handle  # *out is cleared before anything can fail


@pytest.mark.parametrize("po2", [11, 12])
def test_create_refuses_a_program_longer_than_the_segment(po2):
    """more than 2^po2 - 1024 rows (program.rs:56-57); the limit itself passes this check (it
    then needs a device, which the GPU tests have)"""
    limit = (1 << po2) - 1024
    msg, handle = _create(np.zeros(23 * (limit + 1), dtype=np.uint32), po2=po2)
    assert msg is not None and f"{limit + 1} rows" in msg and "n_words" in msg and str(limit) in msg, msg
    assert not handle


@pytest.mark.parametrize("index, word", [(0, P), (22, P + 1), (23 * 5 + 7, 2**31), (23 * 40 - 1, 2**32 - 1)])
def test_create_refuses_a_noncanonical_montgomery_word_with_its_index(index, word):
    code = np.zeros(23 * 40, dtype=np.uint32)
    code[index] = word
    code[index + 1:] = P - 1  # canonical: the first bad word is the one reported
    msg, handle = _create(code, form=1)
    assert msg is not None and f"h_code[{index}]" in msg and str(word) in msg, msg
    assert not handle


def _no_device():
    return not (os.environ.get("HIP_VISIBLE_DEVICES") is None and os.path.exists("/dev/kfd"))


def test_encoded_form_accepts_every_u32_on_the_host():
    """in the encoded form no word is refused: with p, 2^31 and 2^32 - 1 among them the call gets
    past the host checks and, without a device, fails in the runtime instead"""
    if not _no_device():
        return  # a GPU may be present; the GPU tests create such programs
    code = np.zeros(23 * 4, dtype=np.uint32)
    code[[0, 30, 91]] = [P, 2**31, 2**32 - 1]
    msg, handle = _create(code, form=0)
    assert msg is not None and "r0hip_recursion_program_create" not in msg, msg
    assert not handle


def test_other_entry_points_refuse_a_null_handle():
    import risc0_amd as r
    L = r.lib()
    n = C.c_size_t(0)
    p = C.c_void_p()
    calls = {
        "r0hip_recursion_program_info": lambda: L.r0hip_recursion_program_info(None, None, None, None, None, None),
        "r0hip_recursion_program_ctrl": lambda: L.r0hip_recursion_program_ctrl(None, C.byref(p)),
        "r0hip_prove_recursion_program": lambda: L.r0hip_prove_recursion_program(None, None, 0, None, 0, None, 0, None,
                                                                                 0, None, 0, C.byref(n), None),
        "r0hip_recursion_program_destroy": lambda: L.r0hip_recursion_program_destroy(None),
    }
    for name, call in calls.items():
        err = call()
        assert err, name
        msg = C.cast(err, C.c_char_p).value.decode()
        L.r0hip_free_error(err)
        assert name in msg and "program is NULL" in msg, msg


def test_new_entry_points_are_declared_exported_and_bound():
    import risc0_amd as r
    L = r.lib()
    declared = r.exported_symbols()
    for n in ("r0hip_recursion_program_create", "r0hip_recursion_program_info", "r0hip_recursion_program_ctrl",
              "r0hip_prove_recursion_program", "r0hip_recursion_program_destroy"):
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    assert re.search(r"#define R0HIP_JOB_RECURSION_PROGRAM 3\b", hdr)
    assert re.search(r"#define R0HIP_CODE_ENCODED\s+0\b", hdr) and re.search(r"#define R0HIP_CODE_MONTGOMERY\s+1\b", hdr)
    from risc0_amd import hal
    assert hal.JOB_RECURSION_PROGRAM == 3 and (hal.CODE_ENCODED, hal.CODE_MONTGOMERY) == (0, 1)


# r0hip_worker_job as it was before this kind of job: the same declarations, in a struct of the
# probe's own, give the offsets its fields must keep
OLD_JOB = """typedef struct old_worker_job {
  uint32_t kind; int suite; uint32_t po2; r0hip_trace_input trace; const r0hip_bigint_back* h_bigint;
  size_t n_bigint; r0hip_recursion_input recursion; void* user; uint32_t* h_seal; size_t seal_cap; size_t seal_len;
  uint32_t* h_mix_out; const char* error; int verified; double verify_ms; double prove_ms; uint64_t ticket;
  const r0hip_backs* backs;
} old_worker_job;"""
OLD_FIELDS = ["kind", "suite", "po2", "trace", "h_bigint", "n_bigint", "recursion", "user", "h_seal", "seal_cap",
              "seal_len", "h_mix_out", "error", "verified", "verify_ms", "prove_ms", "ticket", "backs"]


def test_worker_job_keeps_its_old_offsets_and_program_is_last():
    """a gcc offsetof probe against the header, compiled as C11 with -Wall -Werror -pedantic: the
    handle travels in r0hip_worker_program_job, whose first member is the job struct with its old
    size and offsets and whose last member, right behind it, is `program`"""
    from risc0_amd import hal
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', OLD_JOB, "int main(void) {"]
    for f in OLD_FIELDS:
        lines.append(f'  printf("{f} %zu %zu\\n", offsetof(r0hip_worker_job, {f}), offsetof(old_worker_job, {f}));')
    lines.append('  printf("jobsize %zu %zu\\n", sizeof(r0hip_worker_job), sizeof(old_worker_job));')
    lines.append('  printf("job %zu %zu\\n", offsetof(r0hip_worker_program_job, job), (size_t)0);')
    lines.append('  printf("program %zu %zu\\n", offsetof(r0hip_worker_program_job, program), sizeof(r0hip_worker_job));')
    lines.append('  printf("sizeof %zu %zu\\n", sizeof(r0hip_worker_program_job), sizeof(const r0hip_recursion_program*));')
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                             src, "-o", exe], capture_output=True, text=True)
        if cc.returncode:
            pytest.fail("the header does not compile as C11:\n" + cc.stderr)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in out if ln}
    for f in OLD_FIELDS + ["jobsize", "job", "program"]:
        assert got[f][0] == got[f][1], f
    for f in OLD_FIELDS:
        assert got[f][0] == getattr(hal.WorkerJobStruct, f).offset, f
    assert C.sizeof(hal.WorkerJobStruct) == got["jobsize"][0]
    # `program` is the last member: nothing follows it
    assert got["sizeof"][0] == got["program"][0] + got["sizeof"][1]
    assert hal.WorkerProgramJobStruct.job.offset == 0
    assert hal.WorkerProgramJobStruct.program.offset == got["program"][0]
    assert C.sizeof(hal.WorkerProgramJobStruct) == got["sizeof"][0]
    assert [f[0] for f in hal.WorkerProgramJobStruct._fields_] == ["job", "program"]


def _c_fields(hdr, cname):
    m = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S)
    assert m, cname
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_mirrors_list_the_header_fields_in_order():
    from risc0_amd import hal
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    for cname, rname, py, want in (("r0hip_worker_job", "R0HipWorkerJob", hal.WorkerJobStruct, OLD_FIELDS),
                                   ("r0hip_worker_program_job", "R0HipWorkerProgramJob", hal.WorkerProgramJobStruct,
                                    ["job", "program"])):
        cfields = _c_fields(hdr, cname)
        assert cfields == want, cname
        m = re.search(r"#\[repr\(C\)\]\s*pub struct " + rname + r" \{(.*?)\n\}", rs, flags=re.S)
        assert m, rname
        assert re.findall(r"pub (\w+):", m.group(1)) == cfields, rname
        assert [f[0] for f in py._fields_] == cfields, cname
    assert re.search(r"pub job: R0HipWorkerJob,\s*pub program: \*const R0HipRecursionProgram,", rs)
    assert re.search(r"pub const R0HIP_JOB_RECURSION_PROGRAM: u32 = 3;", rs)
