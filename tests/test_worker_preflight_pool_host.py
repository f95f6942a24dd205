"""The worker's preflight pool without a GPU (r0hip_worker_set_preflight_threads,
r0hip_worker_get_stats):
  * risc0_amd/csrc/preflight_pool.h driven by tests/native/preflight_pool_host.cpp, a stand-alone
    program with a fake work function and malloc-backed slots: pool sizes 1, 2, 3 and 8, 1 and 3
    releasers, 0, 1 and 200 jobs, a stop with jobs queued, resizes between batches. It checks that
    every job is consumed once and in order, that a failure stays with its job, that the slots in
    use never exceed n + in_flight + 1 and that everything is joined and freed. Built and run
    plain, under ThreadSanitizer and under AddressSanitizer + UBSan, each as its own program (a
    sanitizer leg is skipped, with the reason, only where its runtime is not installed or cannot
    start even a one-line program);
  * the header is free of HIP;
  * the two entry points are declared in the header with their tag, in hal.py, in sys_hip.rs and
    in INTEGRATION.md, and the ctypes and Rust mirrors of r0hip_worker_stats have the C layout;
  * the refusals that need no device: w == NULL, a wrong out_size."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "preflight_pool_host.cpp")
INC = os.path.join(ROOT, "risc0_amd", "csrc")
HEADER = os.path.join(INC, "preflight_pool.h")
NAMES = ("r0hip_worker_set_preflight_threads", "r0hip_worker_get_stats")
RUN_S = 300

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _sanitizer_runner(flags, tmp_path):
    """How a program built with these sanitizer flags is built and started here: (extra link flags,
    command prefix), or a str, the reason why the runtime cannot be used on this host. A one-line
    program is the probe. Not installed: the probe does not link. Installed but unable to start
    any program here: the probe itself dies in the runtime's start-up, before main (ThreadSanitizer
    on a kernel whose address-space randomisation it does not know: "unexpected memory mapping";
    then the probe is tried once more with randomisation off for that one process, setarch -R)."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    probe = tmp_path / "probe"
    # the runtime inside the program where the toolchain has it as an archive, else the shared one
    static = {"-fsanitize=thread": ["-static-libtsan"], "-fsanitize=address,undefined": ["-static-libasan",
                                                                                          "-static-libubsan"]}[flags[0]]
    reason = None
    for extra in (static, []):
        cc = subprocess.run(["g++", *flags, *extra, "-pthread", "-o", str(probe), str(src)], capture_output=True,
                            text=True)
        if cc.returncode:
            reason = reason or "not installed: " + (cc.stderr.strip().split("\n") or ["g++ failed"])[-1][:300]
            continue
        prefixes = [[]]
        if shutil.which("setarch"):
            prefixes.append(["setarch", os.uname().machine, "-R"])
        for prefix in prefixes:
            run = subprocess.run([*prefix, str(probe)], capture_output=True, text=True, timeout=60)
            if run.returncode == 0:
                return extra, prefix
            reason = "cannot start a program on this host: " + (run.stderr.strip().split("\n") or ["?"])[0][:300]
    return reason


@needs_gxx
@pytest.mark.parametrize("name, flags", [
    ("plain", []),
    ("tsan", ["-fsanitize=thread"]),
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_the_pool_under_a_fake_worker(tmp_path, name, flags):
    extra, prefix = [], []
    if flags:
        how = _sanitizer_runner(flags, tmp_path)
        if isinstance(how, str):
            pytest.skip(f"the runtime of {flags[0]}: {how}")
        extra, prefix = how
    exe = tmp_path / f"preflight_pool_host_{name}"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", *flags, *extra, "-I", INC,
                    "-o", str(exe), SRC], check=True)
    out = subprocess.run([*prefix, str(exe)], capture_output=True, text=True, timeout=RUN_S)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-6000:]
    for mark in ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert mark not in out.stderr, out.stderr[-6000:]
    m = re.search(r"^ok: (\d+) scenarios, (\d+) jobs$", out.stdout.strip().split("\n")[-1])
    # 4 pool sizes x 2 in-flight counts x 3 job counts x (run out, stopped early), and 2 resize runs
    assert m and int(m.group(1)) == 4 * 2 * 3 * 2 + 2 and int(m.group(2)) > 3000, out.stdout[-500:]


def test_the_pool_header_has_no_hip():
    text = open(HEADER).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, flags=re.M)
    assert includes and not [i for i in includes if "hip" in i.lower() or i in ("runtime.h", "devmem.h")], includes
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\bhip[A-Z]\w*", code)


def test_the_entry_points_are_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    assert re.search(r"/\* \[host-only\] \*/\nconst char\* r0hip_worker_set_preflight_threads\("
                     r"r0hip_worker\* w, uint32_t n, uint32_t\* was\);", hdr)
    assert re.search(r"/\* \[host-only\] \*/\nconst char\* r0hip_worker_get_stats\("
                     r"r0hip_worker\* w, r0hip_worker_stats\* out, size_t out_size\);", hdr)
    hal = open(os.path.join(ROOT, "risc0_amd", "hal.py")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert f'"{n}"' in hal, n
        assert re.search(r"pub fn " + n + r"\(", rs), n
        assert n in doc, n
    assert "def set_preflight_threads(self, n)" in hal and "def stats(self)" in hal


def _c_fields(hdr):
    m = re.search(r"typedef struct r0hip_worker_stats \{(.*?)\} r0hip_worker_stats;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            out += [w.strip().split()[-1] for w in decl.split(",")]
    return out


def test_the_stats_struct_has_one_layout(tmp_path):
    """the header's fields, in order, in the ctypes and the Rust mirror; sizeof and every offset of
    the ctypes mirror against a C program compiled with the header"""
    from risc0_amd import hal
    hdr = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    fields = _c_fields(hdr)
    assert fields == ["preflight_threads", "preflight_slots", "peak_slots_in_use", "reserved", "pool_jobs",
                      "inline_jobs", "slot_bytes", "pool_busy_ms", "uploader_preflight_ms",
                      "uploader_wait_preflight_ms"]
    assert [f[0] for f in hal.WorkerStats._fields_] == fields
    rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    m = re.search(r"pub struct R0HipWorkerStats \{(.*?)\n\}", rs, flags=re.S)
    assert m and re.findall(r"pub (\w+):", m.group(1)) == fields
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc for the offsets")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "r0hip.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(r0hip_worker_stats));']
    lines += [f'  printf("{f} %zu\\n", offsetof(r0hip_worker_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.strip().split("\n"))
    assert int(got["sizeof"]) == C.sizeof(hal.WorkerStats) == 64
    for f in fields:
        assert int(got[f]) == getattr(hal.WorkerStats, f).offset, f


def _message(err):
    import risc0_amd as r
    assert err, "the call was not refused"
    msg = C.cast(err, C.c_char_p).value.decode()
    r.lib().r0hip_free_error(err)
    return msg


def test_refusals_that_need_no_device():
    import risc0_amd as r
    L = r.lib()
    was = C.c_uint32(77)
    assert "r0hip_worker_set_preflight_threads: w is NULL" in _message(
        L.r0hip_worker_set_preflight_threads(None, 2, C.byref(was)))
    assert was.value == 77
    st = r.WorkerStats()
    assert "r0hip_worker_get_stats: w is NULL" in _message(L.r0hip_worker_get_stats(None, C.byref(st), C.sizeof(st)))
    # a wrong out_size is refused before the handle is read (the address below is never followed)
    buf = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(buf))
    for size in (0, C.sizeof(st) - 8, C.sizeof(st) + 8):
        msg = _message(L.r0hip_worker_get_stats(fake, C.byref(st), size))
        assert f"out_size {size}" in msg and f"sizeof(r0hip_worker_stats) {C.sizeof(st)}" in msg, msg
    assert "out is NULL" in _message(L.r0hip_worker_get_stats(fake, None, C.sizeof(st)))
