"""Host-side checks of the node-heap mirror budget and the path-fetch fallback (no GPU): the
driver exports the budget's entry points, the Rust HAL carries the same fallback, and the
bookkeeping itself (integration/node_reads.h) runs as a stand-alone program against host stubs
of the three r0hip_* calls it makes, under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "integration"))


def test_driver_exports_the_budget_entry_points():
    import halprover
    out = subprocess.check_output(["nm", "-D", "--defined-only", halprover.LIB_PATH], text=True)
    defined = {ln.split()[-1] for ln in out.splitlines()}
    for n in ("halp_set_mirror_budget", "halp_mirror_stats", "halp_reset_mirror_stats"):
        assert n in defined, n
    hdr = open(os.path.join(ROOT, "integration", "hal_prover.h")).read()
    assert re.search(r"halp_set_mirror_budget\(uint64_t bytes\)", hdr)
    assert re.search(r"halp_mirror_stats\(uint64_t out\[5\]\)", hdr)
    # the fallback is the per-op path fetch
    used = subprocess.check_output(["nm", "-D", "--undefined-only", halprover.LIB_PATH], text=True)
    assert "r0hip_merkle_paths_host" in used


def test_rust_hal_has_the_budget_and_the_path_fetch():
    rs = open(os.path.join(ROOT, "integration", "rust", "hal_hip.rs")).read()
    assert re.search(r"r0hip_merkle_paths_host\(", rs)
    assert re.search(r"pub fn with_mirror_budget\(", rs)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "sys_hip.rs")).read()
    assert re.search(r"pub fn r0hip_merkle_paths_host\(", sys_rs)
    py = open(os.path.join(ROOT, "risc0_amd", "hal.py")).read()
    assert '"r0hip_merkle_paths_host"' in py and "def merkle_paths_host(self, nodes, idx, levels)" in py


def test_rust_hal_takes_the_copy_handle_before_finishing_it():
    """DeviceAlloc::host: r0hip_copy_finish releases the handle even when it fails, so the handle
    leaves `pending` before the call and returns only when the copy is not done yet"""
    rs = open(os.path.join(ROOT, "integration", "rust", "hal_hip.rs")).read()
    m = re.search(r"fn host\(&self\)[^{]*\{", rs)
    body = rs[m.end():rs.index("\n    }\n", m.end())]
    take, finish, back = (body.find(s) for s in ("self.pending.replace(std::ptr::null_mut())", "r0hip_copy_finish(",
                                                 "self.pending.set(c)"))
    assert 0 <= take < finish < back, (take, finish, back)
    assert "self.pending.get()" not in body


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_budget_and_path_cache_under_sanitizers(tmp_path):
    exe = tmp_path / "node_reads_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), os.path.join(ROOT, "tests", "native", "node_reads_host.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK") and "runtime error" not in out.stderr
