"""bench.py's host-side choices (no GPU): which committed PMC summary the roofline quotes,
which legs a plain run leaves to --full, and the files --dump-outputs writes."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _summaries(tmp_path, tags, lib_of):
    prof = tmp_path / "profiles"
    prof.mkdir()
    for t in tags:
        doc = {"kernels": {}, "per_proof": {}}
        if t in lib_of:
            doc["lib_sha256_16"] = lib_of[t]
        (prof / f"{t}_pmc_valu.json").write_text(json.dumps(doc))
    return prof


def test_pmc_summary_round_order(tmp_path, monkeypatch):
    # r5an is newer than r5v (tag length first), r5a newer than r4x: plain string order gets both wrong
    _summaries(tmp_path, ["r4x", "r5a", "r5v", "r5z", "r5aa", "r5an"], {})
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "lib_fingerprint", lambda: "0123456789abcdef")
    assert os.path.basename(bench.pmc_summary_file("valu")) == "r5an_pmc_valu.json"
    assert bench.pmc_summary_file("traffic") is None


def test_pmc_summary_prefers_loaded_library(tmp_path, monkeypatch):
    _summaries(tmp_path, ["r5p", "r5v", "r5an"], {"r5p": "aaaa", "r5v": "bbbb", "r5an": "cccc"})
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "lib_fingerprint", lambda: "bbbb")
    assert os.path.basename(bench.pmc_summary_file("valu")) == "r5v_pmc_valu.json"
    monkeypatch.setattr(bench, "lib_fingerprint", lambda: "dddd")
    assert os.path.basename(bench.pmc_summary_file("valu")) == "r5an_pmc_valu.json"


def _legs(args):
    rsteps = args.steps if args.resident_steps is None else args.resident_steps
    return (rsteps, args.e2e_steps, args.accum_steps, args.per_op_steps, not args.no_prove_only, not args.no_cpu_baseline)


def test_plain_run_has_no_side_legs(monkeypatch):
    # a plain run times the headline alone, whatever the leg options say; --full runs them as sized
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--per-op-steps", "5"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    assert _legs(args) == (0, 0, 0, 0, False, False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--full", "--accum-steps", "0"])
    assert _legs(bench.parse()) == (7, 6, 0, 3, True, True)


def test_dump_outputs_files(tmp_path):
    import numpy as np
    seal = np.array([0, 1, 0xFFFFFFFF, 15 * 2**27], dtype=np.uint32)
    mix = np.arange(36, dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "d"), 0, seal, mix)
    bench.dump_outputs(str(tmp_path / "d"), 2, mix, seal)
    assert sorted(os.listdir(tmp_path / "d")) == ["mix.npy", "mix_rank2.npy", "seal.npy", "seal_rank2.npy"]
    got = np.load(tmp_path / "d" / "seal.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), seal)  # u32 words are exact in float64
    assert np.array_equal(np.load(tmp_path / "d" / "mix_rank2.npy"), seal.astype(np.float64))
