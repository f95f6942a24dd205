#!/usr/bin/env python3
"""Record the demo circuit's golden seal (tests/golden/demo/) on a GPU: the device witness of
tests/test_plugin_gpu.py (its noise key, a0, b0 and active rows) proved through
r0hip_prove_segment_cb at po2 8 with Poseidon2, checked by the host verifier before it is written.

Usage: make_demo_golden.py [OUTDIR]      (default tests/golden/demo)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import risc0_amd as r
    from risc0_amd import hal as H
    import test_plugin_gpu as T
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "demo")
    os.makedirs(out, exist_ok=True)
    suite, po2 = 0, 8
    seal, mix, _ = T._prove_demo(r.HipHal(T.SUITE_NAMES[suite]), po2)
    assert H.verify_seal("demo", suite, seal) == po2
    name = f"seal_demo_{T.SUITE_NAMES[suite]}_po2_{po2}.npy"
    np.save(os.path.join(out, name), seal)
    with open(os.path.join(out, "index.json"), "w") as f:
        json.dump({"seals": [{"file": name, "suite": suite, "po2": po2, "words": int(seal.size)}]}, f, indent=1)
        f.write("\n")
    print(f"wrote {name}: {seal.size} words")


if __name__ == "__main__":
    main()
