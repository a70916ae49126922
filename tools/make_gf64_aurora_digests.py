#!/usr/bin/env python3
"""Writes tests/golden/gf64_aurora.json: the SHA-256 and the length of the CPU oracle's Aurora transcripts over GF(2^64) at 2^12, 2^14, 2^16
and 2^18 constraints (15 inputs, seed 0x2204, default rate and localization).  2^14 coefficients are more than one 2^12-element tile of the
gf64 transform, so a proof of that size runs the multi-pass phase 1 of the LDE; 2^16 is the smaller size tools/gf64_aurora_bench.py quotes;
2^18 has a codeword of 2^24 points, past the launch caps of the protocol kernels.  The oracle takes 0.5, 2.5, 12 and about 55 minutes of one
core at these sizes (about 4.6 x per step; 2^20 would take hours and is not recorded): the GPU suite (tests/test_gpu_gf64_aurora.py)
compares against the recorded digests instead of calling it.

    python tools/make_gf64_aurora_digests.py [log_n ...]        # the sizes given, or all; entries of other sizes are kept"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

CASES = [(12, 15), (14, 15), (16, 15), (18, 15)]
SEED = 0x2204


def main():
    path = os.path.join(ROOT, "tests", "golden", "gf64_aurora.json")
    wanted = [int(a) for a in sys.argv[1:]] or [c[0] for c in CASES]
    entries = []
    if os.path.exists(path):
        with open(path) as f:
            entries = [e for e in json.load(f)["aurora"] if e["log_n"] not in wanted]
    for log_n, num_inputs in CASES:
        if log_n not in wanted:
            continue
        t0 = time.time()
        transcript = oracle.aurora_prove(oracle.FIELD_GF64, log_n, num_inputs, SEED)
        assert oracle.aurora_verify(oracle.FIELD_GF64, log_n, num_inputs, SEED, transcript)
        entries.append({"field": "gf64", "log_n": log_n, "num_inputs": num_inputs, "seed": SEED, "bytes": len(transcript),
                        "sha256": hashlib.sha256(transcript).hexdigest()})
        print("2^%d constraints: %d bytes, %.0f s" % (log_n, len(transcript), time.time() - t0), flush=True)
    entries.sort(key=lambda e: e["log_n"])
    with open(path, "w") as f:
        json.dump({"aurora": entries}, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
