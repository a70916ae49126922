#!/usr/bin/env python3
"""Writes tests/golden/gf64_fractal.json: the SHA-256, the length and the index Merkle roots of the CPU oracle's Fractal transcripts over GF(2^64) at
2^10 and 2^14 constraints (no inputs, seed 0x2205, rate 3, localization 2), and beside them that the oracle's verifier accepted the transcript and
rejected it with one bit flipped in the middle.  The oracle's indexer and prover take about 25 s of one core at 2^10 and several minutes at 2^14: the
suites (tests/test_gfx_fractal_emu.py at 2^10, tests/test_gpu_gfx_fractal.py at both) compare against the recorded digests instead of calling it.

    python tools/make_gf64_fractal_digests.py [log_n ...]        # the sizes given, or all; entries of other sizes are kept"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

CASES = [(10, 0), (14, 0)]
SEED = 0x2205
RS_EXTRA, LOCALIZATION = 3, 2


def main():
    path = os.path.join(ROOT, "tests", "golden", "gf64_fractal.json")
    wanted = [int(a) for a in sys.argv[1:]] or [c[0] for c in CASES]
    entries = []
    if os.path.exists(path):
        with open(path) as f:
            entries = [e for e in json.load(f)["fractal"] if e["log_n"] not in wanted]
    for log_n, num_inputs in CASES:
        if log_n not in wanted:
            continue
        t0 = time.time()
        transcript, roots = oracle.fractal_prove(oracle.FIELD_GF64, log_n, num_inputs, SEED, rs_extra=RS_EXTRA, localization=LOCALIZATION)
        accepted = bool(oracle.fractal_verify(oracle.FIELD_GF64, log_n, num_inputs, SEED, transcript, roots, rs_extra=RS_EXTRA, localization=LOCALIZATION))
        flipped = bytearray(transcript)
        flipped[len(flipped) // 2] ^= 1
        rejected = not oracle.fractal_verify(oracle.FIELD_GF64, log_n, num_inputs, SEED, bytes(flipped), roots, rs_extra=RS_EXTRA, localization=LOCALIZATION)
        assert accepted and rejected
        entries.append({"field": "gf64", "log_n": log_n, "num_inputs": num_inputs, "seed": SEED, "rs_extra": RS_EXTRA, "localization": LOCALIZATION,
                        "bytes": len(transcript), "sha256": hashlib.sha256(transcript).hexdigest(), "index_roots": [bytes(r).hex() for r in roots],
                        "accepted": accepted, "rejected_with_a_flipped_bit": rejected})
        print("2^%d constraints: %d bytes, %.0f s" % (log_n, len(transcript), time.time() - t0), flush=True)
    entries.sort(key=lambda e: e["log_n"])
    with open(path, "w") as f:
        json.dump({"fractal": entries}, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
