#!/usr/bin/env python3
"""Writes tests/golden/gfx_fractal_wide.json: the index roots and SHA-256 and length of the Fractal transcript over GF(2^128) and GF(2^256) at
2^10 constraints and 15 inputs, seed 0x2205, rate 3, localization 2, with the model's run time.  The bytes are those of
tests/gfx_fractal_model.py, the restated indexer and prover over the oracle's building blocks, on the CPU, with its degree check on (a satisfied
instance passes it); both suites prove the same instance natively and compare digests.  Beside it the hand-built system of
tests/gfx_fractal_wide_cases.py at two and four words, with its satisfied and its flipped assignment and the degree check's verdict on each: the
MI355X suite compares the native prover with these digests, and the CPU suite, where the model runs, holds the digests to the model.

Before anything is written the model is held to the oracle's own prover at this very tuple, at one and at three words (gf64 and gf192, fields
oracle.fractal_prove knows): index roots and transcript, byte equality.  The file records the two digests that were compared.

    python tools/make_gfx_fractal_wide_digests.py [--log-n 10]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gfx_fractal_model as FM    # noqa: E402
import gfx_fractal_wide_cases as FW  # noqa: E402
import oracle                     # noqa: E402

SEED, INPUTS, RS_EXTRA, LOCALIZATION = 0x2205, 15, 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=10)
    args = ap.parse_args()
    trust = []
    for words, name, ofield in ((1, "gf64", oracle.FIELD_GF64), (3, "gf192", oracle.FIELD_GF192)):
        mine, roots, _ = FM.prove_example(words, args.log_n, INPUTS, SEED, RS_EXTRA, LOCALIZATION)
        ref, ref_roots = oracle.fractal_prove(ofield, args.log_n, INPUTS, SEED, rs_extra=RS_EXTRA, localization=LOCALIZATION)
        if mine != ref or roots != ref_roots:
            sys.exit("the model differs from oracle.fractal_prove over %s at 2^%d: nothing written" % (name, args.log_n))
        trust.append({"field": name, "words": words, "bytes": len(ref), "sha256": hashlib.sha256(ref).hexdigest()})
        print("%s 2^%d: the model equals the oracle's indexer and prover (%d bytes)" % (name, args.log_n, len(ref)), flush=True)
    entries = []
    for words, name in ((2, "gf128"), (4, "gf256")):
        t0 = time.time()
        stats = {}
        transcript, roots, _ = FM.prove_example(words, args.log_n, INPUTS, SEED, RS_EXTRA, LOCALIZATION, check_degrees=True, stats=stats)
        seconds = time.time() - t0
        entries.append({"field": name, "log_n": args.log_n, "num_inputs": INPUTS, "seed": SEED, "rs_extra": RS_EXTRA, "localization": LOCALIZATION,
                        "codeword_domain_dim": stats["parameters"]["codeword_domain_dim"], "index_roots": [r.hex() for r in roots],
                        "bytes": len(transcript), "sha256": hashlib.sha256(transcript).hexdigest(), "model_seconds": round(seconds, 1)})
        print("%s 2^%d: %d bytes, %.0f s" % (name, args.log_n, len(transcript), seconds), flush=True)
    hand = []
    for words, name in ((2, "gf128"), (4, "gf256")):
        system, rs_extra, loc, roots, runs = FW.hand_built_model(words)
        hand.append({"field": name, "rs_extra": rs_extra, "localization": loc, "index_roots": [r.hex() for r in roots],
                     "assignments": {k: {"bytes": len(t), "sha256": hashlib.sha256(t).hexdigest(), "degrees_hold": ok} for k, (_, t, ok) in runs.items()}})
        print("%s hand-built: %s" % (name, {k: v["degrees_hold"] for k, v in hand[-1]["assignments"].items()}), flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "gfx_fractal_wide.json"), "w") as f:
        json.dump({"generated_by": "tools/make_gfx_fractal_wide_digests.py", "source": "tests/gfx_fractal_model.py over the oracle's building blocks",
                   "model_equals_oracle_prover_at_this_tuple": trust, "fractal": entries, "hand_built": hand}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
