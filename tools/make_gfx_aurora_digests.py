#!/usr/bin/env python3
"""Writes tests/golden/gfx_aurora.json: SHA-256 and length of the Aurora transcript over GF(2^128) and GF(2^256) at 2^12 constraints and 15
inputs (a codeword of 2^17 points: many tiles of the transform), seed 0x2204, default rate and localization.  The bytes are those of
tests/gfx_aurora_model.py, the restated prover over the oracle's building blocks, on the CPU (about half a minute per field); both suites
prove the same instance natively, and the GPU suite through the Python prover too, and compare digests.

Before anything is written the model is held to the oracle's own prover at this very tuple, at one and at three words (gf64 and gf192, the
fields oracle.aurora_prove knows): byte equality, about 40 s per width — too long for the suite, whose trust test stops at 2^9.  The file
records the two digests that were compared.

    python tools/make_gfx_aurora_digests.py [--log-n 12]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gfx_aurora_model as M      # noqa: E402
import oracle                     # noqa: E402

SEED, INPUTS = 0x2204, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=12)
    args = ap.parse_args()
    trust = []
    for words, name, ofield in ((1, "gf64", oracle.FIELD_GF64), (3, "gf192", oracle.FIELD_GF192)):
        mine, ref = M.prove_example(words, args.log_n, INPUTS, SEED)[0], oracle.aurora_prove(ofield, args.log_n, INPUTS, SEED)
        if mine != ref:
            sys.exit("the model differs from oracle.aurora_prove over %s at 2^%d: nothing written" % (name, args.log_n))
        trust.append({"field": name, "words": words, "bytes": len(ref), "sha256": hashlib.sha256(ref).hexdigest()})
        print("%s 2^%d: the model equals the oracle's prover (%d bytes)" % (name, args.log_n, len(ref)))
    entries = []
    for words, name in ((2, "gf128"), (4, "gf256")):
        t0 = time.time()
        transcript, P, _ = M.prove_example(words, args.log_n, INPUTS, SEED)
        entries.append({"field": name, "log_n": args.log_n, "num_inputs": INPUTS, "seed": SEED, "rs_extra": 5, "localization": 2,
                        "codeword_domain_dim": P["codeword_domain_dim"], "bytes": len(transcript), "sha256": hashlib.sha256(transcript).hexdigest()})
        print("%s 2^%d: %d bytes, %.0f s" % (name, args.log_n, len(transcript), time.time() - t0))
    with open(os.path.join(ROOT, "tests", "golden", "gfx_aurora.json"), "w") as f:
        json.dump({"generated_by": "tools/make_gfx_aurora_digests.py", "source": "tests/gfx_aurora_model.py over the oracle's building blocks",
                   "model_equals_oracle_prover_at_this_tuple": trust, "aurora": entries}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
