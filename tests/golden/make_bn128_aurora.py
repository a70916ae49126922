"""Writes tests/golden/bn128_aurora.json from the Python-integer model (tests/bn128_aurora_model.py): the BLAKE2b-256 digest and the byte length of
the Aurora transcript over alt_bn128 Fr for each small parameter tuple x the three hash families, and for the GPU suite's larger tuple with
BLAKE2b and starkware Poseidon.  Needs the oracle library (Poseidon permutation, trees, grind); run from the repository root:
    python tests/golden/make_bn128_aurora.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bn128_aurora_cases as C          # noqa: E402
import bn128_aurora_model as M          # noqa: E402


def main():
    out = {"comment": "written by tests/golden/make_bn128_aurora.py; keys: log_n_inputs_rs_loc/hash", "seed": C.SEED, "digests": {}}
    for tup, hashes in [(t, list(C.HASHES)) for t in C.TUPLES] + [(C.GPU_TUPLE, C.GPU_HASHES)]:
        for h in hashes:
            out["digests"][C.key(tup, h)] = C.digest(M.prove_example(M.ALT_BN128_FR, C.HASHES[h], *tup, C.SEED))
    with open(C.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
