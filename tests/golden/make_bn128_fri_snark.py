"""Writes tests/golden/bn128_fri_snark.json from the Python-integer model (tests/bn128_fri_snark_model.py): full transcripts of the FRI-only
SNARK over alt_bn128 Fr for the small parameter tuples x the three hash families, the two short-coefficient cases, and BLAKE2b digests of
the dim-16 transcripts.  Needs the oracle library (Poseidon permutation, trees, grind); run from the repository root:
    python tests/golden/make_bn128_fri_snark.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bn128_fri_snark_cases as C          # noqa: E402
import bn128_fri_snark_model as M          # noqa: E402


def model(tup, hash_name, n_coeffs=None):
    dim, rs_extra = tup[0], tup[1]
    n = (1 << (dim - rs_extra)) if n_coeffs is None else n_coeffs
    return M.prove(M.ALT_BN128_FR, C.HASHES[hash_name], *tup, coeffs=C.seeded(C.SEED, n))


def main():
    out = {"comment": "written by tests/golden/make_bn128_fri_snark.py; keys: dim_rs_loc_interactions_queries/hash[/n<coefficients>]", "seed": C.SEED,
           "transcripts": {}, "digests": {}}
    for tup in C.TUPLES:
        for h in C.HASHES:
            out["transcripts"][C.key(tup, h)] = model(tup, h).hex()
    bound = 1 << (C.SHORT_TUPLE[0] - C.SHORT_TUPLE[1])
    for h in ("blake2b", "poseidon_starkware"):
        for n in (1, bound - 1):
            out["transcripts"][C.key(C.SHORT_TUPLE, h, n)] = model(C.SHORT_TUPLE, h, n).hex()
    for h in C.HASHES:
        t = model(C.LARGE_TUPLE, h)
        out["digests"][C.key(C.LARGE_TUPLE, h)] = {"bytes": len(t), "blake2b": hashlib.blake2b(t, digest_size=32).hexdigest()}
    with open(C.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
