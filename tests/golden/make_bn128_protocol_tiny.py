"""Regenerates tests/golden/bn128_protocol_tiny.json: the digest of every tiny case of tests/bn128_protocol_cases.py over alt_bn128 Fr,
computed by that module's integer model (Python integers only; no library of this repository is called).

    python tests/golden/make_bn128_protocol_tiny.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bn128_protocol_cases as C  # noqa: E402

if __name__ == "__main__":
    doc = {"field": "alt_bn128_Fr", "what": "BLAKE2b-256 of the output words (numerator then denominator for rational_combine) of each tiny case",
           "cases": C.model_tiny(C.BN)}
    with open(os.path.join(HERE, "bn128_protocol_tiny.json"), "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(doc["cases"]), "cases")
