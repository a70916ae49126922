"""Regenerates tests/golden/bn128_protocol_digests_large.json: whole-output BLAKE2b digests and 2^16-element chunk digests of the
protocol-layer recipes of tests/bn128_protocol_cases.py at m = 10, 12 and 22 over alt_bn128 Fr, computed by that module's integer
model (Python integers only).  The cases run in a few worker processes: m = 22 takes two to three minutes of CPU each.

    python tests/golden/make_bn128_protocol_digests_large.py [workers]"""
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bn128_protocol_cases as C  # noqa: E402

import numpy as np  # noqa: E402


def one(job):
    m, k = job
    c = C.large_cases(C.BN, m)[k]
    out = np.concatenate(C.model_words(C.BN, c, C.inputs(C.BN, c)))
    return c["name"], {"digest": C.digest(out), "chunks": C.chunk_digests(out) if m == 22 else []}


if __name__ == "__main__":
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    jobs = [(m, k) for m in (22, 12, 10) for k in range(len(C.large_cases(C.BN, m)))]
    with multiprocessing.Pool(workers) as pool:
        cases = dict(pool.imap_unordered(one, jobs))
    doc = {"field": "alt_bn128_Fr", "chunk_elements": 1 << 16, "cases": cases}
    with open(os.path.join(HERE, "bn128_protocol_digests_large.json"), "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
