"""Writes tests/golden/oracle_function_digests_large.json: digests of the oracle's outputs for the recipes of tests/fullsize_cases.py, at
BASELINE config 2 / 3's full size (m = 22) and at the small sizes the CPU-build tests run.  Only the oracle runs here; every entry records
the seconds its oracle calls took.  Usage: python tests/golden/make_oracle_function_digests_large.py [--jobs N] (one process per entry)."""
import argparse
import hashlib
import json
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import fullsize_cases as fc          # noqa: E402


def entry(task):
    m, key, log_chunk = task
    t0 = time.time()
    if key.startswith("fri_snark"):
        data = fc.oracle_snark(key)
        out = {"transcript_blake2b": hashlib.blake2b(data, digest_size=32).hexdigest(), "argument_bytes": len(data)}
    elif key.startswith("fold_chain"):
        words = fc.oracle_fold_chain(key, m)
        out = dict(fc.record(words[0], log_chunk), folds=[fc.record(w, log_chunk) for w in words[1:]])
    else:
        out = fc.record(fc.oracle_transform(key, m), log_chunk)
    out["oracle_seconds"] = round(time.time() - t0, 1)
    print("%-40s %8.1f s" % (key, out["oracle_seconds"]), flush=True)
    return m, key, out


def tasks():
    out = [(fc.LARGE_M, k, fc.LARGE_LOG_CHUNK) for k in fc.keys(fc.LARGE_M)]
    for m in fc.SMALL_MS:
        out += [(m, k, fc.SMALL_LOG_CHUNK) for k in fc.keys(m) if not k.startswith("fri_snark") or m == fc.SMALL_DIM]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=os.cpu_count())
    ap.add_argument("--out", default=fc.FIXTURE)
    args = ap.parse_args()
    t0 = time.time()
    with Pool(args.jobs) as pool:
        results = pool.map(entry, sorted(tasks(), key=lambda t: -t[0]), chunksize=1)
    doc = {
        "what": "BLAKE2b-256 of the oracle's outputs for the recipes of tests/fullsize_cases.py: the additive FFT / IFFT, the FRI fold chains "
                "(the LDE codeword, then the word after every fold) and the FRI SNARK transcripts, at BASELINE configs 2 / 3's size (m = 22) and at "
                "small sizes for the CPU-build tests. Arrays hash as (n, 3) little-endian uint64, row-major; 'chunks' hash 2^log_chunk consecutive "
                "elements each. oracle_seconds: one host core per entry.",
        "generator": "tests/golden/make_oracle_function_digests_large.py",
        "large": {"m": fc.LARGE_M, "log_chunk": fc.LARGE_LOG_CHUNK, "entries": {}},
        "small": {"log_chunk": fc.SMALL_LOG_CHUNK, "sizes": {str(m): {} for m in fc.SMALL_MS}},
    }
    for m, key, out in results:
        (doc["large"]["entries"] if m == fc.LARGE_M else doc["small"]["sizes"][str(m)])[key] = out
    doc["oracle_seconds_total"] = round(sum(out["oracle_seconds"] for _, _, out in results), 1)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("oracle seconds, one core: %.1f; wall %.1f s with %d jobs" % (doc["oracle_seconds_total"], time.time() - t0, args.jobs))


if __name__ == "__main__":
    main()
