#!/usr/bin/env python3
"""Times the native Aurora prover (iopx_aurora_prove) over gf64 and over gf192 in one process on cuda:0, at 2^16 and 2^20 constraints
(15 inputs, seed 0x2204, default rate and localization), and gives the library's per-kernel profile of one gf64 proof per size.

Per field and size: one instance, iopx_aurora_instance_warm and two untimed proofs, then --reps timed proofs (host clock around a proof that
ends in a device synchronise), the two fields alternating proof by proof so that they see the same neighbours; median, minimum, maximum and
the spread (max - min over the median) are reported.  The profile is taken in a proof of its own, after the timed ones: per kernel the
launches, the milliseconds, the bytes its launches declared and the rate those give.  A run without a GPU fails.

    python tools/gf64_aurora_bench.py [--log-n 16 20] [--reps 7] [--head-eval {0,1}] [--out FILE]

--head-eval sets the option IOPX_GFX_HEAD_EVAL through iopx_set_option before the first proof (1: head evaluation over the subspace-only fields; left
unset without the flag: the library's default, 0).  gf192's schedule does not read it."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import libiop_amd  # noqa: E402

SEED = 0x2204
FIELDS = (("gf64", libiop_amd.FIELD_GF64), ("gf192", libiop_amd.FIELD_GF192))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--head-eval", type=int, choices=(0, 1), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gf64_aurora_bench: no GPU (timings are taken on the device only)")
    lib = libiop_amd.lib()
    lib.init(0)
    if a.head_eval is not None:
        lib.set_option("IOPX_GFX_HEAD_EVAL", a.head_eval)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    results = []
    for log_n in a.log_n:
        n = 1 << log_n
        insts = {name: lib.aurora_example_instance(code, n, 15, n - 1, SEED) for name, code in FIELDS}
        try:
            proofs, times = {}, {name: [] for name, _ in FIELDS}
            for name, _ in FIELDS:
                lib.aurora_instance_warm(insts[name])
                for _ in range(2):
                    proofs[name] = lib.aurora_prove(insts[name])
            for _ in range(a.reps):
                for name, _ in FIELDS:                 # alternating: both fields under the same conditions
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    t = lib.aurora_prove(insts[name])
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                    assert t == proofs[name], "the transcript changed between two proofs of the same instance"
            lib.profile_begin()
            lib.aurora_prove(insts["gf64"])
            prof = lib.profile_report()
            entry = {"log_n": log_n, "head_eval": a.head_eval}
            for name, _ in FIELDS:
                ms = sorted(times[name])
                med = statistics.median(ms)
                entry[name] = {"prover_ms_median": round(med, 3), "prover_ms_min": round(ms[0], 3), "prover_ms_max": round(ms[-1], 3),
                               "spread": round((ms[-1] - ms[0]) / med, 4), "prover_ms": [round(x, 3) for x in times[name]], "argument_bytes": len(proofs[name]),
                               "transcript_sha256": hashlib.sha256(proofs[name]).hexdigest()}
            entry["gf64_over_gf192"] = round(entry["gf64"]["prover_ms_median"] / entry["gf192"]["prover_ms_median"], 4)
            entry["gf64_kernels_ms_total"] = round(sum(v[1] for v in prof.values()), 3)
            entry["gf64_kernels"] = {k: {"launches": v[0], "ms": round(v[1], 4), "declared_bytes": int(v[2]),
                                         "GB_per_s": round(v[2] / v[1] / 1e6, 1) if v[1] > 0 and v[2] > 0 else None}
                                     for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
            results.append(entry)
            print(json.dumps(entry), flush=True)
        finally:
            for inst in insts.values():
                lib.aurora_instance_free(inst)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
