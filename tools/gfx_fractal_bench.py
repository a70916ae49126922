#!/usr/bin/env python3
"""Times the native Fractal prover (iopx_fractal_index / iopx_fractal_prove) over gf64 under IOPX_GFX_FRACTAL=1 next to gf192's in one process on
cuda:0, at 2^16 and 2^20 constraints (no inputs, seed 0x2205, rate 3, localization 2), and gives the library's per-kernel profile of one gf64 proof
per size.  The protocol is tools/gfx_aurora_bench.py's.

Per size: one seeded instance per field, the index (timed once, with the one-time work of a first call in it), iopx_aurora_instance_warm(protocol 1)
and two untimed proofs, then --reps timed proofs (host clock around a proof that ends in a device synchronise), gf64 and gf192 alternating proof by
proof so that they see the same neighbours; median, minimum, maximum and the spread (max - min over the median) are reported, and a second index
build (warm) beside the first.  The profile is taken in a proof of its own, after the timed ones.  With --div, the batch division alone
(iopx_FIELD_div_dev at 2^22 elements over gf64, gf128 and gf256) with the workgroup's root inverted by the Fermat power and by the binary Euclid
(IOPX_GFX_DIV_INVERSION = 1 / 2), seven alternating repetitions, from the profile's milliseconds.  A run without a GPU fails.

    python tools/gfx_fractal_bench.py [--log-n 16 20] [--reps 7] [--div] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import libiop_amd  # noqa: E402

SEED = 0x2205
RS_EXTRA, LOCALIZATION = 3, 2
CODES = {"gf64": libiop_amd.FIELD_GF64, "gf192": libiop_amd.FIELD_GF192}
STEMS = {1: "k64_", 2: "k128_", 4: "k256_"}


def summary(ms):
    s = sorted(ms)
    med = statistics.median(s)
    return {"median": round(med, 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round((s[-1] - s[0]) / med, 4), "all": [round(x, 4) for x in ms]}


def bench_div(lib, reps, log_count=22):
    """k*_div alone: both inversions alternating, milliseconds from the library's profile (HIP events around the launch)"""
    n = 1 << log_count
    out = []
    rng = np.random.Generator(np.random.PCG64(5))
    for W in (1, 2, 4):
        den = rng.integers(1, 1 << 64, size=(n, W), dtype=np.uint64)
        d_den, d_num, d_out = lib.malloc(8 * W * n), lib.malloc(8 * W * n), lib.malloc(8 * W * n)
        try:
            lib.h2d(d_den, den)
            lib.h2d(d_num, den[::-1].copy())
            times = {1: [], 2: []}
            for rep in range(reps + 1):                     # the first round is untimed
                for way in (1, 2):
                    lib.set_option("IOPX_GFX_DIV_INVERSION", way)
                    lib.profile_begin()
                    lib.field_div_dev(d_num, d_den, d_out, n, words=W)
                    prof = lib.profile_report()
                    if rep:
                        times[way].append(prof[STEMS[W] + "div"][1])
            lib.clear_option("IOPX_GFX_DIV_INVERSION")
            entry = {"bench": "div", "words": W, "elements": n, "fermat_ms": summary(times[1]), "euclid_ms": summary(times[2]),
                     "declared_bytes": 6 * n * 8 * W}
            out.append(entry)
            print(json.dumps(entry), flush=True)
        finally:
            for p in (d_den, d_num, d_out):
                lib.free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--div", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gfx_fractal_bench: no GPU (timings are taken on the device only)")
    lib = libiop_amd.lib()
    lib.init(0)
    lib.set_option("IOPX_GFX_FRACTAL", 1)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    results = []

    def save():
        if a.out:                                           # after every entry: a later size that runs out of time loses nothing
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    if a.div:
        results += bench_div(lib, a.reps)
        save()
    for log_n in a.log_n:
        n = 1 << log_n
        names = ("gf64", "gf192")
        insts = {name: lib.aurora_example_instance(CODES[name], n, 0, n - 1, SEED) for name in names}
        try:
            proofs, times, index_ms = {}, {name: [] for name in names}, {}
            for name in names:
                index_ms[name] = []
                for _ in range(2):                          # the first with the one-time work of a first call, the second warm
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lib.fractal_index(insts[name], 128, RS_EXTRA, LOCALIZATION)
                    torch.cuda.synchronize()
                    index_ms[name].append(round((time.perf_counter() - t0) * 1e3, 3))
                lib.aurora_instance_warm(insts[name], fractal=True, RS_extra_dimensions=RS_EXTRA, FRI_localization_parameter=LOCALIZATION)
                for _ in range(2):
                    proofs[name] = lib.fractal_prove(insts[name], 128, RS_EXTRA, LOCALIZATION)
            for _ in range(a.reps):
                for name in names:                          # alternating: both fields under the same conditions
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    t = lib.fractal_prove(insts[name], 128, RS_EXTRA, LOCALIZATION)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3)
                    assert t == proofs[name], "the transcript changed between two proofs of the same instance"
            lib.profile_begin()
            lib.fractal_prove(insts["gf64"], 128, RS_EXTRA, LOCALIZATION)
            prof = lib.profile_report()
            entry = {"bench": "fractal", "log_n": log_n}
            for name in names:
                entry[name] = {"prover_ms": summary(times[name]), "index_ms_first_then_warm": index_ms[name], "argument_bytes": len(proofs[name]),
                               "transcript_sha256": hashlib.sha256(proofs[name]).hexdigest()}
            entry["gf64_over_gf192"] = round(entry["gf64"]["prover_ms"]["median"] / entry["gf192"]["prover_ms"]["median"], 4)
            entry["kernels_ms_total"] = round(sum(v[1] for v in prof.values()), 3)
            entry["kernels"] = {k: {"launches": v[0], "ms": round(v[1], 4), "declared_bytes": int(v[2]),
                                    "GB_per_s": round(v[2] / v[1] / 1e6, 1) if v[1] > 0 and v[2] > 0 else None}
                                for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
            results.append(entry)
            print(json.dumps(entry), flush=True)
        finally:
            for inst in insts.values():
                lib.aurora_instance_free(inst)
        save()


if __name__ == "__main__":
    main()
