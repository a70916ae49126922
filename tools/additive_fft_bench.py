#!/usr/bin/env python3
"""Times each device entry of the additive arm over GF(2^64), GF(2^128), GF(2^192) and GF(2^256) at the same m, in one process, the fields
alternating: the transforms at m = 22 full size, the 2^20 -> 2^25 LDE and the 2^25 IFFT, folds with cosets of 2 and 4 at m = 22, and a
7-oracle LDT combination at m = 22 (Aurora-like degree gaps).  Wall time per call from HIP events (torch.cuda.Event on the stream the library
uses) after warm-up; plans and tables are built during warm-up.  Per case and field: median, min and max over --reps, the launches that ran
and their algorithmic bytes, in total and by kernel, as counted by the library's own profile of one call (not a copy of the schedule), and the
total over the median as a share of 8 TB/s; the sub-millisecond cases time --calls calls per window.  --kernel-ms adds each kernel's summed
time in that one profiled call.  The yardstick of every other field is its gf192 twin in the same run; a comparison holds only when the two
ranges do not overlap:
    gf64_faster_beyond_spread                        the whole gf64 range lies below the gf192 range;
    gf128_below_gf192_beyond_spread                  the whole gf128 range lies below the gf192 range;
    gf256_above_four_thirds_of_gf192_beyond_spread   a gf256 element is 4/3 of the bytes: the whole gf256 range lies above 4/3 of the whole
                                                     gf192 range.
--set NAME=VALUE sets a library option (a tile geometry: IOPX_GF64_TILE_BITS, IOPX_GF128_P1_COLS, IOPX_GF256_P2_COLS, ...) before any plan
is built, and --fields / --cases narrow the run, for comparing neighbouring settings, one process per setting.  Kernel-only times: run this
under `rocprofv3 --kernel-trace --stats -- python tools/additive_fft_bench.py` in a separate run.

    python tools/additive_fft_bench.py [--reps 9] [--set IOPX_GF128_TILE_BITS=10] [--fields gf64,gf192] [--cases fft_2^22,ifft_2^22]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libiop_amd  # noqa: E402

WORDS = {"gf64": 1, "gf128": 2, "gf192": 3, "gf256": 4}
PREFIX = {"gf64": "k64_", "gf128": "k128_", "gf192": "k_", "gf256": "k256_"}
# the binding's method per entry: gf64 has methods of its own, gf128 and gf256 are the gf192 method with words=2 and words=4
GF64_METHOD = {"additive_FFT_dev": "additive_FFT_gf64_dev", "additive_IFFT_dev": "additive_IFFT_gf64_dev", "additive_LDE_dev": "additive_LDE_gf64_dev",
               "fri_fold_dev": "evaluate_next_f_i_over_entire_domain_gf64_dev", "ldt_combine_dev": "ldt_combine_gf64_dev"}


def launches_and_bytes(lib, fn, f):
    """One profiled call: (launches, algorithmic bytes, ms) by kernel as the library's own ProfScope counters report them — the schedule that
    actually ran, whatever the tile options are (the padding copy and the table reads are not in the byte count)."""
    lib.profile_begin()
    fn(f)
    rep = {k: v for k, v in lib.profile_report().items() if k.startswith(PREFIX[f])}
    return {k: v[0] for k, v in rep.items()}, {k: int(v[2]) for k, v in rep.items()}, {k: round(v[1], 4) for k, v in rep.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=8, help="calls per timed window for the sub-millisecond cases (folds, LDT combination)")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="a library option, set before any plan is built")
    ap.add_argument("--fields", default="gf64,gf128,gf192,gf256")
    ap.add_argument("--cases", default="")
    ap.add_argument("--kernel-ms", action="store_true", help="also print each kernel's summed time in the one profiled call (HIP events around every launch)")
    args = ap.parse_args()
    unknown = [f for f in args.fields.split(",") if f not in WORDS]
    if unknown:
        ap.error("unknown field(s) %s: any of %s" % (",".join(unknown), ",".join(WORDS)))
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    for s in args.set:
        name, value = s.split("=")
        lib.set_option(name, int(value))
    fields = [f for f in WORDS if f in args.fields.split(",")]
    rng = np.random.default_rng(7)
    big = 1 << 25
    buf, basis, shift, x = {}, {}, {}, {}
    for f in fields:
        w = WORDS[f]
        a = rng.integers(0, 1 << 63, size=(big, w), dtype=np.uint64)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        buf[f] = (t, torch.empty_like(t), [torch.empty(8 * w << 22, dtype=torch.uint8, device="cuda") for _ in range(7)])
        for m in (22, 25):
            b = np.zeros((m, w), dtype=np.uint64)
            b[:, 0] = [1 << i for i in range(m)]
            basis[(f, m)] = b
        shift[f] = np.array([1 << 40] + [0] * (w - 1), dtype=np.uint64)
        x[f] = rng.integers(0, 1 << 63, size=w, dtype=np.uint64)
    degrees = [1 << 21, (1 << 21) - 1, (1 << 21) - 1, 1 << 20, (1 << 21) - 1, (1 << 20) - 2, 1 << 21]
    coef = {f: rng.integers(0, 1 << 63, size=(14, WORDS[f]), dtype=np.uint64) for f in fields}

    def call(f, name):
        if f == "gf64":
            return getattr(lib, GF64_METHOD[name])
        method = getattr(lib, name)
        return method if f == "gf192" else (lambda *a: method(*a, words=WORDS[f]))

    def fft(f):
        call(f, "additive_FFT_dev")(buf[f][0].data_ptr(), 1 << 22, basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    def ifft(f):
        call(f, "additive_IFFT_dev")(buf[f][0].data_ptr(), basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    def lde(f):
        call(f, "additive_LDE_dev")(buf[f][0].data_ptr(), 1 << 20, basis[(f, 25)], shift[f], 0, 32, buf[f][1].data_ptr())

    def ifft25(f):
        call(f, "additive_IFFT_dev")(buf[f][0].data_ptr(), basis[(f, 25)], shift[f], buf[f][1].data_ptr())

    def fold(coset):
        def run(f):
            call(f, "fri_fold_dev")(buf[f][0].data_ptr(), basis[(f, 22)], shift[f], coset, x[f], buf[f][1].data_ptr())
        return run

    def ldt(f):
        ptrs = [t.data_ptr() for t in buf[f][2]]
        call(f, "ldt_combine_dev")(ptrs, degrees, coef[f], basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    cases = [("fft_2^22", fft, 1), ("ifft_2^22", ifft, 1), ("lde_2^20_to_2^25", lde, 1), ("ifft_2^25", ifft25, 1),
             ("fold_coset2_2^22", fold(2), args.calls), ("fold_coset4_2^22", fold(4), args.calls), ("ldt_combine_7_2^22", ldt, args.calls)]
    if args.cases:
        cases = [c for c in cases if c[0] in args.cases.split(",")]
    times = {(k, f): [] for k, _, _ in cases for f in fields}
    for _ in range(args.warmup):
        for _, fn, _ in cases:
            for f in fields:
                fn(f)
    torch.cuda.synchronize()
    sched = {(k, f): launches_and_bytes(lib, fn, f) for k, fn, _ in cases for f in fields}
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn, calls in cases:
            for f in fields:                           # the fields alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn(f)
                e1.record()
                e1.synchronize()
                times[(k, f)].append(e0.elapsed_time(e1) / calls)
    for k, _, calls in cases:
        row = {"case": k, "calls_per_window": calls, "options": args.set}
        for f in fields:
            t = sorted(times[(k, f)])
            launches, kernel_bytes, kernel_ms = sched[(k, f)]
            nbytes = sum(kernel_bytes.values())
            med = statistics.median(t)
            row[f] = {"median_ms": round(med, 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "launches": launches, "bytes": nbytes,
                      "kernel_bytes": kernel_bytes, "hbm_share_of_8TBps": round(nbytes / (med * 1e-3) / 8e12, 3)}
            if args.kernel_ms:
                row[f]["kernel_ms"] = kernel_ms
        if "gf192" in row:
            for f in fields:
                if f != "gf192":
                    row["ratio_%s_over_gf192" % f] = round(row[f]["median_ms"] / row["gf192"]["median_ms"], 3)
            # each comparison holds only when the two ranges do not overlap
            if "gf64" in row:
                row["gf64_faster_beyond_spread"] = row["gf64"]["max_ms"] < row["gf192"]["min_ms"]
            if "gf128" in row:
                row["gf128_below_gf192_beyond_spread"] = row["gf128"]["max_ms"] < row["gf192"]["min_ms"]
            if "gf256" in row:
                row["gf256_above_four_thirds_of_gf192_beyond_spread"] = row["gf256"]["min_ms"] > 4.0 / 3.0 * row["gf192"]["max_ms"]
        print(json.dumps(row), flush=True)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
