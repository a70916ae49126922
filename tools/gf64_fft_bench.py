#!/usr/bin/env python3
"""Times each GF(2^64) device entry against its GF(2^192) twin at the same m, in one process, alternating the two fields: the transforms at
m = 22 full size, the 2^20 -> 2^25 LDE and the 2^25 IFFT, folds with cosets of 2 and 4 at m = 22, and a 7-oracle LDT combination at m = 22
(Aurora-like degree gaps).  Wall time per call from HIP events (torch.cuda.Event on the stream the library uses) after warm-up, median of
--reps; plans and tables are built during warm-up.  Per case: ms of both fields, the ratio, and for gf64 the algorithmic bytes (8 bytes per
element read and written per HBM pass, as counted by the library's own profile of one call: the launches that ran, not a copy of the
schedule) over time as a share of 8 TB/s, median with min and max over the repetitions; the sub-millisecond cases time --calls calls per
window.  Kernel-only times: run this under `rocprofv3 --kernel-trace --stats
-- python tools/gf64_fft_bench.py` in a separate run.

    python tools/gf64_fft_bench.py [--reps 9]
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


def launches_and_bytes(lib, fn):
    """One profiled call: (k64_* launches by kernel, their algorithmic bytes) as the library's own ProfScope counters report them — the
    schedule that actually ran, whatever the tile options are (the padding copy and the table reads are not in the byte count)."""
    lib.profile_begin()
    fn("gf64")
    rep = lib.profile_report()
    k64 = {k: v for k, v in rep.items() if k.startswith("k64_")}
    return {k: v[0] for k, v in k64.items()}, sum(v[2] for v in k64.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=8, help="calls per timed window for the sub-millisecond cases (folds, LDT combination)")
    args = ap.parse_args()
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    big = 1 << 25
    words = {"gf64": 1, "gf192": 3}
    buf, basis, shift, x = {}, {}, {}, {}
    for f, w in words.items():
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
    coef = {f: rng.integers(0, 1 << 63, size=(14, w), dtype=np.uint64) for f, w in words.items()}

    def call(f, name64, name192):
        return getattr(lib, name64 if f == "gf64" else name192)

    def fft(f):
        call(f, "additive_FFT_gf64_dev", "additive_FFT_dev")(buf[f][0].data_ptr(), 1 << 22, basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    def ifft(f):
        call(f, "additive_IFFT_gf64_dev", "additive_IFFT_dev")(buf[f][0].data_ptr(), basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    def lde(f):
        call(f, "additive_LDE_gf64_dev", "additive_LDE_dev")(buf[f][0].data_ptr(), 1 << 20, basis[(f, 25)], shift[f], 0, 32, buf[f][1].data_ptr())

    def ifft25(f):
        call(f, "additive_IFFT_gf64_dev", "additive_IFFT_dev")(buf[f][0].data_ptr(), basis[(f, 25)], shift[f], buf[f][1].data_ptr())

    def fold(coset):
        def run(f):
            call(f, "evaluate_next_f_i_over_entire_domain_gf64_dev", "fri_fold_dev")(buf[f][0].data_ptr(), basis[(f, 22)], shift[f], coset, x[f],
                                                                                     buf[f][1].data_ptr())
        return run

    def ldt(f):
        ptrs = [t.data_ptr() for t in buf[f][2]]
        call(f, "ldt_combine_gf64_dev", "ldt_combine_dev")(ptrs, degrees, coef[f], basis[(f, 22)], shift[f], buf[f][1].data_ptr())

    cases = [("fft_2^22", fft, 1), ("ifft_2^22", ifft, 1), ("lde_2^20_to_2^25", lde, 1), ("ifft_2^25", ifft25, 1),
             ("fold_coset2_2^22", fold(2), args.calls), ("fold_coset4_2^22", fold(4), args.calls), ("ldt_combine_7_2^22", ldt, args.calls)]
    times = {(k, f): [] for k, _, _ in cases for f in words}
    for _ in range(args.warmup):
        for _, fn, _ in cases:
            for f in words:
                fn(f)
    torch.cuda.synchronize()
    sched = {k: launches_and_bytes(lib, fn) for k, fn, _ in cases}
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn, calls in cases:
            for f in words:                            # the two fields alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn(f)
                e1.record()
                e1.synchronize()
                times[(k, f)].append(e0.elapsed_time(e1) / calls)
    for k, _, calls in cases:
        row = {"case": k, "calls_per_window": calls}
        for f in words:
            t = sorted(times[(k, f)])
            row[f] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}
        row["ratio_gf64_over_gf192"] = round(row["gf64"]["median_ms"] / row["gf192"]["median_ms"], 3)
        # the comparison holds only when the two ranges do not overlap
        row["gf64_faster_beyond_spread"] = row["gf64"]["max_ms"] < row["gf192"]["min_ms"]
        launches, nbytes = sched[k]
        row["gf64_launches"] = launches
        row["gf64_hbm_share_of_8TBps"] = round(nbytes / (row["gf64"]["median_ms"] * 1e-3) / 8e12, 3)
        print(json.dumps(row), flush=True)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
