#!/usr/bin/env python3
"""Times the seventeen alt_bn128 Fr protocol-layer entries (iopx_*_bn128_dev) against their edwards_Fr twins (iopx_*_fp3_dev) on the same
shapes, in one process, the two fields alternating: every entry at 2^25 elements (the Aurora 2^20 / RS_extra_dimensions 5 codeword), SpMV on
2^20 rows of the synthetic instance's shape.  Wall time per call from HIP events (torch.cuda.Event on the stream the library uses) after
warm-up, median of --reps.  Per entry: ms for both fields, their ratio, the vectors read and written per element and the algorithmic bytes
over time as a share of 8 TB/s.  Kernel-only times: `rocprofv3 --kernel-trace --stats -- python tools/bn128_protocol_bench.py --reps 3`
in a run of its own.  The cases and the C calls are those of tests/bn128_protocol_cases.py (the recipes the tests check).

    python tools/bn128_protocol_bench.py [--reps 9] [--log-n 25]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libiop_amd  # noqa: E402
import bn128_protocol_cases as C  # noqa: E402

# vectors of n elements an entry reads and writes.  SpMV is not in this table: its bytes are counted from the matrix (per entry one
# coefficient, one gathered vector element and a 4-byte column; per row one output element and an 8-byte offset)
VECTORS = {"rowcheck": 4, "fz": 3, "sumcheck_g": 3, "lincheck": 7, "lincomb": 7, "lincomb_affine": 4, "rational_combine": 8, "poly_div_vanishing": 2,
           "mul": 3, "sub": 3, "inv": 2, "div": 5, "pow_table": 1, "domain_offsets": 1, "vanishing_evals": 1, "rational_sumcheck_constraint": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=25)
    args = ap.parse_args()
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    m, n = args.log_n, 1 << args.log_n
    fields = [("bn128", C.BN), ("edwards", C.ED)]
    rng = np.random.default_rng(7)
    plans = {}
    for name, F in fields:
        pool = []
        for _ in range(8):                  # canonical in both fields (top word below 2^52)
            a = rng.integers(0, 1 << 62, size=(n, F.words), dtype=np.uint64)
            a[:, -1] &= np.uint64((1 << 52) - 1)
            pool.append(torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda())
        outs = [torch.empty_like(pool[0]), torch.empty_like(pool[0])]
        keep = [pool, outs]
        for case in C.large_cases(F, m):
            nnz = 0
            if case["op"] == "spmv":
                case = dict(case, rows=1 << max(m - 5, 5), accumulate=0)
                inp = C.inputs(F, case)
                d = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda() for k, v in inp.items() if k != "out"}
                keep.append(d)
                d = {k: t.data_ptr() for k, t in d.items()}
                nnz = int(inp["row_ptr"][-1])
            else:
                roles = ["a", "b", "c"] + ["m%d" % i for i in range(8)] + ["n%d" % i for i in range(4)] + ["d%d" % i for i in range(4)]
                d = {r: pool[i % len(pool)].data_ptr() for i, r in enumerate(roles)}
            plans[(case["name"], name)] = (F, case, d, [o.data_ptr() for o in outs], nnz)
        plans[("__keep__", name)] = keep
    names = [c["name"] for c in C.large_cases(C.BN, m)]

    def run(key):
        F, case, d, d_outs, _ = plans[key]
        lib._check(C.call(lib, F, case, d, d_outs))

    times = {(k, f): [] for k in names for f, _ in fields}
    for _ in range(args.warmup):
        for k in names:
            for f, _ in fields:
                run((k, f))
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k in names:
            for f, _ in fields:                        # the two fields alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run((k, f))
                e1.record()
                e1.synchronize()
                times[(k, f)].append(e0.elapsed_time(e1))
    for k in names:
        row = {"case": k}
        for f, F in fields:
            _, case, _, _, nnz = plans[(k, f)]
            ms = statistics.median(times[(k, f)])
            count, s = C.out_count(case), 8 * F.words
            nbytes = nnz * (2 * s + 4) + count * (s + 8) if case["op"] == "spmv" else VECTORS[case["op"]] * count * s
            row[f] = {"ms": round(ms, 3), "bytes_per_element": round(nbytes / count, 1), "hbm_share_of_8TBps": round(nbytes / (ms * 1e-3) / 8e12, 3)}
        row["ratio_bn128_over_edwards"] = round(row["bn128"]["ms"] / row["edwards"]["ms"], 2)
        print(json.dumps(row), flush=True)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
