#!/usr/bin/env python3
"""Times the FRI-only SNARK over alt_bn128 Fr (BLAKE2b and starkware Poseidon) beside the edwards_Fr / BLAKE2b one, and the fixed-shape BLAKE2b leaf
kernel for 32-byte elements (k_merkle_leaves_sub32) against the general kernel on the same shapes — one process, the cases alternating.  Wall time
per call from HIP events (torch.cuda.Event on the stream the library uses), two warm-up rounds, median of --reps; "spread" is (max - min) / median of
the repetitions, the run-to-run spread a difference has to exceed to count.  Kernel-only times: a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bn128_fri_bench.py`.

    python tools/bn128_fri_bench.py [--reps 9] [--dim 22]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libiop_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dim", type=int, default=22)
    args = ap.parse_args()
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)

    def device_words(n, words):
        a = rng.integers(0, 1 << 62, size=(n, words), dtype=np.uint64)       # below both moduli: canonical mont_repr
        a[:, -1] &= np.uint64((1 << 52) - 1)
        return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()

    dim, rs, loc, interactions, queries = args.dim, 2, 2, 1, 10
    bound = 1 << (dim - rs)
    coeffs = {4: device_words(bound, 4), 3: device_words(bound, 3)}

    def prover(field, words, h):
        return lambda: lib.fri_snark_prove(field, coeffs[words].data_ptr(), bound, dim, rs, loc, interactions, queries, hash=h)

    def leaves(n, num_oracles, cs, sub32):
        oracles = [device_words(n, 4) for _ in range(num_oracles)]
        nodes = torch.empty((2 * (n // cs) - 1) * 32, dtype=torch.uint8, device="cuda")

        def run():
            if not sub32:
                lib.set_option("IOPX_LEAVES_SUB32", 0)
            try:
                lib.merkle_leaves_dev([o.data_ptr() for o in oracles], 32, n, cs, nodes.data_ptr(), libiop_amd.DOMAIN_MULTIPLICATIVE)
            finally:
                if not sub32:
                    lib.clear_option("IOPX_LEAVES_SUB32")
        return run

    cases = [("fri_snark alt_bn128_Fr blake2b", prover(libiop_amd.FIELD_ALT_BN128_FR, 4, libiop_amd.HASH_BLAKE2B)),
             ("fri_snark alt_bn128_Fr poseidon_starkware", prover(libiop_amd.FIELD_ALT_BN128_FR, 4, libiop_amd.HASH_POSEIDON_STARKWARE)),
             ("fri_snark edwards_Fr blake2b", prover(libiop_amd.FIELD_EDWARDS_FR, 3, None))]
    for n, num_oracles, cs in ((1 << 22, 1, 4), (1 << 20, 4, 2)):
        for sub32 in (True, False):
            cases.append(("leaves 2^%d x %d oracles x cosets of %d %s" % (n.bit_length() - 1, num_oracles, cs, "sub32" if sub32 else "general"), leaves(n, num_oracles, cs, sub32)))
    times = {k: [] for k, _ in cases}
    for _ in range(args.warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in cases:                                # the cases alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    for k, _ in cases:
        ms = statistics.median(times[k])
        print(json.dumps({"case": k, "ms": round(ms, 3), "min": round(min(times[k]), 3), "max": round(max(times[k]), 3),
                          "spread": round((max(times[k]) - min(times[k])) / ms, 3)}), flush=True)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
