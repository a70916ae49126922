#!/usr/bin/env python3
"""Times the Aurora prover over alt_bn128 Fr — BLAKE2b and starkware Poseidon, each with the windowed last pass of the forward transform
(IOPX_BN128_FFT_WINDOWS=1) and with the plain transform plus gathers (0) — beside the edwards_Fr / BLAKE2b proof of the same size: one process,
the cases alternating.  Wall time per proof from HIP events (torch.cuda.Event on the stream the library uses), two warm-up rounds, median of
--reps; "spread" is (max - min) / median of the repetitions, the run-to-run spread a difference has to exceed to count.

    python tools/bn128_aurora_bench.py [--reps 9] [--log-n 16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libiop_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=16)
    args = ap.parse_args()
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    n, inputs, seed = 1 << args.log_n, 15, 0x2204
    instances = {f: lib.aurora_example_instance(f, n, inputs, n - 1, seed) for f in (libiop_amd.FIELD_ALT_BN128_FR, libiop_amd.FIELD_EDWARDS_FR)}

    def prover(field, h, windows=None):
        def run():
            if windows is not None:
                lib.set_option("IOPX_BN128_FFT_WINDOWS", windows)
            try:
                return lib.aurora_prove(instances[field], hash=h)
            finally:
                if windows is not None:
                    lib.clear_option("IOPX_BN128_FFT_WINDOWS")
        return run

    bn = libiop_amd.FIELD_ALT_BN128_FR
    cases = []
    for name, h in (("blake2b", libiop_amd.HASH_BLAKE2B), ("poseidon_starkware", libiop_amd.HASH_POSEIDON_STARKWARE)):
        for windows in (1, 0):
            cases.append(("aurora 2^%d alt_bn128_Fr %s windows=%d" % (args.log_n, name, windows), prover(bn, h, windows)))
    cases.append(("aurora 2^%d edwards_Fr blake2b" % args.log_n, prover(libiop_amd.FIELD_EDWARDS_FR, None)))
    times = {k: [] for k, _ in cases}
    proofs = {}
    for _ in range(args.warmup):
        for k, fn in cases:
            proofs[k] = fn()
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
                          "spread": round((max(times[k]) - min(times[k])) / ms, 3), "argument_bytes": len(proofs[k])}), flush=True)
    keys = [k for k, _ in cases]
    print(json.dumps({"windows_on_equals_off": proofs[keys[0]] == proofs[keys[1]] and proofs[keys[2]] == proofs[keys[3]]}), flush=True)
    for inst in instances.values():
        lib.aurora_instance_free(inst)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
