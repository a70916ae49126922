#!/usr/bin/env python3
"""Times the alt_bn128 Fr multiplicative-coset kernels against the edwards_Fr ones on the same shapes, in one process, alternating the two
fields: the 2^20-coefficient LDE onto 2^25 points (Aurora at 2^20 constraints with RS_extra_dimensions 5), the square transform and the IFFT
at 2^22, and a localization-2 fold chain from 2^25 down to 2^10.  Wall time per call from HIP events (torch.cuda.Event on the stream the
library uses) after warm-up, median of --reps.  Per timing: ms, elements/s, algorithmic bytes (2 n s per HBM pass, s = bytes per element)
over time as a share of 8 TB/s, and field products per second.  Kernel-only times: run this under `rocprofv3 --kernel-trace --stats -- python
tools/bn128_fft_bench.py` in a separate run.

    python tools/bn128_fft_bench.py [--reps 9]
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

u64p = ctypes.POINTER(ctypes.c_uint64)
TILE_BITS, COLS = 11, 4            # the pass schedule of k_mfft_pass / k_bn_mfft_pass
BN128_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def passes(logn, logrho):
    """HBM sweeps of one transform (run_mfft's schedule)"""
    b, k = logrho, 0
    if logn <= TILE_BITS:
        return 1
    if logrho < TILE_BITS:
        k, b = 1, TILE_BITS
    while b < logn:
        b += min(TILE_BITS - COLS, logn - b)
        k += 1
    return max(k, 1)


class Field:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        self.s = 32 if name == "bn128" else 24
        self.w = self.s // 8

    def gen(self, log_n):
        g = self.lib.bn128_subgroup_generator(log_n) if self.name == "bn128" else libiop_amd.edwards_subgroup_generator(log_n)
        return np.ascontiguousarray(g, dtype=np.uint64)

    def elem(self, v):
        if self.name != "bn128":
            return libiop_amd.edwards_to_montgomery([v])[0]
        m = v * (1 << 256) % BN128_R
        return np.array([(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)

    def fft(self, d_in, nc, log_n, shift, d_out):
        f = self.lib.c.iopx_mul_fft_bn128_dev if self.name == "bn128" else self.lib.c.iopx_mul_fft_fp3_dev
        g = self.gen(log_n)
        self.lib._check(f(ctypes.c_void_p(d_in), nc, log_n, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), ctypes.c_void_p(d_out)))

    def ifft(self, d_in, log_n, shift, d_out):
        f = self.lib.c.iopx_mul_ifft_bn128_dev if self.name == "bn128" else self.lib.c.iopx_mul_ifft_fp3_dev
        g = self.gen(log_n)
        self.lib._check(f(ctypes.c_void_p(d_in), log_n, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), ctypes.c_void_p(d_out)))

    def fold(self, d_in, log_n, shift, x, d_out):
        f = self.lib.c.iopx_fri_fold_mul_bn128_dev if self.name == "bn128" else self.lib.c.iopx_fri_fold_mul_fp3_dev
        g = self.gen(log_n)
        self.lib._check(f(ctypes.c_void_p(d_in), log_n, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), 2, x.ctypes.data_as(u64p),
                          ctypes.c_void_p(d_out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    lib = libiop_amd.lib()
    lib.init(0)
    torch.cuda.set_device(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    fields = [Field(lib, "bn128"), Field(lib, "edwards")]
    rng = np.random.default_rng(7)
    big = 1 << 25
    buf = {}
    for fd in fields:
        a = rng.integers(0, 1 << 62, size=(big, fd.w), dtype=np.uint64)      # canonical in both fields (below 2^190 < p)
        a[:, -1] &= np.uint64((1 << 52) - 1)
        t_in = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        buf[fd.name] = (t_in, torch.empty_like(t_in), torch.empty_like(t_in))
    shift = {fd.name: fd.elem(5) for fd in fields}

    def lde(fd):
        t_in, t_out, _ = buf[fd.name]
        fd.fft(t_in.data_ptr(), 1 << 20, 25, shift[fd.name], t_out.data_ptr())

    def sq(fd):
        t_in, t_out, _ = buf[fd.name]
        fd.fft(t_in.data_ptr(), 1 << 22, 22, shift[fd.name], t_out.data_ptr())

    def ifft(fd):
        t_in, t_out, _ = buf[fd.name]
        fd.ifft(t_in.data_ptr(), 22, shift[fd.name], t_out.data_ptr())

    P = {"bn128": BN128_R, "edwards": libiop_amd.EDWARDS_FR_MODULUS}

    def chain(fd):
        t_in, t_a, t_b = buf[fd.name]
        src, dst, s = t_in, t_a, 5
        for cur in range(25, 10, -1):
            fd.fold(src.data_ptr(), cur, fd.elem(s), fd.elem(1000 + cur), dst.data_ptr())
            src, dst = dst, (t_b if dst is t_a else t_a)
            s = s * s % P[fd.name]

    def model(kind, fd):
        s = fd.s
        if kind == "lde_2^20_to_2^25":
            n = 1 << 25
            return n, 2 * n * s * passes(25, 5), (n // 2) * 20
        if kind == "fft_2^22":
            n = 1 << 22
            return n, 2 * n * s * passes(22, 0), (n // 2) * 22
        if kind == "ifft_2^22":
            n = 1 << 22
            return n, 2 * n * s * passes(22, 0), (n // 2) * 22 + 2 * n
        n = sum(1 << c for c in range(25, 10, -1))
        return n, sum(((1 << c) + (1 << (c - 1))) * s for c in range(25, 10, -1)), sum(3 * (1 << (c - 1)) for c in range(25, 10, -1))

    cases = [("lde_2^20_to_2^25", lde), ("fft_2^22", sq), ("ifft_2^22", ifft), ("fold_chain_2^25_to_2^10", chain)]
    times = {(k, fd.name): [] for k, _ in cases for fd in fields}
    for _ in range(args.warmup):
        for _, fn in cases:
            for fd in fields:
                fn(fd)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in cases:
            for fd in fields:                          # the two fields alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(fd)
                e1.record()
                e1.synchronize()
                times[(k, fd.name)].append(e0.elapsed_time(e1))
    rows = []
    for k, _ in cases:
        row = {"case": k}
        for fd in fields:
            ms = statistics.median(times[(k, fd.name)])
            n, nbytes, prods = model(k, fd)
            row[fd.name] = {"ms": round(ms, 3), "elements_per_s": "%.3g" % (n / ms * 1e3), "hbm_share_of_8TBps": round(nbytes / (ms * 1e-3) / 8e12, 3),
                            "products_per_s": "%.3g" % (prods / ms * 1e3)}
        row["ratio_bn128_over_edwards"] = round(row["bn128"]["ms"] / row["edwards"]["ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    lib.use_own_stream()


if __name__ == "__main__":
    main()
