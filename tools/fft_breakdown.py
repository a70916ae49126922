#!/usr/bin/env python3
"""Per-kernel time of one standalone additive FFT (BASELINE configs[1]: 2^22 coefficients over the standard basis, shift 0) on cuda:0,
with IOPX_PROFILE_LEVELS=1 the phase-1 passes by level.  Usage: fft_breakdown.py [log_n]

fft_breakdown.py reextend [d_dim] [m] [batch] [reps]: over gf64, gf128 and gf256, one fused re-extension of `batch` vectors of 2^d_dim evaluations
onto the 2^m points of the codeword domain (iopx_add_reextend_FIELD_batch_dev) next to the separate calls it replaces (per vector one inverse transform
and one low-degree extension), alternating: median, minimum and maximum of `reps` timings each (host clock around a device synchronise), and the
per-kernel profile of one call of each kind.  Defaults: 17 22 3 7, the shape of Aurora's f_Az, f_Bz, f_Cz at 2^20 constraints with 5 rate bits."""
import sys, time
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import libiop_amd
from libiop_amd import domains



def reextend_mode(argv):
    import statistics
    d, m, batch, reps = (int(a) for a in (argv + ["17", "22", "3", "7"][len(argv):])[:4])
    lib = libiop_amd.Library()
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    for field in (domains.GF64(), domains.GF128(), domains.GF256()):
        W = field.words
        ops = domains.DeviceOps(lib, torch, torch.device("cuda:0"), field)
        basis, shift = field.standard_basis(m), np.zeros(W, dtype=np.uint64)
        shift[0], es = 1 << 40, np.zeros(W, dtype=np.uint64)
        es[0] = 1 << 41
        packed = ops.upload(np.random.Generator(np.random.PCG64(0x2201)).integers(0, 2**64, size=(batch << d, W), dtype=np.uint64))
        outs = [ops.empty(1 << m) for _ in range(batch)]
        coeffs = ops.empty(1 << d)
        ifft = lib.additive_IFFT_gf64_dev if W == 1 else lambda *a: lib.additive_IFFT_dev(*a, words=W)
        lde = lib.additive_LDE_gf64_dev if W == 1 else lambda *a: lib.additive_LDE_dev(*a, words=W)

        def fused():
            lib.additive_reextend_batch_dev(packed.data_ptr(), batch, basis, d, es, shift, 0, 1 << (m - d), [o.data_ptr() for o in outs], words=W)

        def separate():
            for k in range(batch):
                ifft(packed[k << d:(k + 1) << d].data_ptr(), basis[:d], es, coeffs.data_ptr())
                lde(coeffs.data_ptr(), 1 << d, basis, shift, 0, 1 << (m - d), outs[k].data_ptr())

        kinds = {"fused": fused, "separate": separate}
        times = {k: [] for k in kinds}
        for _ in range(2):
            for fn in kinds.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in kinds.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k, fn in kinds.items():
            t = times[k]
            print("%s %-8s d=%d m=%d batch=%d: median %.3f ms (min %.3f, max %.3f)" % (field.name, k, d, m, batch, statistics.median(t), min(t), max(t)))
            lib.profile_begin()
            fn()
            rep = lib.profile_report()
            for name, v in sorted(rep.items(), key=lambda kv: -kv[1][1]):
                print("    %-32s x%-3d %.3f ms" % (name, v[0], v[1]))
            print("    sum %.3f ms in %d launches" % (sum(v[1] for v in rep.values()), sum(v[0] for v in rep.values())))


if len(sys.argv) > 1 and sys.argv[1] == "reextend":
    reextend_mode(sys.argv[2:])
    sys.exit(0)
m = int(sys.argv[1]) if len(sys.argv) > 1 else 22
lib = libiop_amd.Library()
lib.set_stream(torch.cuda.current_stream().cuda_stream)
ops = domains.DeviceOps(lib, torch, torch.device("cuda:0"), domains.GF192())
basis, shift = libiop_amd.standard_basis(m), np.zeros(3, dtype=np.uint64)
d_in = ops.upload(np.random.Generator(np.random.PCG64(0x2201)).integers(0, 2**64, size=(1 << m, 3), dtype=np.uint64))
d_out = ops.empty(1 << m)
for _ in range(3):
    lib.additive_FFT_dev(d_in.data_ptr(), 1 << m, basis, shift, d_out.data_ptr())
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    lib.additive_FFT_dev(d_in.data_ptr(), 1 << m, basis, shift, d_out.data_ptr())
torch.cuda.synchronize()
print("wall %.3f ms per transform" % ((time.perf_counter() - t0) * 100))
lib.profile_begin()
lib.additive_FFT_dev(d_in.data_ptr(), 1 << m, basis, shift, d_out.data_ptr())
rep = lib.profile_report()
tot = 0.0
for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1]):
    print("%-28s x%-3d %.3f ms" % (k, v[0], v[1]))
    tot += v[1]
print("sum %.3f ms in %d launches" % (tot, sum(v[0] for v in rep.values())))
