"""Multiplicative FFT with output windows (iopx_mul_fft_fp3_windows_dev: the last pass also writes up to two strided windows of the codeword,
the positions a known-degree interpolation reads).  Shared by the CPU-emulation and GPU suites: the output equals the oracle's FFT and each
window equals its strided slice; every argument check fails before anything is written."""
import numpy as np
import pytest

import oracle

SHIFTS = {"one": oracle.fp_one, "19": lambda: oracle.fp_from_ints([19])[0]}


def _n_coeffs(log_n):
    n = 1 << log_n
    return sorted({0, 1, 2, n // 2 + 1, n} - {n + 1})


def _windows(log_n, seed):
    """one and two windows: stride 1 (the whole output), one element (stride 2^log_n), first at 0 and at 2^s - 1, and a middle stride"""
    s = max(log_n // 2, 1)
    two = [(0, 0), ((1 << log_n) - 1, log_n)]
    return [[(0, 0)], [((1 << s) - 1, s)], two, [(seed % (1 << s), s), (0, log_n)], [(1, 1), ((1 << s) - 1, s)]]


# (log_n, shift): single-pass plans up to 2^11 (MF_TILE_BITS), multi-pass above
CASES = [(log_n, sh) for log_n in (1, 5, 11, 12, 13, 16, 20) for sh in ("one", "19")]
CASES_EMU = [(log_n, sh) for log_n, sh in CASES if log_n <= 13]


def check(lib, log_n, shift_kind, in_place_too=True):
    shift = SHIFTS[shift_kind]()
    n = 1 << log_n
    for nc in _n_coeffs(log_n):
        coeffs = oracle.fp_rand(log_n * 31 + nc, nc)
        want = oracle.multiplicative_fft(coeffs, n, shift) if nc else np.zeros((n, 3), dtype=np.uint64)
        wl = _windows(log_n, nc)
        for k, windows in enumerate(wl):
            for in_place in ((False, True) if in_place_too and k == 2 else (False,)):
                out, wins = lib.multiplicative_FFT_windows(coeffs, log_n, shift, windows, in_place=in_place)
                assert np.array_equal(out, want), (log_n, nc, windows, in_place)
                for (first, ls), w in zip(windows, wins):
                    assert np.array_equal(w, want[first::1 << ls]), (log_n, nc, first, ls, in_place)


def check_errors(lib, log_n=6):
    """Each rejected call returns an error and leaves the output untouched."""
    n = 1 << log_n
    shift = SHIFTS["19"]()
    coeffs = oracle.fp_rand(3, n)
    pattern = np.full((n, 3), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    d_in, d_out, d_w0, d_w1, d_w2 = (lib.malloc(24 * n) for _ in range(5))
    try:
        lib.h2d(d_in, coeffs)
        bad = [[(0, 0, d_w0), (1, 1, d_w1), (3, 2, d_w2)],        # three windows
               [(0, 1, d_w0), (0, 0, d_out)],                      # a window aliasing the output
               [(2, 1, d_w0)],                                     # first >= 2^stride
               [(0, log_n + 1, d_w0)],                             # stride above the domain
               [(0, 1, d_w0), (1, 1, 0)]]                          # a null window pointer
        for windows in bad:
            lib.h2d(d_out, pattern)
            with pytest.raises(ValueError):
                lib.multiplicative_FFT_windows_dev(d_in, n, log_n, shift, d_out, windows)
            got = np.empty((n, 3), dtype=np.uint64)
            lib.d2h(got, d_out)
            assert np.array_equal(got, pattern), windows
        lib.multiplicative_FFT_windows_dev(d_in, n, log_n, shift, d_out, [(n - 1, log_n, d_w0)])     # the limits themselves are accepted
        got = np.empty((1, 3), dtype=np.uint64)
        lib.d2h(got, d_w0)
        assert np.array_equal(got[0], oracle.multiplicative_fft(coeffs, n, shift)[n - 1])
    finally:
        for d in (d_in, d_out, d_w0, d_w1, d_w2):
            lib.free(d)
