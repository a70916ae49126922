"""The alt_bn128 Fr multiplicative-coset kernels (libiop_amd/csrc/fft_mul.hip, ldt_reducer.hip) compiled for the CPU (tests/emu) against values computed with
Python integers only: every case of tests/golden/bn128_tiny.json, the full-size digest recipes at m = 10 and 12
(tests/golden/bn128_function_digests_large.json), the host scalars, the argument checks and the in-place forms.  The GPU leg is
tests/test_gpu_bn128.py."""
import ctypes

import numpy as np
import pytest

import bn128_cases as C
from emu_lib import emu


def test_tiny_cases():
    want = C.load_json("bn128_tiny.json")["cases"]
    got = C.run_tiny(emu())
    for kind in want:
        bad = sorted(k for k in want[kind] if got[kind].get(k) != want[kind][k])
        assert not bad, "%s: %s" % (kind, bad)


@pytest.mark.parametrize("m", [10, 12])
def test_digest_recipes(m):
    want = C.load_json("bn128_function_digests_large.json")["cases"]
    for name, out in C.run_large(emu(), m):
        assert C.digest(out) == want[name]["digest"], name


def test_generators_and_host_scalars():
    lib = emu()
    for k in (0, 1, 5, 17, 28):
        assert C.words_to_ints(lib.bn128_subgroup_generator(k).reshape(1, 4)) == [C.mont(C.gen(k))]
    assert C.words_to_ints(lib.bn128_subgroup_generator(28).reshape(1, 4)) == [C.mont(C.OMEGA_28)]
    assert C.words_to_ints(lib.bn128_multiplicative_generator().reshape(1, 4)) == [C.mont(5)]
    a, b = C.seeded_scalar("host a"), C.seeded_scalar("host b")
    assert C.words_to_ints(lib.bn128_host_mul(C.elem(a), C.elem(b)).reshape(1, 4)) == [C.mont(a * b % C.P)]
    assert C.words_to_ints(lib.bn128_host_pow(C.elem(a), 12345).reshape(1, 4)) == [C.mont(pow(a, 12345, C.P))]
    assert C.words_to_ints(lib.bn128_host_inverse(C.elem(a)).reshape(1, 4)) == [C.mont(pow(a, C.P - 2, C.P))]
    with pytest.raises(ValueError):
        lib.bn128_host_inverse(C.elem(0))


def test_round_trip_and_canonical_outputs():
    """IFFT(FFT(c)) = c on a coset, and outputs are canonical words (below r)"""
    lib = emu()
    coeffs = C.data_words("round trip", 1 << 9)
    s = C.elem(C.seeded_scalar("round trip shift"))
    evals = lib.multiplicative_FFT_bn128(coeffs, 11, s)
    assert all(v < C.P for v in C.words_to_ints(evals))
    back = lib.multiplicative_IFFT_bn128(evals, s)
    assert np.array_equal(back[:1 << 9], coeffs) and not back[1 << 9:].any()


def test_argument_checks():
    lib = emu()
    one = C.elem(1)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    with pytest.raises(ValueError, match="2-adicity"):
        lib._check(lib.c.iopx_mul_fft_bn128_dev(None, 0, 29, lib.bn128_subgroup_generator(1).ctypes.data_as(u64p), one.ctypes.data_as(u64p), None))
    with pytest.raises(ValueError, match="2-adicity"):
        lib.bn128_subgroup_generator(29)
    with pytest.raises(ValueError, match="null"):
        lib._check(lib.c.iopx_mul_ifft_bn128(None, 3, None, None, None))
    f = C.data_words("checks", 16)
    x = C.elem(7)
    with pytest.raises(ValueError, match="coset size"):
        lib.multiplicative_evaluate_next_f_i_bn128(f, one, 3, x)
    with pytest.raises(ValueError, match="coset size"):
        lib.multiplicative_evaluate_next_f_i_bn128(f, one, 32, x)
    with pytest.raises(ValueError, match="generator"):
        lib.multiplicative_FFT_bn128(f, 4, one, gen=C.elem(C.gen(3)))
    with pytest.raises(ValueError, match="exceed"):
        lib.multiplicative_FFT_bn128(C.data_words("checks", 17), 4, one)
    # the null-pointer checks of these entries are shared with the edwards_Fr ones (one host implementation for both fields)
    for call in (lambda: lib.c.iopx_mul_ifft_known_degree_fp3_dev(None, 4, 3, None, None, None),
                 lambda: lib.c.iopx_mul_ifft_known_degree_bn128_dev(None, 4, 3, None, None, None),
                 lambda: lib.c.iopx_mul_fft_fp3(None, 4, 3, None, None, None),
                 lambda: lib.c.iopx_mul_ifft_fp3(None, 3, None, None, None),
                 lambda: lib.c.iopx_fri_fold_mul_fp3(None, 3, None, None, 2, None, None)):
        with pytest.raises(ValueError, match="null"):
            lib._check(call())


def test_in_place():
    """d_coeffs == d_out / d_evals == d_out, as the edwards_Fr arm allows"""
    lib = emu()
    n, s = 1 << 8, C.elem(C.seeded_scalar("in place shift"))
    coeffs = C.data_words("in place", n)
    want_fft = lib.multiplicative_FFT_bn128(coeffs, 8, s)
    want_ifft = lib.multiplicative_IFFT_bn128(coeffs, s)
    g = lib.bn128_subgroup_generator(8)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    d = lib.malloc(32 * n)
    try:
        lib.h2d(d, coeffs)
        lib._check(lib.c.iopx_mul_fft_bn128_dev(ctypes.c_void_p(d), n, 8, g.ctypes.data_as(u64p), s.ctypes.data_as(u64p), ctypes.c_void_p(d)))
        out = np.empty((n, 4), dtype=np.uint64)
        lib.d2h(out, d)
        assert np.array_equal(out, want_fft)
        lib.h2d(d, coeffs)
        lib._check(lib.c.iopx_mul_ifft_bn128_dev(ctypes.c_void_p(d), 8, g.ctypes.data_as(u64p), s.ctypes.data_as(u64p), ctypes.c_void_p(d)))
        lib.d2h(out, d)
        assert np.array_equal(out, want_ifft)
    finally:
        lib.free(d)


def test_fold_copy_and_whole_domain():
    """eta = 0 is a copy; a coset as large as the domain folds to one value"""
    lib = emu()
    f = C.data_words("fold copy", 32)
    s, x = C.elem(3), C.elem(C.seeded_scalar("fold copy x"))
    assert np.array_equal(lib.multiplicative_evaluate_next_f_i_bn128(f, s, 1, x), f)
    whole = lib.multiplicative_evaluate_next_f_i_bn128(f, s, 32, x)
    assert whole.shape == (1, 4)
    # the interpolant of f on all 32 points, at x: the IFFT's coefficients evaluated there
    coeffs = C.words_to_ints(lib.multiplicative_IFFT_bn128(f, s))
    xv = C.seeded_scalar("fold copy x")
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * xv + c) % C.P
    assert C.words_to_ints(whole) == [acc]
