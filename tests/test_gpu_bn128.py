"""The alt_bn128 Fr multiplicative-coset kernels on the MI355X against values computed with Python integers only: every case of
tests/golden/bn128_tiny.json, the 2^22 digests of tests/golden/bn128_function_digests_large.json, and at 2^25 the 2^20-coefficient LDE
(checked by Horner evaluation at sampled positions), the IFFT of that codeword (a round trip) and a fold chain that stays low-degree."""
import ctypes

import numpy as np
import pytest

import bn128_cases as C

pytestmark = pytest.mark.gpu

u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


def test_tiny_cases(lib):
    want = C.load_json("bn128_tiny.json")["cases"]
    got = C.run_tiny(lib)
    for kind in want:
        bad = sorted(k for k in want[kind] if got[kind].get(k) != want[kind][k])
        assert not bad, "%s: %s" % (kind, bad)


def test_digests_2_22(lib):
    want = C.load_json("bn128_function_digests_large.json")["cases"]
    for name, out in C.run_large(lib, 22):
        if C.digest(out) != want[name]["digest"]:
            got = C.chunk_digests(out)
            bad = [i for i, (a, b) in enumerate(zip(got, want[name]["chunks"])) if a != b]
            pytest.fail("%s: chunks %s of %d differ" % (name, bad[:8], len(got)))


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % C.P
    return acc


def test_lde_2_25_round_trip_and_fold_chain(lib):
    """device-pointer forms at the Aurora 2^20 / RS_extra_dimensions 5 shape"""
    m, k = 25, 20
    n, nc = 1 << m, 1 << k
    coeffs = C.data_words("lde 2^25", nc)
    shift = C.elem(C.LDE_SHIFT)
    g = lib.bn128_subgroup_generator(m)
    d_c, d_e, d_b = lib.malloc(32 * nc), lib.malloc(32 * n), lib.malloc(32 * n)
    try:
        lib.h2d(d_c, coeffs)
        lib._check(lib.c.iopx_mul_fft_bn128_dev(ctypes.c_void_p(d_c), nc, m, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), ctypes.c_void_p(d_e)))
        # sampled positions against Horner's rule (on the Montgomery integers: the transform is linear)
        ci = C.words_to_ints(coeffs)
        gv = C.gen(m)
        for pos in [0, 1, 2, 12345, (1 << 24) + 7, n // 3, n - 2, n - 1]:
            w = np.empty((1, 4), dtype=np.uint64)
            lib.d2h(w, d_e + 32 * pos)
            assert C.words_to_ints(w) == [_horner(ci, C.LDE_SHIFT * pow(gv, pos, C.P) % C.P)], pos
        # IFFT of the codeword: the coefficients, then zeros
        lib._check(lib.c.iopx_mul_ifft_bn128_dev(ctypes.c_void_p(d_e), m, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), ctypes.c_void_p(d_b)))
        head = np.empty((nc, 4), dtype=np.uint64)
        lib.d2h(head, d_b)
        assert np.array_equal(head, coeffs)
        tail = np.empty((n - nc, 4), dtype=np.uint64)
        lib.d2h(tail, d_b + 32 * nc)
        assert not tail.any()
        del tail
        # fold chain with cosets of 2 down to 2^10 points: the degree bound halves each time, so the final codeword has degree < 2^5
        src, dst, cur, s = d_e, d_b, m, C.LDE_SHIFT
        level = 0
        while cur > 10:
            level += 1
            gc = lib.bn128_subgroup_generator(cur)
            x = C.elem(C.fold_chain_challenge(100 + level))
            sw = C.elem(s)
            lib._check(lib.c.iopx_fri_fold_mul_bn128_dev(ctypes.c_void_p(src), cur, gc.ctypes.data_as(u64p), sw.ctypes.data_as(u64p), 2,
                                                         x.ctypes.data_as(u64p), ctypes.c_void_p(dst)))
            src, dst, cur, s = dst, src, cur - 1, s * s % C.P
        last = np.empty((1 << 10, 4), dtype=np.uint64)
        lib.d2h(last, src)
        c_last = lib.multiplicative_IFFT_bn128(last, C.elem(s))
        assert c_last[:1 << 5].any() and not c_last[1 << 5:].any()
    finally:
        for d in (d_c, d_e, d_b):
            lib.free(d)


def test_host_and_device_forms_agree(lib):
    """the host-pointer wrappers and the _dev entries, and the known-degree IFFT against the plain one on the sub-coset"""
    m = 14
    n = 1 << m
    coeffs = C.data_words("forms", n // 2 + 3)
    shift = C.elem(C.seeded_scalar("forms shift"))
    host = lib.multiplicative_FFT_bn128(coeffs, m, shift)
    g = lib.bn128_subgroup_generator(m)
    d_c, d_o = lib.malloc(coeffs.nbytes), lib.malloc(32 * n)
    try:
        lib.h2d(d_c, coeffs)
        lib._check(lib.c.iopx_mul_fft_bn128_dev(ctypes.c_void_p(d_c), coeffs.shape[0], m, g.ctypes.data_as(u64p), shift.ctypes.data_as(u64p), ctypes.c_void_p(d_o)))
        dev = np.empty((n, 4), dtype=np.uint64)
        lib.d2h(dev, d_o)
    finally:
        lib.free(d_c)
        lib.free(d_o)
    assert np.array_equal(host, dev)
    kd = lib.multiplicative_IFFT_of_known_degree_bn128(host, coeffs.shape[0], shift)
    assert np.array_equal(kd[:coeffs.shape[0]], coeffs) and not kd[coeffs.shape[0]:].any()
    for eta in (1, 2, 3, 4, 5):
        f = lib.multiplicative_evaluate_next_f_i_bn128(host, shift, 1 << eta, C.elem(C.seeded_scalar("forms x %d" % eta)))
        assert f.shape == (n >> eta, 4)
