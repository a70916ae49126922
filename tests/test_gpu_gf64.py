"""The GF(2^64) kernels (libiop_amd/csrc/gf64.hip) on the MI355X: the cases of tests/gf64_cases.py against the oracle and the pure-Python
product model (the CPU leg is tests/test_gf64_emu.py), and one full-size run at m = 22."""
import ctypes

import numpy as np
import pytest

import gf64_cases as C
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


def test_product(lib):
    C.check_product(lib)


def test_inverse(lib):
    C.check_inverse(lib)


def test_fft(lib):
    C.check_fft(lib)


def test_fft_schedules(lib):
    C.check_schedules(lib)


def test_placement_and_profile(lib):
    C.check_placement_and_profile(lib)


def test_lde_coset_ranges(lib):
    C.check_lde_ranges(lib)


def test_lde_upper_pass_whole(lib):
    C.check_lde_upper_pass_whole(lib)


def test_ifft(lib):
    C.check_ifft(lib)


def test_ifft_in_place_and_known_degree(lib):
    C.check_ifft_in_place_and_known_degree(lib)


def test_fold(lib):
    C.check_fold(lib)


def test_fold_chain(lib):
    C.check_fold_chain(lib)


def test_domain_chain(lib):
    C.check_domain_chain(lib)


def test_ldt_combination(lib):
    C.check_ldt(lib)


def test_generic_merkle_and_query_responses_on_8_byte_elements(lib):
    """A pin of the existing generic path (elem_bytes = 8): passes without the gf64 kernels."""
    C.check_merkle_and_queries(lib)


def test_host_and_device_forms_agree(lib):
    C.check_host_and_device_forms(lib)


def test_argument_checks(lib):
    C.check_argument_checks(lib)


def test_fri_snark_transcripts(lib):
    import torch
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        C.check_fri_snark(lib, torch, torch.device("cuda:0"))
    finally:
        lib.use_own_stream()


def test_fri_snark_other_fields_unchanged(lib):
    import torch
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        C.check_fri_snark_other_fields_unchanged(lib, torch, torch.device("cuda:0"))
    finally:
        lib.use_own_stream()


def test_full_size_2_22(lib):
    """m = 22 with 2^20 seeded coefficients: the LDE at 8 positions against Horner evaluation, the IFFT of the codeword compared on the device
    with the padded coefficients, and a fold chain with cosets of 4 down to 2^10 that stays within its degree bound.  No whole-vector oracle
    call at this size."""
    m, d = 22, 20
    n = 1 << m
    basis, shift = C.std_basis(m), C.elem((1 << 63) | 0x2A)
    coeffs = C.seeded("full size", 1 << d)
    padded = np.zeros((n, 1), dtype=np.uint64)
    padded[:1 << d] = coeffs
    vp = ctypes.c_void_p
    d_a, d_b, d_c, d_cnt = lib.malloc(8 * n), lib.malloc(8 * n), lib.malloc(8 * n), lib.malloc(8)
    try:
        lib.h2d(d_a, coeffs)
        lib.additive_LDE_gf64_dev(d_a, 1 << d, basis, shift, 0, 1 << (m - d), d_b)
        for pos in (0, 1, 2, 12345, (1 << 21) + 7, n // 3, n - 2, n - 1):
            x = int(shift[0])
            for k in range(m):
                if (pos >> k) & 1:
                    x ^= int(basis[k, 0])
            got = np.empty(1, dtype=np.uint64)
            lib.d2h(got, d_b + 8 * pos)
            assert int(got[0]) == int(oracle.poly_eval(coeffs, C.elem(x))[0]), pos
        lib.additive_IFFT_gf64_dev(d_b, basis, shift, d_c)
        lib.h2d(d_a, padded)
        lib.h2d(d_cnt, np.zeros(1, dtype=np.uint64))
        lib._check(lib.c.iopx_count_mismatch_dev(vp(d_c), vp(d_a), ctypes.c_size_t(8 * n), vp(d_cnt)))
        cnt = np.empty(1, dtype=np.uint64)
        lib.d2h(cnt, d_cnt)
        assert int(cnt[0]) == 0
        # fold chain: d_b (the codeword) -> 2^10 values, degree bound 2^20 / 4^6 = 2^8
        loc = [2] * 6
        domains = lib.fri_additive_domains_gf64(basis, shift, loc)
        src, dst = d_b, d_c
        for i, eta in enumerate(loc):
            b, s = domains[i]
            lib.evaluate_next_f_i_over_entire_domain_gf64_dev(src, b, s, 1 << eta, C.elem(int(C.seeded("full x %d" % i, 1)[0, 0])), dst)
            src, dst = dst, src
        last = np.empty((1 << 10, 1), dtype=np.uint64)
        lib.d2h(last, src)
        nb, ns = domains[-1]
        tail = oracle.additive_ifft(last, nb, ns)
        assert tail[:1 << 8].any() and not tail[1 << 8:].any()
    finally:
        for p in (d_a, d_b, d_c, d_cnt):
            lib.free(p)
