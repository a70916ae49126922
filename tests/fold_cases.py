"""FRI fold cases over cosets larger than the fused kernels take (additive eta > FOLD_MAX_ETA = 3, multiplicative eta > 3): the unfused
k_fri_fold2 / k_fri_fold2_mul chains, which ping-pong through two temporaries.  Shared by the CPU-emulation and GPU suites; every result is
compared bit for bit with the oracle (additive_evaluate_next_f_i_over_entire_domain / multiplicative_..., fri_aux.tcc:36-249).
The reference's own FRI tests draw localization vectors that sum to the codeword dimension (test_fri.cpp), so steps of 4-8 are normal input."""
import numpy as np

import oracle
from helpers import rand_elems

W = 3


def additive_domain(m, kind, seed):
    if kind == "std0":
        return oracle.standard_basis(m, W), np.zeros(W, dtype=np.uint64)
    if kind == "aurora":                       # one-word shift past the basis, as the Aurora codeword domain
        return oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)
    return rand_elems(seed + 1, m, W), rand_elems(seed, 1, W)[0]


def _additive_sizes(ms):
    return [(m, cs) for m in ms for cs in sorted({16, 32, 256, 1 << m}) if cs <= 1 << m]


KINDS = ("std0", "aurora", "general")
# (m, coset size, domain kind): cosets of 16, 32, 256 and the whole domain; at 2^20 (seconds of oracle time per case) one kind per size
ADDITIVE = ([(m, cs, kind) for (m, cs) in _additive_sizes([4, 8, 12, 16]) for kind in KINDS]
            + [(20, cs, KINDS[i % 3]) for i, (_, cs) in enumerate(_additive_sizes([20]))])
ADDITIVE_EMU = [c for c in ADDITIVE if c[0] <= 12] + [(16, 32, "general")]

SHIFTS = ("one", "19", "random")
# (log_n, coset size, shift): cosets of 16, 64 and the whole coset; at 2^20 one shift per size
MULTIPLICATIVE = ([(log_n, cs, sh) for log_n in (4, 10, 16) for cs in sorted({16, 64, 1 << log_n}) if cs <= 1 << log_n for sh in SHIFTS]
                  + [(20, cs, SHIFTS[i]) for i, cs in enumerate((16, 64, 1 << 20))])
MULTIPLICATIVE_EMU = [c for c in MULTIPLICATIVE if c[0] <= 10] + [(8, 256, "random"), (16, 64, "19")]


def fp_shift(kind):
    if kind == "one":
        return oracle.fp_one()
    if kind == "19":
        return oracle.fp_from_ints([19])[0]
    return oracle.fp_rand(5, 1)[0]


def check_additive(lib, m, cs, kind):
    basis, shift = additive_domain(m, kind, 400 + m)
    f = rand_elems(500 + m + cs, 1 << m, W)
    x = rand_elems(600 + m, 1, W)[0]
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain(f, basis, shift, cs, x),
                          oracle.fri_fold_additive(f, basis, shift, cs, x)), (m, cs, kind)


def check_additive_x_in_domain(lib, m, cs):
    """x_i equal to a point of the first, a middle and the last coset: the interpolation's denominators vanish there."""
    basis, shift = additive_domain(m, "general", 9)
    f = rand_elems(1, 1 << m, W)
    pts = oracle.all_subset_sums(basis, shift)
    n = 1 << m
    for idx in (0, 1, n // 2 + cs // 2, n - 1):
        assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain(f, basis, shift, cs, pts[idx]),
                              oracle.fri_fold_additive(f, basis, shift, cs, pts[idx])), idx


def check_multiplicative(lib, log_n, cs, shift_kind):
    shift = fp_shift(shift_kind)
    f = oracle.fp_rand(log_n * 7 + cs, 1 << log_n)
    x = oracle.fp_rand(99 + cs, 1)[0]
    assert np.array_equal(lib.multiplicative_evaluate_next_f_i(f, shift, cs, x),
                          oracle.fri_fold_multiplicative(f, shift, cs, x)), (log_n, cs, shift_kind)


def _fp_pow2k(a, k):
    for _ in range(k):
        a = oracle.fp_mul(a[None, :], a[None, :])[0]
    return a


def check_additive_chain(lib, m, deg_log, etas, seed, low_degree_only=False):
    """Folds of the codeword of a degree-2^deg_log polynomial, one coset size after the other over the derived domains (fri_ldt.tcc round
    structure): each step equal to the oracle's (unless low_degree_only), and the last word again of the folded degree (its IFFT's high
    coefficients are zero)."""
    basis, shift = additive_domain(m, "aurora", seed)
    doms = oracle.fri_domains_additive(basis, shift, etas)
    cw = lib.additive_FFT(rand_elems(seed, 1 << deg_log, W), basis, shift)
    cb, csh, deg = basis, shift, 1 << deg_log
    for i, eta in enumerate(etas):
        x = rand_elems(seed + 50 + i, 1, W)[0]
        nxt = lib.evaluate_next_f_i_over_entire_domain(cw, cb, csh, 1 << eta, x)
        if not low_degree_only:
            assert np.array_equal(nxt, oracle.fri_fold_additive(cw, cb, csh, 1 << eta, x)), i
        cw, (cb, csh) = nxt, doms[i]
        deg >>= eta
        assert not lib.additive_IFFT(cw, cb, csh)[deg:].any(), i


def check_multiplicative_chain(lib, log_n, deg_log, etas, seed, low_degree_only=False):
    shift = fp_shift("19")
    cw = lib.multiplicative_FFT(oracle.fp_rand(seed, 1 << deg_log), log_n, shift)
    deg = 1 << deg_log
    for i, eta in enumerate(etas):
        x = oracle.fp_rand(seed + 50 + i, 1)[0]
        nxt = lib.multiplicative_evaluate_next_f_i(cw, shift, 1 << eta, x)
        if not low_degree_only:
            assert np.array_equal(nxt, oracle.fri_fold_multiplicative(cw, shift, 1 << eta, x)), i
        cw, shift, deg = nxt, _fp_pow2k(shift, eta), deg >> eta
        assert not lib.multiplicative_IFFT(cw, shift)[deg:].any(), i
