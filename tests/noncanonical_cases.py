"""Prime-field elements that are not canonical Montgomery representatives (raw 192-bit words, what libiop's random_vector<FieldT> produces — "invalid
elements for libff prime fields", algebra/polynomials/polynomial.tcc:233-234): outside the library's contract, but its behaviour on them is defined and
tested — the multiplicative transforms return CANONICAL words that are congruent mod p to the results a CPU path computes from the same raw words,
for edwards_Fr while every raw word is below edwards_raw_limit(levels) (`check` draws its seeded words below it; `check_raw_limit` sits at the bound) and for
alt_bn128 Fr for every raw 256-bit word (the CPU path carries unreduced representatives through its additions: two of libiop's Ligero tests depend on that and are not served)."""
import numpy as np

import libiop_amd
import oracle

P = libiop_amd.EDWARDS_FR_MODULUS


def _ints(a):
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) for r in a]


def check(lib, seed=5):
    rng = np.random.default_rng(seed)
    shift = libiop_amd.edwards_to_montgomery([3])[0]
    for m in (1, 4, 7):
        n = 1 << m
        limit = edwards_raw_limit(m)                                                   # the promise ends there (about 2^11 p; see below)
        draws = [int.from_bytes(rng.bytes(32), "little") % limit for _ in range(n)]
        assert max(draws) < limit and max(draws) > (1 << 190)
        raw = np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(3)] for v in draws], dtype=np.uint64)
        for got, want in ((lib.multiplicative_FFT(raw, m, shift), oracle.multiplicative_fft(raw, n, shift)),
                          (lib.multiplicative_IFFT(raw, shift), oracle.multiplicative_ifft(raw, shift))):
            g, w = _ints(got), _ints(want)
            assert all(x < P for x in g), "the kernels return canonical representatives"
            assert all((x - y) % P == 0 for x, y in zip(g, w)), "congruent mod p to the CPU path's result"


# ---- how far the promise reaches: the largest raw word, per field ------------------------------------------------------------------------------
def edwards_raw_limit(levels):
    """The multiplicative transforms take raw edwards_Fr words below 2^192 - 8 p * levels, `levels` being the radix-2 levels they run (log2 n for
    the IFFT, ceil(log2 #coefficients) for the FFT).  fp7_bfly forms (x + t, x + 8p - t) with t < 2p and no reduction, so the largest value grows
    by at most 8p per level, and fp7_pack keeps 192 bits: max + 8 p levels must stay below 2^192.  Canonical inputs (below p) are far inside it
    for every length (31 levels: 249 p < 2^188).  The bound is exact at n = 2 — (limit, 0) gives x + 8p - 0 = 2^192 — and only SUFFICIENT beyond: the
    true threshold for n > 2 is not known (growth of exactly 8p needs t = 0 at every level), so between this limit and 2^192 results are undefined.
    A transform on a coset with shift != 1 starts with a product (k_fp_scale_pow) when it is forward: that one takes any 192-bit word."""
    return (1 << 192) - 8 * P * levels


def _congruent(F, got, want, what):
    assert all(x < F.P for x in got), "%s: canonical words out" % what
    bad = [i for i, (x, y) in enumerate(zip(got, want)) if (x - y) % F.P]
    assert not bad, "%s: %d outputs not congruent, first at %s" % (what, len(bad), bad[:6])


def _raw_vectors(n, limit, seed):
    rng = np.random.default_rng(seed)
    top = limit - 1
    yield "every word at the limit", [top] * n
    yield "even at the limit, odd 0", [top if i % 2 == 0 else 0 for i in range(n)]
    yield "even at the limit, odd limit - 12345", [top if i % 2 == 0 else top - 12345 for i in range(n)]
    yield "impulse at 0", [top] + [0] * (n - 1)
    yield "random below the limit", [int.from_bytes(rng.bytes(40), "little") % limit for _ in range(n)]


def check_raw_limit(lib, field):
    """edwards_Fr: congruent canonical outputs for raw words up to edwards_raw_limit(levels) - 1, at 1 to 13 levels (one and two passes); AT the
    limit with n = 2 the second output is wrong (2^192 is dropped by fp7_pack), which pins the limit as exact rather than cautious — a change
    that makes the first pass reduce what it loads must remove that assertion (it pins a wrong answer on purpose) and raise the limit; above it results are undefined (canonical
    words, not congruent: the vector of the issue, even 2^192 - 1 / odd 2^192 - 12346, is kept as a run that must not fault).
    alt_bn128 Fr: EVERY raw 256-bit word is taken — bn9_unpack gives normalised limbs and a value below 2^256, which is a "weak" value
    (bn254_dev.h), and every sum or difference goes through bn9_reduce: transforms, folds and the LDT combination return canonical words
    congruent to the plain-integer result, up to 2^256 - 1 everywhere."""
    import limb_bound_cases as C
    F = C.FIELDS[field]
    s = F.scalar("raw shift")
    if F is C.FP:
        for log_n in (1, 2, 4, 7, 11, 13):
            n = 1 << log_n
            for name, vec in _raw_vectors(n, edwards_raw_limit(log_n), log_n):
                red = [v % P for v in vec]
                _congruent(F, C.lib_ifft(lib, F, vec, 1), C.ifft_radix2(F, red, log_n, 1), "raw ifft 2^%d, %s" % (log_n, name))
                _congruent(F, C.lib_ifft(lib, F, vec, s), C.ifft_radix2(F, red, log_n, s), "raw coset ifft 2^%d, %s" % (log_n, name))
                _congruent(F, C.lib_fft(lib, F, vec, log_n, 1), C.fft_radix2(F, red, log_n, 1), "raw fft 2^%d, %s" % (log_n, name))
            any_word = [(1 << 192) - 1 - 12345 * i for i in range(n)]                  # the forward coset transform pre-scales: any 192-bit word
            _congruent(F, C.lib_fft(lib, F, any_word, log_n, s), C.fft_radix2(F, [v % P for v in any_word], log_n, s), "raw coset fft 2^%d" % log_n)
        at = [edwards_raw_limit(1), 0]
        got = C.lib_ifft(lib, F, at, 1)
        want = C.ifft_radix2(F, [v % P for v in at], 1, 1)
        assert all(x < P for x in got) and got[0] == want[0] and got[1] != want[1], "n = 2 at the limit: x + 8p reaches 2^192"
        for log_n in (1, 4, 7, 12):
            n = 1 << log_n
            above = [(1 << 192) - 1 if i % 2 == 0 else (1 << 192) - 12346 for i in range(n)]
            assert all(x < P for x in C.lib_ifft(lib, F, above, 1)) and all(x < P for x in C.lib_fft(lib, F, above, log_n, 1))
        return
    top = (1 << 256) - 1
    for log_n in (1, 4, 7, 12):
        n = 1 << log_n
        for name, vec in _raw_vectors(n, 1 << 256, log_n):
            red = [v % F.P for v in vec]
            _congruent(F, C.lib_ifft(lib, F, vec, 1), C.ifft_radix2(F, red, log_n, 1), "raw ifft 2^%d, %s" % (log_n, name))
            _congruent(F, C.lib_ifft(lib, F, vec, s), C.ifft_radix2(F, red, log_n, s), "raw coset ifft 2^%d, %s" % (log_n, name))
            _congruent(F, C.lib_fft(lib, F, vec, log_n, 1), C.fft_radix2(F, red, log_n, 1), "raw fft 2^%d, %s" % (log_n, name))
            _congruent(F, C.lib_fft(lib, F, vec[:n // 2 + 1], log_n, s), C.fft_radix2(F, red[:n // 2 + 1], log_n, s), "raw coset fft 2^%d, %s" % (log_n, name))
            if log_n <= 7:
                for eta in (1, 2, 3, 4):
                    if eta <= log_n:
                        x = F.scalar("raw x")
                        _congruent(F, C.lib_fold(lib, F, vec, s, eta, x), C.fold_expected(F, red, log_n, s, eta, x), "raw fold 2^%d eta %d, %s" % (log_n, eta, name))
                coeffs = [F.scalar("raw ldt %d" % i) for i in range(4)]
                evals = [vec, [top - v for v in vec]]
                _congruent(F, C.lib_ldt(lib, F, evals, [n, n // 2 + 1], coeffs, log_n, 5),
                           C.ldt_expected(F, [[v % F.P for v in e] for e in evals], [n, n // 2 + 1], coeffs, log_n, 5), "raw ldt 2^%d, %s" % (log_n, name))
