#!/usr/bin/env python3
"""Writes tests/golden/bn128_function_digests_large.json: BLAKE2b-256 digests (whole output and per 2^16-element chunk) of the full-size
alt_bn128 Fr multiplicative-coset recipes of tests/bn128_cases.py, computed with PYTHON INTEGERS ONLY (an iterative radix-2 number-theoretic
transform and the two-point fold formula) — independent of the kernels and of oracle/.  For each m in DIGEST_LOGS:

  * lde:    the first 2^min(20, m - 2) seeded coefficients evaluated over 5 * <g>, |<g>| = 2^m (multiplicative_FFT, fft.tcc:236-317);
  * fft:    2^m seeded coefficients over 5 * <g> (the square transform);
  * ifft:   the coefficients of 2^m seeded evaluations over 5 * <g> (multiplicative_IFFT, fft.tcc:343-361);
  * fold_k: the localization-2 fold chain of `fft`'s codeword (fri_aux.tcc:106-249, cosets of 2): level k folds the level k - 1 codeword
            over 5^(2^(k-1)) * <g^(2^(k-1))> at the seeded challenge fold_chain_challenge(k), down to 2^(m - 6) points; each level is
            f'(y) = (f(s) + f(-s)) / 2 + x (f(s) - f(-s)) / (2 s) for the pair {s, -s} over y = s^2.

    python tests/golden/make_bn128_digests_large.py        (minutes: rewrites the JSON next to it)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bn128_cases as C  # noqa: E402

P = C.P


def ntt(a, w):
    """a[i] -> sum_k a[k] w^(ik), natural order in and out, len(a) a power of two"""
    n = len(a)
    a = list(a)
    j = 0
    for i in range(1, n):
        bit = n >> 1
        while j & bit:
            j ^= bit
            bit >>= 1
        j |= bit
        if i < j:
            a[i], a[j] = a[j], a[i]
    length = 2
    while length <= n:
        wl = pow(w, n // length, P)
        half = length >> 1
        tw = [1] * half
        for k in range(1, half):
            tw[k] = tw[k - 1] * wl % P
        for start in range(0, n, length):
            for k in range(half):
                u = a[start + k]
                v = a[start + k + half] * tw[k] % P
                a[start + k] = (u + v) % P
                a[start + k + half] = (u - v) % P
        length <<= 1
    return a


def coset_fft(coeffs, log_n, shift):
    n = 1 << log_n
    c = [0] * n
    t = 1
    for k, v in enumerate(coeffs):
        c[k] = v * t % P
        t = t * shift % P
    return ntt(c, C.gen(log_n))


def coset_ifft(vals, log_n, shift):
    n = 1 << log_n
    c = ntt(vals, pow(C.gen(log_n), P - 2, P))
    ninv, sinv = pow(n, P - 2, P), pow(shift, P - 2, P)
    t = ninv
    for k in range(n):
        c[k] = c[k] * t % P
        t = t * sinv % P
    return c


def fold2(f, log_n, shift, x):
    """one fold with cosets {j, j + n/2}: points s = shift g^j and -s"""
    n = 1 << log_n
    half = n >> 1
    g = C.gen(log_n)
    inv2 = pow(2, P - 2, P)
    ginv = pow(g, P - 2, P)
    out = [0] * half
    xs = x * pow(shift, P - 2, P) % P          # x / s for s = shift g^j
    for j in range(half):
        a, b = f[j], f[j + half]
        out[j] = ((a + b) + (a - b) * xs) % P * inv2 % P
        xs = xs * ginv % P
    return out


def record(a):
    w = C.ints_to_words(a)
    return {"n": len(a), "digest": C.digest(w), "chunks": C.chunk_digests(w)}


def recipes(m):
    """(name, ints) for every output of the size-2^m recipes"""
    lde_k = min(C.LDE_LOG_COEFFS, m - 2)
    coeffs = C.words_to_ints(C.data_words("large coeffs %d" % m, 1 << m))
    yield "lde", coset_fft(coeffs[:1 << lde_k], m, C.LDE_SHIFT)
    code = coset_fft(coeffs, m, C.LDE_SHIFT)
    yield "fft", code
    yield "ifft", coset_ifft(C.words_to_ints(C.data_words("large evals %d" % m, 1 << m)), m, C.LDE_SHIFT)
    shifts = C.fold_chain_shifts(C.LDE_SHIFT, 6)
    cur = code
    for level in range(1, 7):
        cur = fold2(cur, m - level + 1, shifts[level - 1], C.fold_chain_challenge(level))
        yield "fold_%d" % level, cur


def main():
    t0 = time.time()
    out = {"generator": "tests/golden/make_bn128_digests_large.py", "field": "alt_bn128 Fr", "chunk_log": C.CHUNK_LOG, "cases": {}}
    for m in C.DIGEST_LOGS:
        for name, vals in recipes(m):
            out["cases"]["%s_%d" % (name, m)] = record(vals)
            print("m=%d %s done at %.0f s" % (m, name, time.time() - t0), flush=True)
    out["generation_seconds"] = round(time.time() - t0, 1)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn128_function_digests_large.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
