#!/usr/bin/env python3
"""Writes tests/golden/bn128_tiny.json: small cases of every multiplicative-coset step over alt_bn128 Fr, computed with PYTHON INTEGERS
ONLY from the definitions — independent of the kernels and of oracle/:

  * multiplicative FFT over the coset shift * <g> (g = 5^((r - 1) / n), subgroup.tcc:55-59) = the polynomial's values at shift * g^i in
    natural order, by Horner's rule, for orders 2 .. 2^10, shifts 1, 5 and a seeded one, and coefficient counts 0, 1, n/2 + 1, n - 1, n
    (the degree-aware branch, fft.tcc:236-317);
  * multiplicative IFFT (fft.tcc:343-361): c_k = n^-1 shift^-k sum_i v_i g^-ik, by the definition;
  * IFFT_of_known_degree_over_field_subset (fft.tcc:435-456): the IFFT of every (n / 2^ceil(log2 degree))-th evaluation over that sub-coset;
  * FRI folds (fri_aux.tcc:106-249) for cosets of 2 .. 16, one with the challenge on a domain point: the value at x of the polynomial of
    degree < 2^eta interpolating f on each coset {j + k n / 2^eta} (subgroup.tcc:175-197), by Lagrange's formula (at a node: that value);
  * the LDT combination (ldt_reducer_aux.tcc:3-37,104-128) of three oracles, two of them submaximal: coefficients_ = {1} + random, oracle
    k weighted by coefficients_[k] and the i-th submaximal one also by coefficients_[num + i] x^(max_degree - degree_k).

Outputs are recorded as BLAKE2b-256 digests of the Montgomery words (bn128_cases.digest); inputs come from the recipes in
tests/bn128_cases.py.

    python tests/golden/make_bn128_tiny.py        (rewrites the JSON next to it)
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bn128_cases as C  # noqa: E402

P = C.P


def inv(a):
    return pow(a, P - 2, P)


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def fft(coeffs, log_n, shift):
    n = 1 << log_n
    g = C.gen(log_n)
    return [horner(coeffs, shift * pow(g, i, P) % P) for i in range(n)]


def ifft(vals, log_n, shift):
    n = len(vals)
    gi = inv(C.gen(log_n))
    ninv, sinv = inv(n), inv(shift)
    out = []
    for k in range(n):
        w = pow(gi, k, P)
        acc, t = 0, 1
        for v in vals:
            acc = (acc + v * t) % P
            t = t * w % P
        out.append(acc * ninv % P * pow(sinv, k, P) % P)
    return out


def lagrange_at(points, values, x):
    for xk, fk in zip(points, values):
        if xk == x % P:
            return fk
    acc = 0
    for k, (xk, fk) in enumerate(zip(points, values)):
        num, den = 1, 1
        for l, xl in enumerate(points):
            if l != k:
                num = num * (x - xl) % P
                den = den * (xk - xl) % P
        acc = (acc + fk * num % P * inv(den)) % P
    return acc


def fold(f, log_n, shift, eta, x):
    n, c = 1 << log_n, 1 << eta
    q = n // c
    g = C.gen(log_n)
    out = []
    for j in range(q):
        pts = [shift * pow(g, j + k * q, P) % P for k in range(c)]
        out.append(lagrange_at(pts, [f[j + k * q] for k in range(c)], x))
    return out


def ldt(evals, degrees, coeffs, log_n, shift):
    n, num = 1 << log_n, len(evals)
    co = [1] + coeffs
    top = max(degrees)
    g = C.gen(log_n)
    out = [0] * n
    sub = 0
    for k in range(num):
        bump = None
        if degrees[k] < top:
            bump = (co[num + sub], top - degrees[k])
            sub += 1
        for j in range(n):
            w = co[k]
            if bump:
                w = (w + bump[0] * pow(shift * pow(g, j, P), bump[1], P)) % P
            out[j] = (out[j] + w * evals[k][j]) % P
    return out


def main():
    assert (P - 1) % (1 << 28) == 0 and (P - 1) % (1 << 29) != 0
    assert C.gen(28) == C.OMEGA_28
    cases = {"fft": {}, "ifft": {}, "known_degree": {}, "fold": {}, "ldt": {}}
    for name, log_n, s, count in C.tiny_fft_cases():
        coeffs = C.words_to_ints(C.data_words("fft %d" % log_n, 1 << log_n)[:count])
        cases["fft"][name] = C.digest(C.ints_to_words(fft(coeffs, log_n, s)))
    for name, log_n, s in C.tiny_ifft_cases():
        vals = C.words_to_ints(C.data_words("ifft %d" % log_n, 1 << log_n))
        cases["ifft"][name] = C.digest(C.ints_to_words(ifft(vals, log_n, s)))
    for log_n, degree in C.TINY_KNOWN_DEGREE:
        vals = C.words_to_ints(C.data_words("known degree %d" % log_n, 1 << log_n))
        k = (degree - 1).bit_length()
        stride = (1 << log_n) >> k
        s = C.seeded_scalar("known degree shift")
        cases["known_degree"]["kd_%d_%d" % (log_n, degree)] = C.digest(C.ints_to_words(ifft(vals[::stride], k, s)))
    for log_n, eta, on_domain in C.TINY_FOLDS:
        f = C.words_to_ints(C.data_words("fold %d %d" % (log_n, eta), 1 << log_n))
        s = C.seeded_scalar("fold shift")
        x = C.fold_x(log_n, on_domain, s)
        cases["fold"]["fold_%d_%d_%s" % (log_n, eta, "node" if on_domain else "seeded")] = C.digest(C.ints_to_words(fold(f, log_n, s, eta, x)))
    L = C.TINY_LDT
    evals = [C.words_to_ints(C.data_words("ldt %d" % k, 1 << L["log_n"])) for k in range(len(L["degrees"]))]
    rc = [C.seeded_scalar("ldt coefficient %d" % i) for i in range(2 * len(L["degrees"]))]
    cases["ldt"]["ldt_5"] = C.digest(C.ints_to_words(ldt(evals, L["degrees"], rc, L["log_n"], C.GENERATOR)))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn128_tiny.json")
    with open(out, "w") as fh:
        json.dump({"generator": "tests/golden/make_bn128_tiny.py", "field": "alt_bn128 Fr", "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
