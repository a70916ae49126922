"""The dev:: layer of libiop_amd/cpp instantiated for gf192_element, edwards_Fr_element and alt_bn128_Fr_element (tests/cpp/test_field_ops.cpp):
every C entry it reaches is picked by the dispatch table of cpp/field_ops.hpp, so each output is compared in full with values computed here from
integers alone -- never with the library's own host scalars, which go through the same table and could agree with a misrouted entry.

Prime fields: model() of bn128_protocol_cases.py for the operations it covers; the transforms, the fold, the LDT combination (and everything over
GF(2^192), through helpers.gf_mul_int) from the definitions below.  A 32-byte instantiation that reached a 24-byte entry would show as wrong values from
index 1 on (the element stride differs); the output length is checked as well.

Shapes: codeword domain 2^6 and sub-domain 2^3, both shifted; a 24-coefficient polynomial; three constituent oracles; a 5 x 8 matrix with an empty row."""
import os
import subprocess

import numpy as np
import pytest

import bn128_cases as B
import bn128_protocol_cases as P
import helpers
import libiop_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_L, LOG_H, N_POLY, FOLD, DEGREES = 6, 3, 24, 4, [64, 40, 7]
MATRIX_COLS, MATRIX_ROW_LEN, MATRIX_WIDTH = [0, 1, 2, 3, 4, 5, 7], [2, 0, 1, 3, 1], 8       # as in test_field_ops.cpp
SCALARS = ["L shift", "H shift", "point", "constant", "base", "init", "scale", "mu", "x_i", "c0", "c1", "c2",
           "l0", "l1", "l2", "l3", "l4", "l5", "spmv scale"]


class Prime:
    """plain residues; stored as Montgomery words"""
    additive = False

    def __init__(self, F):
        self.F, self.p, self.words = F, F.p, F.words

    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def mul(self, a, b):
        return a * b % self.p

    def inv(self, a):
        return pow(a, self.p - 2, self.p)

    def draw(self, tag):
        return B.seeded_scalar("field ops " + self.F.name + " " + tag) % self.p

    def points(self, log_n, shift):
        g = self.F.gen(log_n)
        return [shift * pow(g, i, self.p) % self.p for i in range(1 << log_n)]

    def coset_positions(self, n, size, j):                                          # subgroup.tcc:175-197
        return [j + k * (n // size) for k in range(size)]

    def stored(self, vals):
        if self.words == 4:
            return B.ints_to_words([B.mont(v) for v in vals])
        return libiop_amd.edwards_to_montgomery(vals)


class Binary:
    """GF(2^192) elements as integers (polynomial basis), stored as they are"""
    additive, words = True, 3

    def add(self, a, b):
        return a ^ b

    sub = add

    def mul(self, a, b):
        return helpers.gf_mul_int(a, b, 3)

    def inv(self, a):                                                               # a^(2^192 - 2)
        r, sq = 1, a
        for _ in range(191):
            sq = self.mul(sq, sq)
            r = self.mul(r, sq)
        return r

    def draw(self, tag):
        return B.seeded_scalar("field ops gf192 " + tag) & ((1 << 192) - 1)

    def points(self, log_n, shift):                                                 # standard basis: index i <-> shift + i
        return [shift ^ i for i in range(1 << log_n)]

    def coset_positions(self, n, size, j):                                          # subspace.tcc:73-91
        return [j * size + k for k in range(size)]

    def stored(self, vals):
        return np.array([helpers.from_int(v, 3) for v in vals], dtype=np.uint64).reshape(-1, 3)


def inv_many(A, vals):
    """the inverses of non-zero vals with one field inversion"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = A.mul(acc, v)
    inv, out = A.inv(acc), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = A.mul(inv, pre[i])
        inv = A.mul(inv, vals[i])
    return out


def power(A, x, e):
    r = 1
    for _ in range(e):
        r = A.mul(r, x)
    return r


def summed(A, terms):
    acc = 0
    for t in terms:
        acc = A.add(acc, t)
    return acc


def vanishing(A, S, x):
    """Z_S(x) = prod_{s in S} (x - s)"""
    r = 1
    for s in S:
        r = A.mul(r, A.sub(x, s))
    return r


def vanishing_coefficients(A, S):
    poly = [1]
    for s in S:                                                                     # times (X - s)
        poly = [A.sub(lo, A.mul(s, hi)) for lo, hi in zip([0] + poly, poly + [0])]
    return poly


def horner(A, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = A.add(A.mul(acc, x), c)
    return acc


def inputs(A):
    sc = {k: A.draw(k) for k in SCALARS}
    vec = lambda tag, n: [A.draw("%s %d" % (tag, i)) for i in range(n)]            # noqa: E731
    data = {"a": vec("a", 64), "b": vec("b", 64), "c": vec("c", 64), "poly": vec("poly", N_POLY), "m": vec("m", len(MATRIX_COLS)), "x": vec("x", MATRIX_WIDTH)}
    return sc, data


def expected(A, sc, d):
    """[(name, values)] in the order test_field_ops.cpp writes them"""
    a, b, c, poly = d["a"], d["b"], d["c"], d["poly"]
    L, H = A.points(LOG_L, sc["L shift"]), A.points(LOG_H, sc["H shift"])
    n, comb, ldt = len(L), [sc["c0"], sc["c1"], sc["c2"]], [sc["l%d" % i] for i in range(6)]
    b_inv, ZH = inv_many(A, b), [vanishing(A, H, x) for x in L]
    out = [("sub", [A.sub(u, v) for u, v in zip(a, b)]),
           ("mul", [A.mul(u, v) for u, v in zip(a, b)]),
           ("div", [A.mul(u, v) for u, v in zip(a, b_inv)]),
           ("div without a numerator", b_inv),
           ("pow_table", [A.mul(sc["init"], power(A, sc["base"], i)) for i in range(64)]),
           ("scaled", [A.mul(sc["scale"], u) for u in a]),
           ("lincomb_affine", [summed(A, [A.mul(k, v) for k, v in zip(comb, col)] + [sc["constant"]]) for col in zip(a, b, c)]),
           ("domain_offsets", [A.sub(sc["point"], x) for x in L]),
           ("domain_elements", L),
           ("vanishing_evals", [A.sub(sc["constant"], z) for z in ZH])]
    Z, rem, quotient = vanishing_coefficients(A, H), list(poly), [0] * (N_POLY - len(H))     # long division by the monic Z_H
    for k in range(len(quotient) - 1, -1, -1):
        quotient[k] = rem[k + len(H)]
        for i, z in enumerate(Z):
            rem[k + i] = A.sub(rem[k + i], A.mul(quotient[k], z))
    evals = [horner(A, poly, x) for x in L]
    out += [("poly_div_vanishing", quotient), ("FFT", evals), ("IFFT of the FFT", poly + [0] * (n - N_POLY)), ("IFFT_of_known_degree", poly + [0] * (32 - N_POLY))]
    folded = []                                                                     # fri_aux.tcc: the interpolant of f on each coset, at x_i
    for j in range(n // FOLD):
        pos = A.coset_positions(n, FOLD, j)
        pts = [L[t] for t in pos]
        dens = inv_many(A, [vanishing(A, pts[:k] + pts[k + 1:], pts[k]) for k in range(FOLD)])
        folded.append(summed(A, [A.mul(A.mul(a[pos[k]], vanishing(A, pts[:k] + pts[k + 1:], sc["x_i"])), dens[k]) for k in range(FOLD)]))
    ZH_inv, L_inv = inv_many(A, ZH), inv_many(A, L)
    if A.additive:                                                                  # sumcheck.tcc:58-119: f - eps^-1 mu x^(|H| - 1) - Z_H h
        eps = vanishing(A, A.points(LOG_H, 0)[1:], 0)                               # the linear coefficient of Z_H: the product of span(H) \ {0}
        m = A.mul(sc["mu"], A.inv(eps))
        g = [A.sub(A.sub(f, A.mul(m, power(A, x, len(H) - 1))), A.mul(z, h)) for f, h, x, z in zip(a, b, L, ZH)]
    else:                                                                           # (f - mu / |H| - Z_H h) / x
        m = A.mul(sc["mu"], A.inv(len(H)))
        g = [A.mul(A.sub(A.sub(f, m), A.mul(z, h)), xi) for f, h, xi, z in zip(a, b, L_inv, ZH)]
    # ldt_reducer_aux.tcc:26-131: coefficients_ = {1} + the random ones; oracle k is weighted by coefficients_[k], the i-th submaximal one
    # also by coefficients_[3 + i] x^(max degree - its degree)
    co, top, sub_i, combined = [1] + ldt, max(DEGREES), 0, [0] * n
    for k, (col, deg) in enumerate(zip((a, b, c), DEGREES)):
        for t in range(n):
            w = co[k] if deg == top else A.add(co[k], A.mul(co[3 + sub_i], power(A, L[t], top - deg)))
            combined[t] = A.add(combined[t], A.mul(w, col[t]))
        sub_i += deg != top
    out += [("fold", folded),
            ("rowcheck", [A.mul(A.sub(A.mul(u, v), w), zi) for u, v, w, zi in zip(a, b, c, ZH_inv)]),
            ("sumcheck_g", g),
            ("random_linear_combination", [summed(A, [A.mul(k, v) for k, v in zip(comb, col)]) for col in zip(a, b, c)]),
            ("combined_LDT", combined)]
    rows, t = [], 0
    for ln in MATRIX_ROW_LEN:
        rows.append(summed(A, [A.mul(d["m"][t + i], d["x"][MATRIX_COLS[t + i]]) for i in range(ln)]))
        t += ln
    out += [("times_vector", rows), ("times_vector, scaled and accumulated", [A.add(r, A.mul(sc["spmv scale"], r)) for r in rows])]
    return out


def model_expected(A, sc, d):
    """the same outputs from model() of bn128_protocol_cases.py, for the operations it covers (prime fields)"""
    F = A.F
    w = {k: A.stored(v) for k, v in d.items()}
    dom = {"log_n": LOG_L, "shift": sc["L shift"], "sub_log": LOG_H, "sub_shift": sc["H shift"]}
    comb = [sc["c0"], sc["c1"], sc["c2"]]
    abc = {"m0": w["a"], "m1": w["b"], "m2": w["c"]}
    rp = np.concatenate([[0], np.cumsum(MATRIX_ROW_LEN)]).astype(np.uint64)
    spmv = {"row_ptr": rp, "col": np.array(MATRIX_COLS, dtype=np.uint32), "coeff": w["m"], "vec": w["x"], "out": A.stored([0] * 5)}
    cases = {"sub": ({"op": "sub", "n": 64}, w), "mul": ({"op": "mul", "n": 64}, w),
             "div": ({"op": "div", "n": 64, "with_num": 1}, w), "div without a numerator": ({"op": "div", "n": 64, "with_num": 0}, w),
             "pow_table": ({"op": "pow_table", "n": 64, "base": sc["base"], "init": sc["init"]}, {}),
             "scaled": ({"op": "lincomb", "n": 64, "num": 1, "coeffs": [sc["scale"]]}, abc),
             "lincomb_affine": ({"op": "lincomb_affine", "n": 64, "num": 3, "coeffs": comb, "constant": sc["constant"]}, abc),
             "domain_offsets": (dict(dom, op="domain_offsets", point=sc["point"]), {}),
             "vanishing_evals": (dict(dom, op="vanishing_evals", constant=sc["constant"]), {}),
             "poly_div_vanishing": ({"op": "poly_div_vanishing", "n_coeffs": N_POLY, "sub_log": LOG_H, "shift": sc["H shift"]}, {"a": w["poly"]}),
             "rowcheck": (dict(dom, op="rowcheck"), w), "sumcheck_g": (dict(dom, op="sumcheck_g", mu=sc["mu"]), w),
             "random_linear_combination": ({"op": "lincomb", "n": 64, "num": 3, "coeffs": comb}, abc),
             "times_vector": ({"op": "spmv", "rows": 5, "scale": None, "accumulate": 0}, spmv)}
    return {name: P.model(F, case, inp)[0] for name, (case, inp) in cases.items()}


FIELDS = {"gf192": Binary, "edwards": lambda: Prime(P.ED), "bn128": lambda: Prime(P.BN)}


def _run(tmp_path, lib_dir, lib_file):
    exe = str(tmp_path / "field_ops")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + ROOT, os.path.join(ROOT, "tests", "cpp", "test_field_ops.cpp"),
                           "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    for name, make in FIELDS.items():
        A = make()
        sc, d = inputs(A)
        want = expected(A, sc, d)
        if not A.additive:
            by_model = model_expected(A, sc, d)
            for op, vals in want:                                                   # the two integer computations agree before either is used
                assert op not in by_model or by_model[op] == vals, (name, op)
        work = tmp_path / name
        work.mkdir()
        flat = [sc[k] for k in SCALARS] + d["a"] + d["b"] + d["c"] + d["poly"] + d["m"] + d["x"]
        A.stored(flat).tofile(str(work / "in.bin"))
        r = subprocess.run([exe, str(work), name], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "field ops ok" in r.stdout, name + ": " + r.stdout + r.stderr
        got = np.fromfile(str(work / "out.bin"), dtype=np.uint64)
        assert got.size == A.words * sum(len(v) for _, v in want), "%s: %d output words for %d elements" % (name, got.size, sum(len(v) for _, v in want))
        got, at = got.reshape(-1, A.words), 0
        for op, vals in want:
            assert np.array_equal(got[at:at + len(vals)], A.stored(vals)), "%s: %s differs" % (name, op)
            at += len(vals)


def test_field_ops_on_the_cpu_build(tmp_path):
    from emu_lib import emu
    emu()
    _run(tmp_path, os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so")


@pytest.mark.gpu
def test_field_ops_on_the_gpu(tmp_path):
    _run(tmp_path, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH))
