"""Cases for Aurora over GF(2^64): the protocol-layer entries (libiop_amd/csrc/gfx_ops.h, instantiated by gf64_ops.hip) against the function-level oracle, and the
Python prover (libiop_amd/aurora.py over domains.GF64AuroraOps) and the native one (field code 4 of the C ABI) against the oracle's prover
and verifier.  Shared by
tests/test_gf64_aurora_emu.py (CPU emulation) and tests/test_gpu_gf64_aurora.py (MI355X): every function takes the Library under test.

Every comparison is byte equality.  Elements are (n, 1) uint64 arrays.  Each kernel case runs with its vectors at a 16-byte boundary and 8
bytes past one: the entries take two elements per lane in the first placement (the profile's k64_<name>) and one in the second
(k64_<name>_w64).  The edge cases (check_small_domains, check_short_vectors, check_mixed_placements, check_aliased_outputs, check_small_grid,
check_domain_table_turnover) add the smallest domains and vectors, one argument alone off the boundary, outputs over inputs, a grid of two
or three blocks and the turnover of the library's domain tables; tests/gf64_large_cases.py has the same entries past their launch caps."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import gf64_cases as G
import oracle

U64P = ctypes.POINTER(ctypes.c_uint64)
VP = ctypes.c_void_p
BIT63 = 1 << 63
OFFSETS = (0, 8)


def xor_all(terms):
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc ^ t
    return acc


def scaled(v, c):
    """v[i] * c for one element c"""
    return oracle.gf_mul(v, np.repeat(np.asarray(c, dtype=np.uint64).reshape(1, 1), v.shape[0], axis=0))


class Device:
    """host arrays in device buffers placed `off` bytes past a 16-byte boundary; everything is freed on the way out"""

    def __init__(self, lib, off=0):
        self.lib, self.off, self.blocks = lib, off, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.blocks:
            self.lib.free(b)

    def empty(self, nbytes):
        base = self.lib.malloc(nbytes + 32)
        self.blocks.append(base)
        return base + (-base) % 16 + self.off

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.empty(max(a.nbytes, 8))
        if a.nbytes:
            self.lib.h2d(p, a)
        return p

    def get(self, p, count, dtype=np.uint64):
        out = np.empty((count, 1), dtype=dtype)
        if count:
            self.lib.d2h(out, p)
        return out


def on_device(lib, inputs, out_count, call, init=None):
    """call(pointers of the inputs, pointer of the output) at both placements; the outputs (equal) as one array"""
    results = []
    for off in OFFSETS:
        with Device(lib, off) as dev:
            ptrs = [dev.put(a) for a in inputs]
            out = dev.put(init) if init is not None else dev.empty(8 * max(out_count, 1))
            call(ptrs, out)
            results.append(dev.get(out, out_count))
    assert np.array_equal(results[0], results[1]), "the two placements disagree"
    return results[0]


# ---- domains ----
def codeword_domain(m, shifted=True):
    return G.std_basis(m), G.elem((BIT63 | 0x1234567 | (1 << m)) if shifted else 0)


def derived_domain(index):
    """non-standard bases of dimension 11, 9, 6 (gf64_cases.derived_domains)"""
    return tuple(G.derived_domains(BIT63 | 5)[index])


# ---- kernel cases ----
ROWCHECK_CASES = [(9, 4), (11, 7), (13, 13)]


def check_rowcheck(lib):
    domains = [codeword_domain(m) + (h,) for m, h in ROWCHECK_CASES] + [derived_domain(1) + (4,)]
    for basis, shift, h in domains:
        m, n = basis.shape[0], 1 << basis.shape[0]
        cshift = G.elem(0x55 if h < 7 else BIT63 >> 1)
        az, bz, cz = (G.seeded("rowcheck %s %d %d" % (t, m, h), n) for t in "abc")
        got = on_device(lib, [az, bz, cz], n, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, h, cshift, o, words=1))
        assert np.array_equal(got, oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)), (m, h)
    basis, shift = codeword_domain(4)
    with Device(lib) as dev:
        p = dev.put(G.seeded("rowcheck refused", 16))
        with pytest.raises(ValueError, match="the constraint domain must be a sub-domain of the codeword domain"):
            lib.rowcheck_dev(p, p, p, basis, shift, 5, G.elem(0), p, words=1)
        with pytest.raises(ValueError, match="the codeword domain intersects the constraint domain"):
            lib.rowcheck_dev(p, p, p, basis, G.elem(0), 2, G.elem(0), p, words=1)


def check_fz(lib):
    m = 10
    for basis, shift in (codeword_domain(m), derived_domain(1)):
        n = 1 << basis.shape[0]
        fw, f1v = G.seeded("fz w", n), G.seeded("fz 1v", n)
        for input_dim in (0, 1, 4):
            ib, ishift = basis[:input_dim], G.elem(BIT63 | 9)
            got = on_device(lib, [fw, f1v], n, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, ib, ishift, o, words=1))
            assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)), (basis.shape[0], input_dim)
    basis, shift = codeword_domain(3)
    with Device(lib) as dev:
        p = dev.put(G.seeded("fz refused", 8))
        with pytest.raises(ValueError, match="Codeword domain must be bigger than the input variable domain."):
            lib.fz_dev(p, p, basis, shift, G.std_basis(4), G.elem(0), p, words=1)


def check_sumcheck_g(lib):
    mu = G.elem(int(G.seeded("sumcheck mu", 1)[0, 0]) | BIT63)
    cases = [(m, shifted, claimed) for m in (9, 12) for shifted in (True,) for claimed in (G.elem(0), mu)]
    cases += [(9, False, G.elem(0)), (9, False, mu)]                   # unshifted: position 0 is the zero element
    for m, shifted, claimed in cases:
        basis, shift = codeword_domain(m, shifted)
        n = 1 << m
        sb, sshift = basis[:6], G.elem(0)
        f, h = G.seeded("sumcheck f %d" % m, n), G.seeded("sumcheck h %d" % m, n)
        got = on_device(lib, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, claimed, o, words=1))
        assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, claimed)), (m, shifted, int(claimed[0]))
    # a summation domain that is a shifted coset of a non-prefix span
    basis, shift = derived_domain(1)
    n = 1 << basis.shape[0]
    sb, sshift = G.std_basis(3), G.elem(BIT63 | 0x40)
    f, h = G.seeded("sumcheck f derived", n), G.seeded("sumcheck h derived", n)
    got = on_device(lib, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, mu, o, words=1))
    assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, mu))
    dep = G.std_basis(3).copy()
    dep[2] = dep[0] ^ dep[1]
    with Device(lib) as dev:
        p = dev.put(f)
        with pytest.raises(ValueError, match="the summation domain's basis is linearly dependent"):
            lib.sumcheck_g_dev(p, p, basis, shift, dep, sshift, mu, p, words=1)


def check_lincheck(lib):
    n = 1000
    fz, p1, p2 = G.seeded("lincheck fz", n), G.seeded("lincheck p1", n), G.seeded("lincheck p2", n)
    mz = [G.seeded("lincheck mz %d" % k, n) for k in range(9)]
    r = G.seeded("lincheck r", 9)
    r[1, 0] = 0
    for num in (1, 3, 8):
        got = on_device(lib, [fz, p1, p2] + mz[:num], n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r[:num], p[1], p[2], n, o, words=1))
        assert np.array_equal(got, oracle.lincheck_combine(fz, mz[:num], r[:num], p1, p2)), num
    with Device(lib) as dev:
        p = dev.put(fz)
        with pytest.raises(ValueError, match="multi_lincheck uses more constituent oracles than what was provided."):
            lib.lincheck_dev(p, [p] * 9, r, p, p, n, p, words=1)


def check_lincomb(lib):
    for n in (1000, 4097):
        vecs = [G.seeded("lincomb %d %d" % (n, k), n) for k in range(16)]
        coef = G.seeded("lincomb coef %d" % n, 16)
        coef[1, 0] = 0
        coef[2, 0] |= np.uint64(BIT63)
        constant = G.elem(int(G.seeded("lincomb constant", 1)[0, 0]))
        for num in (1, 3, 16):
            want = xor_all([scaled(v, c) for v, c in zip(vecs[:num], coef[:num])])
            got = on_device(lib, vecs[:num], n, lambda p, o: lib.lincomb_dev(p, coef[:num], n, o, words=1))
            assert np.array_equal(got, want), (n, num)
            got = on_device(lib, vecs[:num], n, lambda p, o: lib.lincomb_affine_dev(p, coef[:num], constant, n, o, words=1))
            assert np.array_equal(got, want ^ constant.reshape(1, 1)), (n, num)
    with Device(lib) as dev:
        p = dev.put(vecs[0])
        many = G.seeded("lincomb 17", 17)
        for call in (lambda: lib.lincomb_dev([p] * 17, many, 8, p, words=1), lambda: lib.lincomb_affine_dev([p] * 17, many, constant, 8, p, words=1)):
            with pytest.raises(ValueError, match="Expected same number of evaluations as in registration."):
                call()


def _spmv(lib, row_ptr, col, coeff, vec, rows, scale=None, accumulate=False, init=None):
    def call(p, o):
        lib.spmv_dev(p[0], p[1], p[2], rows, p[3], o, scale=scale, accumulate=accumulate, words=1)
    return on_device(lib, [np.asarray(row_ptr, dtype=np.uint64), np.asarray(col, dtype=np.uint32), coeff, vec], rows, call, init=init)


def check_spmv(lib):
    # the seeded instance's Az, Bz, Cz (r1cs_examples.tcc:23-78: one entry per row; C's column 0 is the constant)
    log_n, k, seed = 8, 15, 0x2204
    n = 1 << log_n
    matrices, z = example_csr(log_n, k, seed)
    bad, Az, Bz, Cz = oracle.r1cs_check_csr(oracle.FIELD_GF64, matrices, n - 1, k, z)
    assert bad == 0
    vec = np.concatenate([np.ones((1, 1), dtype=np.uint64), z])
    for (rp, col, coef), want in zip(matrices, (Az, Bz, Cz)):
        assert np.array_equal(_spmv(lib, rp, col, coef, vec, n), want)
    # by hand: an empty row, a 100-entry row, column 0, more rows than one workgroup
    rows, cols = 300, 128
    rng = np.random.default_rng(64)
    lengths = rng.integers(0, 4, size=rows)
    lengths[3], lengths[7] = 0, 100
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, cols, size=int(row_ptr[-1])).astype(np.uint32)
    col[int(row_ptr[7])] = 0
    coef, vec = G.seeded("spmv coef", col.shape[0]), G.seeded("spmv vec", cols)
    prod = oracle.gf_mul(coef, vec[col])
    want = np.zeros((rows, 1), dtype=np.uint64)
    for r in range(rows):
        for t in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            want[r] ^= prod[t]
    assert not want[3].any() and want[7].any()
    assert np.array_equal(_spmv(lib, row_ptr, col, coef, vec, rows), want)
    scale, old = G.elem(int(G.seeded("spmv scale", 1)[0, 0]) | BIT63), G.seeded("spmv old", rows)
    assert np.array_equal(_spmv(lib, row_ptr, col, coef, vec, rows, scale=scale), scaled(want, scale))
    assert np.array_equal(_spmv(lib, row_ptr, col, coef, vec, rows, accumulate=True, init=old), want ^ old)
    assert np.array_equal(_spmv(lib, row_ptr, col, coef, vec, rows, scale=scale, accumulate=True, init=old), scaled(want, scale) ^ old)


def _poly_mul(a, b):
    """the product of two coefficient vectors over gf64 (schoolbook, through oracle.gf_mul)"""
    out = np.zeros((a.shape[0] + b.shape[0] - 1, 1), dtype=np.uint64)
    for i in range(b.shape[0]):
        if b[i, 0]:
            out[i:i + a.shape[0]] ^= scaled(a, b[i])
    return out


def _vanishing_coefficients(basis, shift):
    """Z_S for S = span(basis) + shift as 2^dim + 1 coefficients: prod_{s in S} (X + s)"""
    z = np.ones((1, 1), dtype=np.uint64)
    points = oracle.all_subset_sums(basis, shift) if basis.shape[0] else np.asarray(shift, dtype=np.uint64).reshape(1, 1)
    for s in points:
        z = _poly_mul(z, np.array([[int(s[0])], [1]], dtype=np.uint64))
    return z


def check_poly_div_vanishing(lib):
    big_basis, big_shift = codeword_domain(9)
    for basis, shift in ((G.std_basis(6), G.elem(BIT63 | 0x80)), (G.std_basis(6), G.elem(0)), (derived_domain(2)[0], derived_domain(2)[1])):
        N = 1 << basis.shape[0]
        Z = _vanishing_coefficients(basis, shift)
        assert Z.shape[0] == N + 1 and int(Z[N, 0]) == 1
        for n_coeffs in (N, N + 1, 2 * N, 4 * N - 3):
            poly = G.seeded("polydiv %d %d" % (int(shift[0]) & 0xFF, n_coeffs), n_coeffs)
            M = n_coeffs - N
            got = on_device(lib, [poly], M, lambda p, o: lib.poly_div_vanishing_dev(p[0], n_coeffs, basis, shift, o, words=1))
            assert got.shape[0] == M
            if M == 0:
                continue
            # multiplying back: Q Z + R = P with deg R < N, as evaluations on a domain of 2^9 points
            remainder = poly ^ _poly_mul(got, Z)
            assert not remainder[N:].any(), (n_coeffs, "the remainder has degree >= |H|")
            ev = lambda c: oracle.additive_fft(c, big_basis, big_shift)
            zq = oracle.gf_mul(ev(got), ev(Z))
            assert np.array_equal(zq ^ ev(remainder[:N]), ev(poly)), n_coeffs


def check_pow_table(lib):
    base = G.elem(int(G.seeded("pow base", 1)[0, 0]) | BIT63)
    init = G.elem(int(G.seeded("pow init", 1)[0, 0]))
    for count in (1, 257, 4097):
        for b, i0 in ((G.elem(1), init), (base, G.elem(1)), (base, init)):
            got = on_device(lib, [], count, lambda p, o: lib.pow_table_dev(o, count, b, i0, words=1))
            want = np.empty((count, 1), dtype=np.uint64)
            cur = i0.reshape(1, 1)
            for l in range(count):
                want[l] = cur[0]
                cur = oracle.gf_mul(cur, b.reshape(1, 1))
            assert np.array_equal(got, want), (count, int(b[0]))


def check_add(lib):
    for n in (1, 4097):
        a, b = G.seeded("add a %d" % n, n), G.seeded("add b %d" % n, n)
        assert np.array_equal(on_device(lib, [a, b], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=1)), a ^ b)


# ---- edges of the same entries: the smallest domains, short and odd vectors, one argument off the 16-byte boundary, outputs over inputs ----
def check_small_domains(lib):
    """m = 0 and m = 1 (at n = 1 the pair form's second element is absent), h = 0 and h = m, input_dim = m, summation_dim = 0"""
    mu = G.elem(int(G.seeded("sumcheck mu", 1)[0, 0]) | BIT63)
    for m, h in ((0, 0), (1, 0), (1, 1), (9, 0), (9, 9)):
        basis, shift = codeword_domain(m)
        n = 1 << m
        cshift = G.elem(BIT63 >> 1)
        az, bz, cz = (G.seeded("small rowcheck %s %d" % (t, m), n) for t in "abc")
        got = on_device(lib, [az, bz, cz], n, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, h, cshift, o, words=1))
        assert np.array_equal(got, oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)), (m, h)
    for m, input_dim in ((0, 0), (1, 0), (1, 1), (10, 10)):
        basis, shift = codeword_domain(m)
        n = 1 << m
        ib, ishift = basis[:input_dim], G.elem(BIT63 | 9)
        fw, f1v = G.seeded("small fz w %d" % m, n), G.seeded("small fz 1v %d" % m, n)
        got = on_device(lib, [fw, f1v], n, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, ib, ishift, o, words=1))
        assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)), (m, input_dim)
    for m, sdim in ((0, 0), (1, 0), (1, 1), (9, 0)):
        for shifted in (True, False):                                  # unshifted: position 0 is the zero element
            for claimed in (G.elem(0), mu):
                basis, shift = codeword_domain(m, shifted)
                n = 1 << m
                sb, sshift = basis[:sdim], G.elem(BIT63 | 0x40)
                f, h = G.seeded("small sumcheck f %d" % m, n), G.seeded("small sumcheck h %d" % m, n)
                got = on_device(lib, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, claimed, o, words=1))
                assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, claimed)), (m, sdim, shifted, int(claimed[0]))


def check_short_vectors(lib):
    """n in {1, 2, 3, 511, 513} for the vector entries, two and three powers, division by X + s and by one coefficient more than |H|"""
    for n in (1, 2, 3, 511, 513):
        a, b = G.seeded("short add a %d" % n, n), G.seeded("short add b %d" % n, n)
        assert np.array_equal(on_device(lib, [a, b], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=1)), a ^ b), n
        vecs = [G.seeded("short lincomb %d %d" % (n, k), n) for k in range(3)]
        coef, constant = G.seeded("short lincomb coef", 3), G.elem(int(G.seeded("lincomb constant", 1)[0, 0]))
        want = xor_all([scaled(v, c) for v, c in zip(vecs, coef)])
        assert np.array_equal(on_device(lib, vecs, n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=1)), want), n
        assert np.array_equal(on_device(lib, vecs, n, lambda p, o: lib.lincomb_affine_dev(p, coef, constant, n, o, words=1)), want ^ constant.reshape(1, 1)), n
        fz, p1, p2 = (G.seeded("short lincheck %s %d" % (t, n), n) for t in ("fz", "p1", "p2"))
        mz, r = [G.seeded("short lincheck mz %d %d" % (n, k), n) for k in range(2)], G.seeded("short lincheck r", 2)
        got = on_device(lib, [fz, p1, p2] + mz, n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r, p[1], p[2], n, o, words=1))
        assert np.array_equal(got, oracle.lincheck_combine(fz, mz, r, p1, p2)), n
    base, init = G.elem(int(G.seeded("pow base", 1)[0, 0]) | BIT63), G.elem(int(G.seeded("pow init", 1)[0, 0]))
    for count in (2, 3):
        got = on_device(lib, [], count, lambda p, o: lib.pow_table_dev(o, count, base, init, words=1))
        want = [init.reshape(1, 1)]
        while len(want) < count:
            want.append(oracle.gf_mul(want[-1], base.reshape(1, 1)))
        assert np.array_equal(got, np.concatenate(want)), count
    big_basis, big_shift = codeword_domain(9)
    ev = lambda c: oracle.additive_fft(c, big_basis, big_shift)
    for basis, shift, counts in ((G.std_basis(0), G.elem(BIT63 | 0x80), (1, 2, 3, 300)), (G.std_basis(0), G.elem(0), (2, 257)), (G.std_basis(6), G.elem(BIT63 | 0x80), (65,))):
        N = 1 << basis.shape[0]
        Z = _vanishing_coefficients(basis, shift)
        assert Z.shape[0] == N + 1 and int(Z[N, 0]) == 1
        for n_coeffs in counts:
            poly = G.seeded("short polydiv %d %d" % (N, n_coeffs), n_coeffs)
            M = n_coeffs - N
            got = on_device(lib, [poly], M, lambda p, o: lib.poly_div_vanishing_dev(p[0], n_coeffs, basis, shift, o, words=1))
            assert got.shape[0] == M
            if M == 0:
                continue
            remainder = poly ^ _poly_mul(got, Z)
            assert not remainder[N:].any(), (N, n_coeffs, "the remainder has degree >= |H|")
            assert np.array_equal(oracle.gf_mul(ev(got), ev(Z)) ^ ev(remainder[:N]), ev(poly)), (N, n_coeffs)


def run_placed(lib, inputs, out_count, call, offsets, alias=None):
    """call(pointers of the inputs, pointer of the output) with input i placed offsets[i] bytes past a 16-byte boundary and the output offsets[-1]
    past one, or over input `alias`; (the output, the library's profile of the call)"""
    with Device(lib) as dev:
        ptrs = []
        for a, off in zip(inputs, offsets):
            dev.off = off
            ptrs.append(dev.put(a))
        dev.off = offsets[-1]
        out = ptrs[alias] if alias is not None else dev.empty(8 * max(out_count, 1))
        lib.profile_begin()
        call(ptrs, out)
        prof = lib.profile_report()
        return dev.get(out, out_count), prof


def pair_form_entries(lib, n=513, m=9):
    """(profile label, inputs, output length, call) of every entry of the protocol layer that has a two-elements-per-lane form, at a length that
    ends in half a pair (513) or on a domain of 2^9"""
    basis, shift = codeword_domain(m)
    mu = G.elem(int(G.seeded("sumcheck mu", 1)[0, 0]) | BIT63)
    coef, constant, r = G.seeded("placed lincomb coef", 3), G.elem(int(G.seeded("lincomb constant", 1)[0, 0])), G.seeded("placed lincheck r", 2)
    vec = lambda tag, count: [G.seeded("placed %s %d" % (tag, k), count) for k in range(5)]
    sb, sshift = basis[:6], G.elem(0)
    return [
        ("k64_add", vec("add", n)[:2], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=1)),
        ("k64_lincomb", vec("lincomb", n)[:3], n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=1)),
        ("k64_lincomb", vec("affine", n)[:3], n, lambda p, o: lib.lincomb_affine_dev(p, coef, constant, n, o, words=1)),
        ("k64_lincheck", vec("lincheck", n), n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r, p[1], p[2], n, o, words=1)),
        ("k64_rowcheck", vec("rowcheck", 1 << m)[:3], 1 << m, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, 4, G.elem(0x55), o, words=1)),
        ("k64_fz", vec("fz", 1 << m)[:2], 1 << m, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, basis[:4], G.elem(BIT63 | 9), o, words=1)),
        ("k64_sumcheck_g_zero_sum", vec("sumcheck 0", 1 << m)[:2], 1 << m,
         lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, G.elem(0), o, words=1)),
        ("k64_sumcheck_g", vec("sumcheck mu", 1 << m)[:2], 1 << m, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, mu, o, words=1)),
    ]


def one_form_entries(lib, n):
    """the same of the entries that take one element per lane wherever their vectors lie (one kernel, one profile label): the powers of a base, the
    CSR product and one division pass exactly (|H| / 2 < n <= |H|: the passes of a longer division alternate with a temporary of the library's)"""
    base, init = G.elem(int(G.seeded("pow base", 1)[0, 0]) | BIT63), G.elem(int(G.seeded("pow init", 1)[0, 0]))
    rng = np.random.default_rng(n)
    lengths = rng.integers(0, 4, size=n)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, 64, size=int(row_ptr[-1])).astype(np.uint32)
    dbasis, dshift = G.std_basis(max(n - 1, 0).bit_length()), G.elem(BIT63 | 0x80)
    dN = 1 << dbasis.shape[0]

    def spmv(p, o):
        with Device(lib) as dev:            # the CSR offsets and columns are not element vectors: they sit in buffers of their own, aligned
            lib.spmv_dev(dev.put(row_ptr), dev.put(col), p[0], n, p[1], o, words=1)
            lib.synchronize()
    return [
        ("k64_pow_table", [], n, lambda p, o: lib.pow_table_dev(o, n, base, init, words=1)),
        ("k64_spmv", [G.seeded("placed spmv coef", col.shape[0]), G.seeded("placed spmv vec", 64)], n, spmv),
        ("k64_polydiv_pass", [G.seeded("placed polydiv", n + dN)], n, lambda p, o: lib.poly_div_vanishing_dev(p[0], n + dN, dbasis, dshift, o, words=1)),
    ]


def launches(prof, label):
    """(launches of the 16-byte form, launches of the 64-bit-word form) of one kernel in a profile"""
    return prof.get(label, (0,))[0], prof.get(label + "_w64", (0,))[0]


def _for_each_entry(lib, body):
    for label, inputs, out_count, call in pair_form_entries(lib):
        aligned, prof = run_placed(lib, inputs, out_count, call, [0] * (len(inputs) + 1))
        assert launches(prof, label) == (1, 0), (label, "all aligned: one launch of the two-element form", launches(prof, label))
        body(label, inputs, out_count, call, aligned)


def check_mixed_placements(lib):
    """exactly one vector, each argument in turn and the output last, 8 bytes past a 16-byte boundary: the entry takes one element per lane
    (the profile's label + "_w64", and no launch under the plain label), launches once and returns the all-aligned result"""
    def body(label, inputs, out_count, call, aligned):
        for which in range(len(inputs) + 1):
            offsets = [8 if i == which else 0 for i in range(len(inputs) + 1)]
            got, prof = run_placed(lib, inputs, out_count, call, offsets)
            assert launches(prof, label) == (0, 1), (label, which, launches(prof, label))
            assert np.array_equal(got, aligned), (label, which)
    _for_each_entry(lib, body)


def check_aliased_outputs(lib):
    """the output over each input in turn, at both placements: every entry here is elementwise (position j of the output depends on position j
    of the inputs), and the provers call them that way.  One launch in all, under the name of the placement's form."""
    def body(label, inputs, out_count, call, aligned):
        for off in OFFSETS:
            for which in range(len(inputs)):
                got, prof = run_placed(lib, inputs, out_count, call, [off] * (len(inputs) + 1), alias=which)
                assert launches(prof, label) == ((1, 0) if off == 0 else (0, 1)), (label, off, which, launches(prof, label))
                assert np.array_equal(got, aligned), (label, off, which)
    _for_each_entry(lib, body)


def check_small_grid(lib):
    """IOPX_GFX_OPS_MAX_BLOCKS = 2 and vectors of 2 * (2 * 256 * 2) + 3 = 2051 elements: the two-element form takes a third trip round its
    grid-stride loop that ends in half a pair, the one-element form a fifth trip of 3.  A domain has 2^m points, so the domain-shaped entries
    (the head route's division by Z_S among them) run 2^12 points under a cap of 3 blocks: 1536 per trip of the two-element form (the third
    trip has 1024), 768 per trip of the other (the sixth has 256).  Every entry, at both placements, launches once under the name of its form
    and returns what it returns under the default grid, with the output apart and, for the elementwise entries, over the first input (a loop that
    visited a position twice would then work on its own output); lincomb and fz equal the oracle's results under the cap too."""
    n, m = 2 * (2 * 256 * 2) + 3, 12
    N = 1 << m
    basis, shift = codeword_domain(m)
    div = ("k64_div_by_vanishing", [G.seeded("placed div", N)], N, lambda p, o: lib.div_by_vanishing(p[0], basis, shift, 4, G.elem(0x55), o, words=1))
    paired = [(e, True) for e in pair_form_entries(lib, n, m) + [div]]
    for cap, count, entries in ((2, n, paired + [(e, False) for e in one_form_entries(lib, n)]), (3, N, paired)):
        ran = 0
        for (label, inputs, out_count, call), two_forms in entries:
            if out_count != count:
                continue
            ran += 1
            want, _ = run_placed(lib, inputs, out_count, call, [0] * (len(inputs) + 1))
            with options(lib, IOPX_GFX_OPS_MAX_BLOCKS=cap):
                for off in OFFSETS:
                    got, prof = run_placed(lib, inputs, out_count, call, [off] * (len(inputs) + 1))
                    assert launches(prof, label) == ((0, 1) if off and two_forms else (1, 0)), (label, cap, off, launches(prof, label))
                    assert np.array_equal(got, want), (label, cap, off)
                    if two_forms:       # the output over the first input: a stride of fewer than V elements per lane would process a position twice
                        got, _ = run_placed(lib, inputs, out_count, call, [off] * (len(inputs) + 1), alias=0)
                        assert np.array_equal(got, want), (label, cap, off, "aliased")
        assert ran == (7 if cap == 2 else 5), (cap, ran)      # add, lincomb, affine lincomb, lincheck, pow_table, spmv, division | rowcheck, fz, two sumchecks, div
    with options(lib, IOPX_GFX_OPS_MAX_BLOCKS=2):
        vecs, coef = [G.seeded("grid lincomb %d" % k, n) for k in range(2)], G.seeded("grid coef", 2)
        got = on_device(lib, vecs, n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=1))
        assert np.array_equal(got, xor_all([scaled(v, c) for v, c in zip(vecs, coef)]))
    with options(lib, IOPX_GFX_OPS_MAX_BLOCKS=3):
        fw, f1v = G.seeded("grid fz w", N), G.seeded("grid fz v", N)
        got = on_device(lib, [fw, f1v], N, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, basis[:3], G.elem(5), o, words=1))
        assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, basis[:3], G.elem(5)))


def check_domain_table_turnover(lib):
    """70 distinct codeword domains in a row through fz_dev (the library keeps the tables of 64 pairs of domains), then the first again"""
    m = 6
    basis, n = G.std_basis(m), 1 << m
    ib, ishift = basis[:2], G.elem(BIT63 | 9)
    fw, f1v = G.seeded("turnover w", n), G.seeded("turnover 1v", n)
    shifts = [G.elem(BIT63 | ((t + 1) << 8)) for t in range(70)]
    with Device(lib) as dev:
        pw, pf, out = dev.put(fw), dev.put(f1v), dev.empty(8 * n)
        first = None
        for shift in shifts + shifts[:1]:
            lib.fz_dev(pw, pf, basis, shift, ib, ishift, out, words=1)
            got = dev.get(out, n)
            assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)), int(shift[0])
            first = got if first is None else first
        assert np.array_equal(got, first)


def check_null_pointers(lib):
    """every entry refuses null pointers with its gf192 twin's message"""
    c = lib.c
    basis, shift = G.std_basis(4), G.elem(BIT63)
    bp, sp = basis.ctypes.data_as(U64P), shift.ctypes.data_as(U64P)
    b3 = oracle.standard_basis(4, 3)
    s3 = np.array([0, 0, 1], dtype=np.uint64)
    dom = {"gf64": (bp, sp), "gf192": (b3.ctypes.data_as(U64P), s3.ctypes.data_as(U64P))}
    one = VP(8)
    calls = [
        lambda g: getattr(c, "iopx_%s_add_dev" % g)(None, one, one, 4),
        lambda g: getattr(c, "iopx_%s_add_dev" % g)(one, one, None, 4),
        lambda g: getattr(c, "iopx_%s_pow_table_dev" % g)(None, 4, dom[g][1], dom[g][1]),
        lambda g: getattr(c, "iopx_%s_pow_table_dev" % g)(one, 4, None, dom[g][1]),
        lambda g: getattr(c, "iopx_lincomb_%s_dev" % g)(None, 1, dom[g][1], 4, one),
        lambda g: getattr(c, "iopx_lincomb_%s_dev" % g)((VP * 1)(None), 1, dom[g][1], 4, one),
        lambda g: getattr(c, "iopx_lincomb_affine_%s_dev" % g)((VP * 1)(8), 1, dom[g][1], None, 4, one),
        lambda g: getattr(c, "iopx_spmv_%s_dev" % g)(one, one, None, 4, one, None, 0, one),
        lambda g: getattr(c, "iopx_lincheck_%s_dev" % g)(one, None, 1, dom[g][1], one, one, 4, one),
        lambda g: getattr(c, "iopx_lincheck_%s_dev" % g)(one, (VP * 1)(8), 1, None, one, one, 4, one),
        lambda g: getattr(c, "iopx_rowcheck_%s_dev" % g)(one, one, None, dom[g][0], 4, dom[g][1], 2, dom[g][1], one),
        lambda g: getattr(c, "iopx_rowcheck_%s_dev" % g)(one, one, one, None, 4, dom[g][1], 2, dom[g][1], one),
        lambda g: getattr(c, "iopx_fz_%s_dev" % g)(one, None, dom[g][0], 4, dom[g][1], dom[g][0], 2, dom[g][1], one),
        lambda g: getattr(c, "iopx_fz_%s_dev" % g)(one, one, dom[g][0], 4, dom[g][1], None, 2, dom[g][1], one),
        lambda g: getattr(c, "iopx_sumcheck_g_%s_dev" % g)(one, one, dom[g][0], 4, dom[g][1], dom[g][0], 2, dom[g][1], None, one),
        lambda g: getattr(c, "iopx_sumcheck_g_%s_dev" % g)(None, one, dom[g][0], 4, dom[g][1], dom[g][0], 2, dom[g][1], dom[g][1], one),
        lambda g: getattr(c, "iopx_poly_div_vanishing_%s_dev" % g)(None, 40, dom[g][0], 4, dom[g][1], one),
        lambda g: getattr(c, "iopx_poly_div_vanishing_%s_dev" % g)(one, 40, dom[g][0], 4, None, one),
    ]
    for k, call in enumerate(calls):
        msgs = []
        for g in ("gf192", "gf64"):
            with pytest.raises(ValueError, match="null") as e:
                lib._check(call(g))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], (k, msgs)


# ---- the Python prover ----
PYTHON_TUPLES = [(6, 3, 0x2204, 5, 2), (8, 15, 0x2204, 5, 2), (9, 1, 0x2204, 5, 2), (7, 3, 7, 3, 3), (7, 7, 8, 2, 1)]      # (log_n, inputs, seed, rs_extra, localization)


def aurora_ops(lib, torch, device):
    from libiop_amd import domains
    ops = domains.GF64AuroraOps(lib, torch, device, domains.GF64())
    assert isinstance(ops, domains.GF64DeviceOps)
    assert type(domains.DeviceOps(lib, torch, device, domains.GF64())) is domains.GF64DeviceOps      # the plain construction keeps its class
    return ops


def python_prove(lib, torch, device, log_n, num_inputs, seed, rs_extra=5, localization=2):
    from libiop_amd import aurora, r1cs
    ops = aurora_ops(lib, torch, device)
    n = 1 << log_n
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, num_inputs, n - 1, seed)
    params = aurora.AuroraParameters(ops.field, n, n - 1, num_inputs, RS_extra_dimensions=rs_extra, FRI_localization_parameter=localization)
    return aurora.aurora_snark_prover(ops, cs, primary, auxiliary, params), params


def check_parameters():
    """the repetition counts no 24-byte field reaches, against the oracle's"""
    from libiop_amd import aurora, domains
    for log_n, k, _, rs_extra, loc in PYTHON_TUPLES + [(16, 15, 0, 5, 2)]:
        n = 1 << log_n
        mine = aurora.AuroraParameters(domains.GF64(), n, n - 1, k, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
        want = oracle.aurora_params(oracle.FIELD_GF64, log_n, k, rs_extra=rs_extra, localization=loc)
        for name in ("codeword_domain_dim", "pow_bits", "multi_lincheck_repetitions", "num_output_LDT_instances", "fri_interactive_repetitions",
                     "fri_query_repetitions", "absolute_proximity_parameter"):
            assert getattr(mine, name) == want[name], (log_n, name)
        assert list(mine.localization_parameters) == want["localization_parameters"]
        assert mine.multi_lincheck_repetitions == 3 and mine.fri_interactive_repetitions == 3
        assert mine.num_output_LDT_instances == (4 if log_n >= 16 else 3)
    last = aurora.AuroraParameters(domains.GF64(), 128, 127, 7, RS_extra_dimensions=2, FRI_localization_parameter=1)
    assert (last.codeword_domain_dim, last.fri_query_repetitions) == (9, 119)


def check_python_prover(lib, torch, device, case):
    log_n, k, seed, rs_extra, loc = case
    transcript, _ = python_prove(lib, torch, device, log_n, k, seed, rs_extra, loc)
    mine = transcript.serialize()
    ref = oracle.aurora_prove(oracle.FIELD_GF64, log_n, k, seed, rs_extra=rs_extra, localization=loc)
    if mine != ref:
        first = next((i for i, (a, b) in enumerate(zip(mine, ref)) if a != b), min(len(mine), len(ref)))
        raise AssertionError("transcript differs from the oracle prover's at byte %d (lengths %d / %d)" % (first, len(mine), len(ref)))
    assert oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, seed, mine, rs_extra=rs_extra, localization=loc)
    if case == PYTHON_TUPLES[0]:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript_digests.json")) as f:
            pins = [e for e in json.load(f)["aurora"] if e["field"] == "gf64" and (e["log_n"], e["num_inputs"], e["seed"]) == (log_n, k, seed)]
        assert len(pins) == 1
        assert len(mine) == pins[0]["bytes"] and hashlib.sha256(mine).hexdigest() == pins[0]["sha256"]


def check_tampering(lib, torch, device):
    import aurora_cases
    log_n, k, seed = 7, 3, 11
    transcript, _ = python_prove(lib, torch, device, log_n, k, seed)
    assert oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, seed, transcript.serialize())
    cases = aurora_cases.tamper_cases(transcript)
    assert len(cases) == 7
    for label, data in cases:
        assert not oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, seed, data), label
    wrong = oracle.r1cs_example(oracle.FIELD_GF64, log_n, k, seed)[0][:k].copy()
    wrong[1, 0] ^= np.uint64(1)
    assert not oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, seed, transcript.serialize(), primary_override=wrong)


def check_unsatisfied_witness(lib, torch, device):
    """a witness that violates one constraint: the prover runs as over gf192 and the oracle's verifier rejects the proof"""
    from libiop_amd import aurora, r1cs
    log_n, k, seed = 6, 3, 5
    n = 1 << log_n
    ops = aurora_ops(lib, torch, device)
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, k, n - 1, seed)
    params = aurora.AuroraParameters(ops.field, n, n - 1, k)
    auxiliary = auxiliary.copy()
    auxiliary[17, 0] ^= np.uint64(BIT63)
    bad = aurora.aurora_snark_prover(ops, cs, primary, auxiliary, params).serialize()
    assert not oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, seed, bad)


def check_fractal_operators_refused(lib, torch, device):
    ops = aurora_ops(lib, torch, device)
    for name in ("div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine", "rational_sumcheck_constraint"):
        with pytest.raises(NotImplementedError, match="gf64"):
            getattr(ops, name)(None, None, None, None, None, None)
    # lincomb_affine is the one operator of Fractal's that the class allows (its entry shares the kernel of lincomb) and the prover never calls
    vecs, coef, constant = [G.seeded("ops affine %d" % k, 100) for k in range(3)], G.seeded("ops affine coef", 3), G.seeded("ops affine constant", 1)
    got = ops.download(ops.lincomb_affine([ops.upload(v) for v in vecs], coef, constant[0], 100))
    assert np.array_equal(got, xor_all([scaled(v, c) for v, c in zip(vecs, coef)]) ^ constant)


def check_other_fields_unchanged(lib, torch, device):
    """the Python prover over GF192 and EdwardsFr still returns the oracle's bytes"""
    import aurora_cases
    aurora_cases.check_transcript_equals_oracle(lib, torch, device, "gf192", 6, 3, 0x2204, rs_extra=3, localization=2)
    aurora_cases.check_transcript_equals_oracle(lib, torch, device, "edwards_Fr", 7, 7, 0x2204, rs_extra=2, localization=3)


# ---- the native prover (libiop_amd/csrc/prover_capi.hip, field code 4) ----
NATIVE_TUPLES = [(7, 15), (9, 15), (7, 0)]          # (log_n, inputs) at seed 0x2204, default rate and localization
SEED = 0x2204


def example_csr(log_n, num_inputs, seed):
    """the seeded instance as CSR triples (r1cs_examples.tcc:23-78: one entry per row; C's column 0 is the constant) and its assignment"""
    n = 1 << log_n
    z, c_idx, c_coef = oracle.r1cs_example(oracle.FIELD_GF64, log_n, num_inputs, seed)
    i = np.arange(n)
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    ones = np.ones((n, 1), dtype=np.uint64)
    return [(row_ptr, (i % (n - 1) + 1).astype(np.uint32), ones), (row_ptr, ((i + 7) % (n - 1) + 1).astype(np.uint32), ones),
            (row_ptr, c_idx.astype(np.uint32), c_coef)], z


def hand_built_system():
    """(matrices, assignment, inputs, rs_extra, localization): 64 constraints over 63 variables, (z_a + c1 z_a') * (c2 z_b or the constant c2)
    = coef z_c with coef chosen so that the seeded assignment satisfies it"""
    n, num_inputs = 64, 3
    z = G.seeded("hand-built z", n - 1)
    z[z == 0] = 1
    full = np.concatenate([np.ones((1, 1), dtype=np.uint64), z])
    i = np.arange(n)
    a1, a2, b, c = i % (n - 1) + 1, (3 * i + 5) % (n - 1) + 1, np.where(i % 5 == 0, 0, (i + 11) % (n - 1) + 1), (2 * i + 1) % (n - 1) + 1
    c1, c2 = G.seeded("hand-built c1", n), G.seeded("hand-built c2", n)
    az = full[a1] ^ oracle.gf_mul(c1, full[a2])
    bz = oracle.gf_mul(c2, full[b])
    coef = oracle.gf_mul(oracle.gf_mul(az, bz), oracle.gf_inv(full[c]))
    A = (2 * np.arange(n + 1, dtype=np.uint64), np.stack([a1, a2], axis=1).reshape(-1).astype(np.uint32),
         np.stack([np.ones((n, 1), dtype=np.uint64), c1], axis=1).reshape(-1, 1))
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    matrices = [A, (row_ptr, b.astype(np.uint32), c2), (row_ptr, c.astype(np.uint32), coef)]
    assert oracle.r1cs_check_csr(oracle.FIELD_GF64, matrices, n - 1, num_inputs, z)[0] == 0
    return matrices, z, num_inputs, 3, 2


class options:
    def __init__(self, lib, **values):
        self.lib, self.values = lib, values

    def __enter__(self):
        for k, v in self.values.items():
            self.lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.lib.clear_option(k)


def _first_difference(mine, ref):
    return next((i for i, (a, b) in enumerate(zip(mine, ref)) if a != b), min(len(mine), len(ref))), len(mine), len(ref)


def check_native_prover(lib, case):
    import libiop_amd as la
    log_n, k = case
    n = 1 << log_n
    ref = oracle.aurora_prove(oracle.FIELD_GF64, log_n, k, SEED)
    inst = lib.aurora_example_instance(la.FIELD_GF64, n, k, n - 1, SEED)
    try:
        for head_eval in (1, 0):                    # gf64 runs the reference's schedule either way
            with options(lib, IOPX_HEAD_EVAL=head_eval):
                mine = lib.aurora_prove(inst)
                assert mine == ref, (head_eval,) + _first_difference(mine, ref)
        assert lib.aurora_prove(inst, hash=la.HASH_BLAKE2B) == ref
        lib.aurora_instance_warm(inst)
    finally:
        lib.aurora_instance_free(inst)
    assert oracle.aurora_verify(oracle.FIELD_GF64, log_n, k, SEED, mine)
    if case == NATIVE_TUPLES[0]:                    # the caller's own system: CSR plus assignment
        matrices, z = example_csr(log_n, k, SEED)
        inst = lib.aurora_instance(la.FIELD_GF64, matrices, n - 1, k, z)
        try:
            mine = lib.aurora_prove(inst)
        finally:
            lib.aurora_instance_free(inst)
        assert mine == oracle.aurora_prove_csr(oracle.FIELD_GF64, matrices, n - 1, k, z) == ref


def check_native_unsatisfied_witness(lib):
    """one auxiliary element changed: the prover emits the transcript the oracle's prover emits for it, with IOPX_HEAD_EVAL set either way (as
    over gf192), and the oracle's verifier rejects it"""
    import libiop_amd as la
    matrices, z, k, rs_extra, loc = hand_built_system()
    bad = z.copy()
    bad[k + 11, 0] ^= np.uint64(1)
    assert oracle.r1cs_check_csr(oracle.FIELD_GF64, matrices, z.shape[0], k, bad)[0] > 0
    want = oracle.aurora_prove_csr(oracle.FIELD_GF64, matrices, z.shape[0], k, bad, rs_extra=rs_extra, localization=loc)
    inst = lib.aurora_instance(la.FIELD_GF64, matrices, z.shape[0], k, bad)
    try:
        for head_eval in (1, 0):
            with options(lib, IOPX_HEAD_EVAL=head_eval):
                mine = lib.aurora_prove(inst, 128, rs_extra, loc)
                assert mine == want, (head_eval,) + _first_difference(mine, want)
    finally:
        lib.aurora_instance_free(inst)
    assert not oracle.aurora_verify_csr(oracle.FIELD_GF64, matrices, z.shape[0], k, bad[:k], want, rs_extra=rs_extra, localization=loc)
    good = oracle.aurora_prove_csr(oracle.FIELD_GF64, matrices, z.shape[0], k, z, rs_extra=rs_extra, localization=loc)
    assert oracle.aurora_verify_csr(oracle.FIELD_GF64, matrices, z.shape[0], k, z[:k], good, rs_extra=rs_extra, localization=loc)


def check_native_fri_snark(lib):
    import libiop_amd as la
    from libiop_amd import domains, r1cs
    for (dim, rs_extra, loc, interactions, queries), size in G.FRI_SNARK_TUPLES:
        coeffs = r1cs.seeded_elements(domains.GF64(), 5, 1 << (dim - rs_extra))
        with Device(lib) as dev:
            d = dev.put(coeffs)
            mine = lib.fri_snark_prove(la.FIELD_GF64, d, coeffs.shape[0], dim, rs_extra, loc, interactions, queries)
            assert mine == lib.fri_snark_prove(la.FIELD_GF64, d, coeffs.shape[0], dim, rs_extra, loc, interactions, queries, hash=la.HASH_BLAKE2B)
        ref = oracle.fri_snark_prove(oracle.FIELD_GF64, dim, rs_extra, loc, interactions, queries, 5)
        assert len(ref) == size and mine == ref, (dim,) + _first_difference(mine, ref)


def check_native_refusals(lib):
    import libiop_amd as la
    inst = lib.aurora_example_instance(la.FIELD_GF64, 128, 3, 127, SEED)
    comm = lib.comm_create_replay(0, 1)
    try:
        with pytest.raises(ValueError, match="gf64 has no distributed prover"):
            lib.aurora_prove_dist(inst, comm)
        with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over gf64"):
            lib.fractal_index(inst)
        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over gf64"):
            lib.fractal_prove(inst)
        for h in (la.HASH_POSEIDON_STARKWARE, la.HASH_POSEIDON_HIGH_ALPHA):
            with pytest.raises(ValueError, match="gf64 proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only"):
                lib.aurora_prove(inst, hash=h)
        with pytest.raises(ValueError, match="security_parameter 100 is not supported"):
            lib.aurora_prove(inst, 100)
        with pytest.raises(ValueError, match="codeword domain dimension 41: the gf64 transforms take domains of dimension up to 40"):
            lib.aurora_prove(inst, 128, 34, 2)
        with Device(lib) as dev:
            d = dev.put(G.seeded("refused fri", 16))
            with pytest.raises(ValueError, match="codeword domain dimension 41: the gf64 transforms take domains of dimension up to 40"):
                lib.fri_snark_prove(la.FIELD_GF64, d, 16, 41, 2)
            with pytest.raises(ValueError, match="gf64 has no distributed prover"):
                lib.fri_snark_prove(la.FIELD_GF64, d, 16, 8, 2, comm=comm)
            with pytest.raises(ValueError, match="gf64 proves with BLAKE2b"):
                lib.fri_snark_prove(la.FIELD_GF64, d, 16, 8, 2, hash=la.HASH_POSEIDON_STARKWARE)
        assert lib.aurora_prove(inst) == oracle.aurora_prove(oracle.FIELD_GF64, 7, 3, SEED)          # the instance still proves after the refusals
    finally:
        lib.comm_destroy(comm)
        lib.aurora_instance_free(inst)


def check_native_other_fields_unchanged(lib):
    """gf192 (6, 3; rate 3, localization 2) and edwards Fr (7, 7; 2, 3) through the native prover still equal the oracle's bytes"""
    import libiop_amd as la
    for code, ocode, log_n, k, rs_extra, loc in ((la.FIELD_GF192, oracle.FIELD_GF192, 6, 3, 3, 2), (la.FIELD_EDWARDS_FR, oracle.FIELD_EDWARDS, 7, 7, 2, 3)):
        n = 1 << log_n
        inst = lib.aurora_example_instance(code, n, k, n - 1, SEED)
        try:
            assert lib.aurora_prove(inst, 128, rs_extra, loc) == oracle.aurora_prove(ocode, log_n, k, SEED, rs_extra=rs_extra, localization=loc), code
        finally:
            lib.aurora_instance_free(inst)


def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gf64_aurora.json")) as f:
        return {(e["log_n"], e["num_inputs"]): e for e in json.load(f)["aurora"] if e["field"] == "gf64" and e["seed"] == SEED}


def check_native_digest(lib, log_n, k):
    import libiop_amd as la
    pin = golden_digests()[(log_n, k)]
    n = 1 << log_n
    inst = lib.aurora_example_instance(la.FIELD_GF64, n, k, n - 1, SEED)
    try:
        mine = lib.aurora_prove(inst)
    finally:
        lib.aurora_instance_free(inst)
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])


def check_python_digest(lib, torch, device, log_n, k):
    pin = golden_digests()[(log_n, k)]
    mine = python_prove(lib, torch, device, log_n, k, SEED)[0].serialize()
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])
