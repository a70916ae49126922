"""Cases for Aurora over GF(2^128) and GF(2^256), parametrised by the words per element W in {2, 4}: the protocol-layer entries of
libiop_amd/csrc/gfx_ops.h (gf128_ops.hip, gf256_ops.hip) against the function-level oracle, and the Python prover (libiop_amd/aurora.py over
domains.GF128AuroraOps / GF256AuroraOps) and the native one (field codes 5 and 6 of the C ABI) against tests/gfx_aurora_model.py.  Shared by
tests/test_gfx_aurora_emu.py (CPU emulation) and tests/test_gpu_gfx_aurora.py (MI355X): every function takes the Library under test.

Every comparison is byte equality of whole vectors or transcripts.  Elements are (n, W) uint64 arrays.  Each kernel case runs with its
vectors at a 16-byte boundary and 8 bytes past one: the entries move an element in 128-bit accesses in the first placement and in 64-bit
words in the second (the profile's "_w64" names).

The oracle has no prover and no verifier over these fields, so the expected transcripts are the model's (trusted after it reproduced the
oracle at one and three words: tests/test_gfx_aurora_emu.py) and tamper-rejection tests are out of scope."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import gfx_aurora_model as M
import oracle

U64P = ctypes.POINTER(ctypes.c_uint64)
VP = ctypes.c_void_p
OFFSETS = (0, 8)
WORDS = (2, 4)
NAME = {2: "gf128", 4: "gf256"}
STEM = {2: "k128_", 4: "k256_"}


def field_code(W):
    import libiop_amd as la
    return {2: la.FIELD_GF128, 4: la.FIELD_GF256}[W]


def seeded(tag, n, W):
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(("%s/%d" % (tag, W)).encode()).digest()[:8], "little")))
    return rng.integers(0, 1 << 64, size=(n, W), dtype=np.uint64)


def elem(W, v):
    return M.elem(W, v)


def top(W):
    return 1 << (64 * W - 1)


def one_seeded(tag, W, force_top=False):
    e = seeded(tag, 1, W)[0].copy()
    if force_top:
        e[W - 1] |= np.uint64(1 << 63)
    return e


def xor_all(terms):
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc ^ t
    return acc


scaled = M.scaled


class Device:
    """host arrays in device buffers placed `off` bytes past a 16-byte boundary; everything is freed on the way out"""

    def __init__(self, lib, W, off=0):
        self.lib, self.W, self.off, self.blocks = lib, W, off, []

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

    def get(self, p, count):
        out = np.empty((count, self.W), dtype=np.uint64)
        if count:
            self.lib.d2h(out, p)
        return out


def on_device(lib, W, inputs, out_count, call, init=None):
    """call(pointers of the inputs, pointer of the output) at both placements; the outputs (equal) as one array"""
    results = []
    for off in OFFSETS:
        with Device(lib, W, off) as dev:
            ptrs = [dev.put(a) for a in inputs]
            out = dev.put(init) if init is not None else dev.empty(8 * W * max(out_count, 1))
            call(ptrs, out)
            results.append(dev.get(out, out_count))
    assert np.array_equal(results[0], results[1]), "the two placements disagree"
    return results[0]


# ---- domains ----
def codeword_domain(m, W, shifted=True):
    return oracle.standard_basis(m, W), elem(W, (top(W) | 0x1234567 | (1 << m)) if shifted else 0)


def derived_domain(W, dim=9):
    """a non-standard basis: seeded elements (independent with overwhelming probability; the transforms are not involved here)"""
    return seeded("derived basis", dim, W), one_seeded("derived shift", W, True)


# ---- kernel cases ----
def check_rowcheck(lib, W):
    domains = [codeword_domain(m, W) + (h,) for m, h in ((8, 4), (9, 7), (10, 10))] + [derived_domain(W) + (4,)]
    for basis, shift, h in domains:
        m, n = basis.shape[0], 1 << basis.shape[0]
        cshift = elem(W, 0x55 if h < 7 else top(W) >> 1)
        az, bz, cz = (seeded("rowcheck %s %d %d" % (t, m, h), n, W) for t in "abc")
        got = on_device(lib, W, [az, bz, cz], n, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, h, cshift, o, words=W))
        assert np.array_equal(got, oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)), (m, h)
    basis, shift = codeword_domain(4, W)
    with Device(lib, W) as dev:
        p = dev.put(seeded("rowcheck refused", 16, W))
        with pytest.raises(ValueError, match="the constraint domain must be a sub-domain of the codeword domain"):
            lib.rowcheck_dev(p, p, p, basis, shift, 5, elem(W, 0), p, words=W)
        with pytest.raises(ValueError, match="the codeword domain intersects the constraint domain"):
            lib.rowcheck_dev(p, p, p, basis, elem(W, 0), 2, elem(W, 0), p, words=W)


def check_fz(lib, W):
    for basis, shift in (codeword_domain(10, W), derived_domain(W)):
        n = 1 << basis.shape[0]
        fw, f1v = seeded("fz w", n, W), seeded("fz 1v", n, W)
        for input_dim in (0, 1, 4):
            ib, ishift = basis[:input_dim], elem(W, top(W) | 9)
            got = on_device(lib, W, [fw, f1v], n, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, ib, ishift, o, words=W))
            assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)), (basis.shape[0], input_dim)
    basis, shift = codeword_domain(3, W)
    with Device(lib, W) as dev:
        p = dev.put(seeded("fz refused", 8, W))
        with pytest.raises(ValueError, match="Codeword domain must be bigger than the input variable domain."):
            lib.fz_dev(p, p, basis, shift, oracle.standard_basis(4, W), elem(W, 0), p, words=W)


def check_sumcheck_g(lib, W):
    mu = one_seeded("sumcheck mu", W, True)
    cases = [(m, True, claimed) for m in (8, 10) for claimed in (elem(W, 0), mu)]
    cases += [(9, False, elem(W, 0)), (9, False, mu)]                  # unshifted: position 0 is the zero element, whose inverse is taken as zero
    for m, shifted, claimed in cases:
        basis, shift = codeword_domain(m, W, shifted)
        n = 1 << m
        sb, sshift = basis[:6], elem(W, 0)
        f, h = seeded("sumcheck f %d" % m, n, W), seeded("sumcheck h %d" % m, n, W)
        got = on_device(lib, W, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, claimed, o, words=W))
        assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, claimed)), (m, shifted, claimed.any())
    # a summation domain that is a shifted coset of a non-prefix span
    basis, shift = derived_domain(W)
    n = 1 << basis.shape[0]
    sb, sshift = oracle.standard_basis(3, W), elem(W, top(W) | 0x40)
    f, h = seeded("sumcheck f derived", n, W), seeded("sumcheck h derived", n, W)
    got = on_device(lib, W, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, mu, o, words=W))
    assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, mu))
    dep = oracle.standard_basis(3, W).copy()
    dep[2] = dep[0] ^ dep[1]
    with Device(lib, W) as dev:
        p = dev.put(f)
        with pytest.raises(ValueError, match="the summation domain's basis is linearly dependent"):
            lib.sumcheck_g_dev(p, p, basis, shift, dep, sshift, mu, p, words=W)


def check_lincheck(lib, W):
    n = 1000
    fz, p1, p2 = seeded("lincheck fz", n, W), seeded("lincheck p1", n, W), seeded("lincheck p2", n, W)
    mz = [seeded("lincheck mz %d" % k, n, W) for k in range(9)]
    r = seeded("lincheck r", 9, W)
    r[1] = 0
    for num in (1, 3, 8):
        got = on_device(lib, W, [fz, p1, p2] + mz[:num], n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r[:num], p[1], p[2], n, o, words=W))
        assert np.array_equal(got, oracle.lincheck_combine(fz, mz[:num], r[:num], p1, p2)), num
    with Device(lib, W) as dev:
        p = dev.put(fz)
        with pytest.raises(ValueError, match="multi_lincheck uses more constituent oracles than what was provided."):
            lib.lincheck_dev(p, [p] * 9, r, p, p, n, p, words=W)


def check_lincomb(lib, W):
    n = 1000
    vecs = [seeded("lincomb %d" % k, n, W) for k in range(16)]
    coef = seeded("lincomb coef", 16, W)
    coef[1] = 0
    coef[2, W - 1] |= np.uint64(1 << 63)
    constant = one_seeded("lincomb constant", W)
    for num in (1, 3, 16):
        want = xor_all([scaled(v, c) for v, c in zip(vecs[:num], coef[:num])])
        got = on_device(lib, W, vecs[:num], n, lambda p, o: lib.lincomb_dev(p, coef[:num], n, o, words=W))
        assert np.array_equal(got, want), num
        got = on_device(lib, W, vecs[:num], n, lambda p, o: lib.lincomb_affine_dev(p, coef[:num], constant, n, o, words=W))
        assert np.array_equal(got, want ^ constant.reshape(1, W)), num
    with Device(lib, W) as dev:
        p = dev.put(vecs[0])
        many = seeded("lincomb 17", 17, W)
        for call in (lambda: lib.lincomb_dev([p] * 17, many, 8, p, words=W), lambda: lib.lincomb_affine_dev([p] * 17, many, constant, 8, p, words=W)):
            with pytest.raises(ValueError, match="Expected same number of evaluations as in registration."):
                call()


def _spmv(lib, W, row_ptr, col, coeff, vec, rows, scale=None, accumulate=False, init=None):
    def call(p, o):
        lib.spmv_dev(p[0], p[1], p[2], rows, p[3], o, scale=scale, accumulate=accumulate, words=W)
    return on_device(lib, W, [np.asarray(row_ptr, dtype=np.uint64), np.asarray(col, dtype=np.uint32), coeff, vec], rows, call, init=init)


def spmv_reference(row_ptr, col, coef, vec, rows):
    prod = oracle.gf_mul(coef, vec[col])
    want = np.zeros((rows, coef.shape[1]), dtype=np.uint64)
    for r in range(rows):
        for t in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            want[r] ^= prod[t]
    return want


def spmv_system(W, rows=300, cols=128, seed=64):
    """an empty row, a 100-entry row, column 0, more rows than one workgroup"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 4, size=rows)
    lengths[3], lengths[7] = 0, 100
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, cols, size=int(row_ptr[-1])).astype(np.uint32)
    col[int(row_ptr[7])] = 0
    return row_ptr, col, seeded("spmv coef", col.shape[0], W), seeded("spmv vec", cols, W)


def short_spmv_system(W, rows, cols=40):
    """`rows` rows of 0 to 3 entries (the last row never empty), any number of rows from one up"""
    rng = np.random.default_rng(1000 + rows)
    lengths = rng.integers(0, 4, size=rows)
    lengths[-1] = 2
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, cols, size=int(row_ptr[-1])).astype(np.uint32)
    return row_ptr, col, seeded("short spmv coef %d" % rows, col.shape[0], W), seeded("short spmv vec", cols, W)


def check_spmv(lib, W):
    rows = 300
    row_ptr, col, coef, vec = spmv_system(W, rows)
    want = spmv_reference(row_ptr, col, coef, vec, rows)
    assert not want[3].any() and want[7].any()
    assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, rows), want)
    scale, old = one_seeded("spmv scale", W, True), seeded("spmv old", rows, W)
    assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, rows, scale=scale), scaled(want, scale))
    assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, rows, accumulate=True, init=old), want ^ old)
    assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, rows, scale=scale, accumulate=True, init=old), scaled(want, scale) ^ old)
    # the seeded instance's Az: one entry per row
    inst = M.example(W, 8, 15, SEED)
    zfull = np.concatenate([elem(W, 1).reshape(1, W), inst["z"]])
    for rp, cl, cf in inst["matrices"]:
        assert np.array_equal(_spmv(lib, W, rp, cl, cf, zfull, 256), spmv_reference(rp, cl, cf, zfull, 256))


def check_poly_div_vanishing(lib, W):
    """the quotient against the model's division (oracle products): dividing Q Z + R gives Q back"""
    for basis, shift in ((oracle.standard_basis(6, W), elem(W, top(W) | 0x80)), (oracle.standard_basis(6, W), elem(W, 0)), (seeded("polydiv basis", 5, W), one_seeded("polydiv shift", W))):
        N = 1 << basis.shape[0]
        for n_coeffs in (N, N + 1, 2 * N, 4 * N - 3, 9 * N + 1):
            poly = seeded("polydiv %d" % n_coeffs, n_coeffs, W)
            Mq = n_coeffs - N
            got = on_device(lib, W, [poly], Mq, lambda p, o: lib.poly_div_vanishing_dev(p[0], n_coeffs, basis, shift, o, words=W))
            assert got.shape[0] == Mq
            assert np.array_equal(got, M.div_vanishing(poly, n_coeffs, basis, shift)), (N, n_coeffs)
    # the model's division itself: Q Z + R = P as evaluations (Z's values through the oracle's row check: a b / Z with b = 1, c = 0)
    basis, shift = oracle.standard_basis(4, W), elem(W, top(W) | 0x80)
    big, bshift = codeword_domain(8, W)
    poly = seeded("polydiv identity", 100, W)
    q = M.div_vanishing(poly, 100, basis, shift)
    ev = lambda c: oracle.additive_fft(c, big, bshift)      # noqa: E731
    ones = np.ascontiguousarray(np.broadcast_to(elem(W, 1), (256, W)))
    # P / Z - Q = R / Z on the codeword domain, R of degree below 16: (P + Q Z) Z^-1 Z = R
    pz = oracle.rowcheck_additive(ev(poly), ones, np.zeros((256, W), dtype=np.uint64), big, bshift, 4, shift)       # P / Z
    r_over_z = pz ^ ev(q)
    zvals = oracle.gf_inv(oracle.rowcheck_additive(ones, ones, np.zeros((256, W), dtype=np.uint64), big, bshift, 4, shift))
    rem = oracle.additive_ifft(oracle.gf_mul(r_over_z, zvals), big, bshift)
    assert not rem[16:].any(), "the remainder has degree >= |H|"


def pow_reference(base, init, count):
    return scaled(M.powers(base, count), init)


def check_pow_table(lib, W):
    base, init = one_seeded("pow base", W, True), one_seeded("pow init", W)
    for count in (1, 2, 3, 257, 1000):
        for b, i0 in ((elem(W, 1), init), (base, elem(W, 1)), (base, init)):
            got = on_device(lib, W, [], count, lambda p, o: lib.pow_table_dev(o, count, b, i0, words=W))
            assert np.array_equal(got, pow_reference(b, i0, count)), count


def check_add(lib, W):
    for n in (1, 4097):
        a, b = seeded("add a %d" % n, n, W), seeded("add b %d" % n, n, W)
        assert np.array_equal(on_device(lib, W, [a, b], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=W)), a ^ b)


# ---- edges: the smallest domains, short and odd vectors ----
def check_small_domains(lib, W):
    """m = 0 and m = 1, h = 0 and h = m, input_dim = m, summation_dim = 0"""
    mu = one_seeded("sumcheck mu", W, True)
    for m, h in ((0, 0), (1, 0), (1, 1), (8, 0), (8, 8)):
        basis, shift = codeword_domain(m, W)
        n = 1 << m
        cshift = elem(W, top(W) >> 1)
        az, bz, cz = (seeded("small rowcheck %s %d" % (t, m), n, W) for t in "abc")
        got = on_device(lib, W, [az, bz, cz], n, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, h, cshift, o, words=W))
        assert np.array_equal(got, oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)), (m, h)
    for m, input_dim in ((0, 0), (1, 0), (1, 1), (9, 9)):
        basis, shift = codeword_domain(m, W)
        n = 1 << m
        ib, ishift = basis[:input_dim], elem(W, top(W) | 9)
        fw, f1v = seeded("small fz w %d" % m, n, W), seeded("small fz 1v %d" % m, n, W)
        got = on_device(lib, W, [fw, f1v], n, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, ib, ishift, o, words=W))
        assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)), (m, input_dim)
    for m, sdim in ((0, 0), (1, 0), (1, 1), (8, 0)):
        for shifted in (True, False):                                  # unshifted: position 0 is the zero element
            for claimed in (elem(W, 0), mu):
                basis, shift = codeword_domain(m, W, shifted)
                n = 1 << m
                sb, sshift = basis[:sdim], elem(W, top(W) | 0x40)
                f, h = seeded("small sumcheck f %d" % m, n, W), seeded("small sumcheck h %d" % m, n, W)
                got = on_device(lib, W, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, claimed, o, words=W))
                assert np.array_equal(got, oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, claimed)), (m, sdim, shifted, claimed.any())


SHORT = (1, 2, 3, 255, 257, 511, 513)


def check_short_vectors(lib, W):
    """n in SHORT for the vector entries, the CSR product's rows included; division by X + s and by one coefficient more than |H|"""
    for n in SHORT:
        a, b = seeded("short add a %d" % n, n, W), seeded("short add b %d" % n, n, W)
        assert np.array_equal(on_device(lib, W, [a, b], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=W)), a ^ b), n
        vecs = [seeded("short lincomb %d %d" % (n, k), n, W) for k in range(3)]
        coef, constant = seeded("short lincomb coef", 3, W), one_seeded("lincomb constant", W)
        want = xor_all([scaled(v, c) for v, c in zip(vecs, coef)])
        assert np.array_equal(on_device(lib, W, vecs, n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=W)), want), n
        assert np.array_equal(on_device(lib, W, vecs, n, lambda p, o: lib.lincomb_affine_dev(p, coef, constant, n, o, words=W)), want ^ constant.reshape(1, W)), n
        fz, p1, p2 = (seeded("short lincheck %s %d" % (t, n), n, W) for t in ("fz", "p1", "p2"))
        mz, r = [seeded("short lincheck mz %d %d" % (n, k), n, W) for k in range(2)], seeded("short lincheck r", 2, W)
        got = on_device(lib, W, [fz, p1, p2] + mz, n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r, p[1], p[2], n, o, words=W))
        assert np.array_equal(got, oracle.lincheck_combine(fz, mz, r, p1, p2)), n
        base, init = one_seeded("pow base", W, True), one_seeded("pow init", W)
        got = on_device(lib, W, [], n, lambda p, o: lib.pow_table_dev(o, n, base, init, words=W))
        assert np.array_equal(got, pow_reference(base, init, n)), n
        row_ptr, col, coef, vec = short_spmv_system(W, n)
        old, scale = seeded("short spmv old %d" % n, n, W), one_seeded("spmv scale", W, True)
        want = spmv_reference(row_ptr, col, coef, vec, n)
        assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, n), want), n
        assert np.array_equal(_spmv(lib, W, row_ptr, col, coef, vec, n, scale=scale, accumulate=True, init=old), scaled(want, scale) ^ old), n
    for basis, shift, counts in ((oracle.standard_basis(0, W), elem(W, top(W) | 0x80), (1, 2, 3, 300)), (oracle.standard_basis(0, W), elem(W, 0), (2, 257)),
                                 (oracle.standard_basis(6, W), elem(W, top(W) | 0x80), (65,))):
        N = 1 << basis.shape[0]
        for n_coeffs in counts:
            poly = seeded("short polydiv %d %d" % (N, n_coeffs), n_coeffs, W)
            Mq = n_coeffs - N
            got = on_device(lib, W, [poly], Mq, lambda p, o: lib.poly_div_vanishing_dev(p[0], n_coeffs, basis, shift, o, words=W))
            assert np.array_equal(got, M.div_vanishing(poly, n_coeffs, basis, shift)), (N, n_coeffs)


# ---- every entry, placed: one argument off the boundary, the output over an input, a small grid ----
def run_placed(lib, W, inputs, out_count, call, offsets, alias=None):
    """call(pointers of the inputs, pointer of the output) with input i placed offsets[i] bytes past a 16-byte boundary and the output offsets[-1]
    past one, or over input `alias`; (the output, the library's profile of the call)"""
    with Device(lib, W) as dev:
        ptrs = []
        for a, off in zip(inputs, offsets):
            dev.off = off
            ptrs.append(dev.put(a))
        dev.off = offsets[-1]
        out = ptrs[alias] if alias is not None else dev.empty(8 * W * max(out_count, 1))
        lib.profile_begin()
        call(ptrs, out)
        prof = lib.profile_report()
        return dev.get(out, out_count), prof


def entries(lib, W, n=513, m=9):
    """(profile label, element-vector inputs, other inputs, output length, call(p, o), aliasable) of every entry: vectors of n elements, domains of 2^m"""
    basis, shift = codeword_domain(m, W)
    mu = one_seeded("sumcheck mu", W, True)
    coef, constant, r = seeded("placed lincomb coef", 3, W), one_seeded("lincomb constant", W), seeded("placed lincheck r", 2, W)
    vec = lambda tag, count: [seeded("placed %s %d %d" % (tag, count, k), count, W) for k in range(5)]      # noqa: E731
    sb, sshift = basis[:6], elem(W, 0)
    base, init = one_seeded("pow base", W, True), one_seeded("pow init", W)
    row_ptr, col, sc, sv = spmv_system(W, n, 64, 5)
    # one division pass exactly (the passes of a longer division alternate between the caller's buffers and a temporary of the library's):
    # |H| / 2 < n <= |H|
    dbasis, dshift = oracle.standard_basis(max(n - 1, 0).bit_length(), W), elem(W, top(W) | 0x80)
    dN = 1 << dbasis.shape[0]
    s = STEM[W]
    N = 1 << m
    return [
        (s + "add", vec("add", n)[:2], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=W), True),
        (s + "pow_table", [], n, lambda p, o: lib.pow_table_dev(o, n, base, init, words=W), True),
        (s + "lincomb", vec("lincomb", n)[:3], n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=W), True),
        (s + "lincomb", vec("affine", n)[:3], n, lambda p, o: lib.lincomb_affine_dev(p, coef, constant, n, o, words=W), True),
        (s + "lincheck", vec("lincheck", n), n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r, p[1], p[2], n, o, words=W), True),
        (s + "spmv", [sc, sv], n, lambda p, o, row_ptr=row_ptr, col=col: _spmv_placed(lib, W, row_ptr, col, p, o, n), False),
        (s + "polydiv_pass", [seeded("placed polydiv %d" % n, n + dN, W)], n, lambda p, o: lib.poly_div_vanishing_dev(p[0], n + dN, dbasis, dshift, o, words=W), False),
        (s + "rowcheck", vec("rowcheck", N)[:3], N, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, 4, elem(W, 0x55), o, words=W), True),
        (s + "fz", vec("fz", N)[:2], N, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, basis[:4], elem(W, top(W) | 9), o, words=W), True),
        (s + "sumcheck_g_zero_sum", vec("sumcheck 0", N)[:2], N, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, elem(W, 0), o, words=W), True),
        (s + "sumcheck_g", vec("sumcheck mu", N)[:2], N, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, mu, o, words=W), True),
    ]


def _spmv_placed(lib, W, row_ptr, col, p, o, rows):
    """the CSR offsets and columns are not element vectors: they sit in buffers of their own, aligned"""
    with Device(lib, W) as dev:
        lib.spmv_dev(dev.put(row_ptr), dev.put(col), p[0], rows, p[1], o, words=W)
        lib.synchronize()


def _launches(prof, label):
    return prof.get(label, (0,))[0], prof.get(label + "_w64", (0,))[0]


def _for_each_entry(lib, W, body, **shape):
    for label, inputs, out_count, call, aliasable in entries(lib, W, **shape):
        aligned, prof = run_placed(lib, W, inputs, out_count, call, [0] * (len(inputs) + 1))
        wide, narrow = _launches(prof, label)
        assert wide >= 1 and narrow == 0, (label, "all aligned: the 128-bit form runs", wide, narrow)
        body(label, inputs, out_count, call, aligned, aliasable)


def check_mixed_placements(lib, W):
    """exactly one vector, each argument in turn and the output last, 8 bytes past a 16-byte boundary: the profile shows the 64-bit-word form
    (and not the other one), and the result is the all-aligned one"""
    def body(label, inputs, out_count, call, aligned, aliasable):
        for which in range(len(inputs) + 1):
            offsets = [8 if i == which else 0 for i in range(len(inputs) + 1)]
            got, prof = run_placed(lib, W, inputs, out_count, call, offsets)
            wide, narrow = _launches(prof, label)
            assert narrow >= 1 and wide == 0, (label, which, wide, narrow)
            assert np.array_equal(got, aligned), (label, which)
    _for_each_entry(lib, W, body)


def check_aliased_outputs(lib, W):
    """the output over each input in turn, at both placements, for the elementwise entries (position j of the output depends on position j
    of the inputs: the provers call them that way).  The CSR product gathers and a division pass reaches ahead: their outputs stay apart."""
    def body(label, inputs, out_count, call, aligned, aliasable):
        if not aliasable:
            return
        for off in OFFSETS:
            for which in range(len(inputs)):
                got, prof = run_placed(lib, W, inputs, out_count, call, [off] * (len(inputs) + 1), alias=which)
                assert sum(_launches(prof, label)) >= 1, (label, off, which)
                assert np.array_equal(got, aligned), (label, off, which)
    _for_each_entry(lib, W, body)


class options:
    def __init__(self, lib, **values):
        self.lib, self.values = lib, values

    def __enter__(self):
        for k, v in self.values.items():
            self.lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.lib.clear_option(k)


def check_small_grid(lib, W):
    """IOPX_GFX_OPS_MAX_BLOCKS = 2 and vectors of 2 * 256 * 2 + 3 elements: every grid-stride loop takes a third trip with a ragged tail.  A
    domain has 2^m points, so the domain-shaped entries run 2^11 points under a cap of 3 blocks (768 per trip: the third trip has 512).
    The results equal those of the default grid."""
    n = 2 * 256 * 2 + 3
    for cap, pick, shape in ((2, lambda out_count: out_count == n, {"n": n, "m": 11}), (3, lambda out_count: out_count == 2048, {"n": 8, "m": 11})):
        for label, inputs, out_count, call, _ in entries(lib, W, **shape):
            if not pick(out_count):
                continue
            want, _ = run_placed(lib, W, inputs, out_count, call, [0] * (len(inputs) + 1))
            with options(lib, IOPX_GFX_OPS_MAX_BLOCKS=cap):
                for off in OFFSETS:
                    got, prof = run_placed(lib, W, inputs, out_count, call, [off] * (len(inputs) + 1))
                    assert sum(_launches(prof, label)) >= 1, (label, off)
                    assert np.array_equal(got, want), (label, cap, off)
    # against the references too, under the cap: one vector entry and one domain entry
    with options(lib, IOPX_GFX_OPS_MAX_BLOCKS=2):
        vecs, coef = [seeded("grid lincomb %d" % k, n, W) for k in range(2)], seeded("grid coef", 2, W)
        got = on_device(lib, W, vecs, n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=W))
        assert np.array_equal(got, xor_all([scaled(v, c) for v, c in zip(vecs, coef)]))
        basis, shift = codeword_domain(11, W)
        fw, f1v = seeded("grid fz w", 2048, W), seeded("grid fz v", 2048, W)
        got = on_device(lib, W, [fw, f1v], 2048, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, basis[:3], elem(W, 5), o, words=W))
        assert np.array_equal(got, oracle.fz_additive(fw, f1v, basis, shift, basis[:3], elem(W, 5)))


def check_domain_table_turnover(lib, W):
    """70 distinct codeword domains in a row through fz_dev, rowcheck_dev and sumcheck_g_dev (the library keeps the tables of 64 pairs of domains),
    then the first again"""
    m = 6
    basis, n = oracle.standard_basis(m, W), 1 << m
    ib, ishift = basis[:2], elem(W, top(W) | 9)
    fw, f1v, cz = seeded("turnover w", n, W), seeded("turnover 1v", n, W), seeded("turnover c", n, W)
    shifts = [elem(W, top(W) | ((t + 1) << 8)) for t in range(70)]
    with Device(lib, W) as dev:
        pw, pf, pc, out = dev.put(fw), dev.put(f1v), dev.put(cz), dev.empty(8 * W * n)
        for shift in shifts + shifts[:1]:
            lib.fz_dev(pw, pf, basis, shift, ib, ishift, out, words=W)
            assert np.array_equal(dev.get(out, n), oracle.fz_additive(fw, f1v, basis, shift, ib, ishift))
            lib.rowcheck_dev(pw, pf, pc, basis, shift, 2, elem(W, 0), out, words=W)
            assert np.array_equal(dev.get(out, n), oracle.rowcheck_additive(fw, f1v, cz, basis, shift, 2, elem(W, 0)))
            lib.sumcheck_g_dev(pw, pf, basis, shift, ib, elem(W, 0), elem(W, 0), out, words=W)
            assert np.array_equal(dev.get(out, n), oracle.sumcheck_g_additive(fw, f1v, basis, shift, ib, elem(W, 0), elem(W, 0)))


def check_null_pointers(lib, W):
    """every entry refuses null pointers with its gf64 twin's message"""
    c = lib.c
    dom = {}
    keep = []
    for g, w in (("gf64", 1), (NAME[W], W)):
        b, s = oracle.standard_basis(4, w), elem(w, 1 << (64 * w - 1))
        keep += [b, s]
        dom[g] = (b.ctypes.data_as(U64P), s.ctypes.data_as(U64P))
    one = VP(16)
    calls = [
        lambda g: getattr(c, "iopx_%s_add_dev" % g)(None, one, one, 4),
        lambda g: getattr(c, "iopx_%s_add_dev" % g)(one, one, None, 4),
        lambda g: getattr(c, "iopx_%s_pow_table_dev" % g)(None, 4, dom[g][1], dom[g][1]),
        lambda g: getattr(c, "iopx_%s_pow_table_dev" % g)(one, 4, None, dom[g][1]),
        lambda g: getattr(c, "iopx_lincomb_%s_dev" % g)(None, 1, dom[g][1], 4, one),
        lambda g: getattr(c, "iopx_lincomb_%s_dev" % g)((VP * 1)(None), 1, dom[g][1], 4, one),
        lambda g: getattr(c, "iopx_lincomb_affine_%s_dev" % g)((VP * 1)(16), 1, dom[g][1], None, 4, one),
        lambda g: getattr(c, "iopx_spmv_%s_dev" % g)(one, one, None, 4, one, None, 0, one),
        lambda g: getattr(c, "iopx_lincheck_%s_dev" % g)(one, None, 1, dom[g][1], one, one, 4, one),
        lambda g: getattr(c, "iopx_lincheck_%s_dev" % g)(one, (VP * 1)(16), 1, None, one, one, 4, one),
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
        for g in ("gf64", NAME[W]):
            with pytest.raises(ValueError, match="null") as e:
                lib._check(call(g))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], (k, msgs)


# ---- the provers ----
SEED = 0x2204
PYTHON_TUPLES = {2: [(6, 3, 0x2204, 5, 2), (8, 15, 0x2204, 5, 2), (7, 3, 7, 3, 3), (7, 7, 8, 2, 1)],       # (log_n, inputs, seed, rs_extra, localization)
                 4: [(6, 3, 0x2204, 5, 2), (7, 3, 7, 3, 3)]}
NATIVE_TUPLES = [(7, 15), (9, 15), (7, 0)]          # (log_n, inputs) at SEED, default rate and localization
TRUST_TUPLES = sorted(set(PYTHON_TUPLES[2] + [(log_n, k, SEED, 5, 2) for log_n, k in NATIVE_TUPLES] + [(6, 3, 5, 5, 2)]))

_MODEL = {}


def model(W, log_n, k, seed=SEED, rs_extra=5, loc=2):
    """(transcript, parameters, instance) of the seeded instance, computed once per tuple"""
    key = (W, log_n, k, seed, rs_extra, loc)
    if key not in _MODEL:
        _MODEL[key] = M.prove_example(W, log_n, k, seed, rs_extra, loc)
    return _MODEL[key]


def first_difference(mine, ref):
    return next((i for i, (a, b) in enumerate(zip(mine, ref)) if a != b), min(len(mine), len(ref))), len(mine), len(ref)


def check_model_reproduces_the_oracle(words, tup):
    """the trust condition: at one and three words the model is the oracle's prover, parameters and instance"""
    ofield = {1: oracle.FIELD_GF64, 3: oracle.FIELD_GF192}[words]
    log_n, k, seed, rs_extra, loc = tup
    mine, P, inst = M.prove_example(words, log_n, k, seed, rs_extra, loc)
    ref = oracle.aurora_prove(ofield, log_n, k, seed, rs_extra=rs_extra, localization=loc)
    assert mine == ref, first_difference(mine, ref)
    want = oracle.aurora_params(ofield, log_n, k, rs_extra=rs_extra, localization=loc)
    for name in M.PARAM_NAMES + ("localization_parameters",):
        assert P[name] == want[name], name
    z, c_idx, c_coef = oracle.r1cs_example(ofield, log_n, k, seed)
    n = 1 << log_n
    i = np.arange(n)
    assert np.array_equal(z, inst["z"])
    (_, ca, va), (_, cb, vb), (_, cc, vc) = inst["matrices"]
    assert np.array_equal(ca, i % (n - 1) + 1) and np.array_equal(cb, (i + 7) % (n - 1) + 1) and np.array_equal(cc, c_idx)
    assert np.array_equal(vc, c_coef) and not (va ^ M.elem(words, 1)).any() and not (vb ^ M.elem(words, 1)).any()
    assert mine == oracle.aurora_prove_csr(ofield, inst["matrices"], n - 1, k, z, rs_extra=rs_extra, localization=loc)


def domain_field(W):
    from libiop_amd import domains
    return {2: domains.GF128, 4: domains.GF256}[W]()


def check_parameters(W):
    """aurora.AuroraParameters over the field equal the model's; the repetition counts no other field reaches"""
    from libiop_amd import aurora
    for log_n, k, rs_extra, loc in [(t[0], t[1], t[3], t[4]) for t in PYTHON_TUPLES[2]] + [(9, 15, 5, 2), (12, 15, 5, 2), (16, 15, 5, 2), (20, 15, 5, 2)]:
        n = 1 << log_n
        mine = aurora.AuroraParameters(domain_field(W), n, n - 1, k, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
        want = M.parameters(W, log_n, n - 1, rs_extra, loc)
        for name in M.PARAM_NAMES:
            assert getattr(mine, name) == want[name], (log_n, name)
        assert list(mine.localization_parameters) == want["localization_parameters"]
        reps = (mine.multi_lincheck_repetitions, mine.num_output_LDT_instances, mine.fri_interactive_repetitions)
        assert reps == ((2, 2, 2) if W == 2 else (1, 1, 1)), (log_n, reps)


def aurora_ops(lib, torch, device, W):
    from libiop_amd import domains
    cls, plain = {2: (domains.GF128AuroraOps, domains.GF128DeviceOps), 4: (domains.GF256AuroraOps, domains.GF256DeviceOps)}[W]
    ops = cls(lib, torch, device, domain_field(W))
    assert isinstance(ops, plain)
    assert type(domains.DeviceOps(lib, torch, device, domain_field(W))) is plain      # the plain construction keeps its class
    return ops


def python_prove(lib, torch, device, W, inst, rs_extra=5, loc=2):
    """the Python prover on the model's instance (CSR matrices plus assignment)"""
    from libiop_amd import aurora, r1cs
    ops = aurora_ops(lib, torch, device, W)
    n, k, z = len(inst["matrices"][0][0]) - 1, inst["num_inputs"], inst["z"]
    mats = [r1cs.CSRMatrix(ops, np.asarray(rp, dtype=np.int64), np.asarray(cl, dtype=np.int64), cf, n) for rp, cl, cf in inst["matrices"]]
    cs = r1cs.R1CS(mats[0], mats[1], mats[2], k, inst["num_variables"])
    params = aurora.AuroraParameters(ops.field, n, inst["num_variables"], k, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
    return aurora.aurora_snark_prover(ops, cs, z[:k].copy(), z[k:].copy(), params).serialize()


def check_python_prover(lib, torch, device, W, case):
    log_n, k, seed, rs_extra, loc = case
    want, _, inst = model(W, log_n, k, seed, rs_extra, loc)
    mine = python_prove(lib, torch, device, W, inst, rs_extra, loc)
    assert mine == want, first_difference(mine, want)
    # the library's own generator gives the model's instance
    from libiop_amd import r1cs
    ops = aurora_ops(lib, torch, device, W)
    n = 1 << log_n
    _, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, k, n - 1, seed)
    assert np.array_equal(np.concatenate([primary, auxiliary]), inst["z"])


def native_prove(lib, W, inst, rs_extra=5, loc=2, **kw):
    h = lib.aurora_instance(field_code(W), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
    try:
        return lib.aurora_prove(h, 128, rs_extra, loc, **kw)
    finally:
        lib.aurora_instance_free(h)


def check_native_prover(lib, torch, device, W, case):
    import libiop_amd as la
    log_n, k = case
    want, _, inst = model(W, log_n, k)
    h = lib.aurora_instance(field_code(W), inst["matrices"], inst["num_variables"], k, inst["z"])
    try:
        for head_eval in (1, 0):                    # a subspace-only field runs the reference's schedule either way
            with options(lib, IOPX_HEAD_EVAL=head_eval):
                mine = lib.aurora_prove(h)
                assert mine == want, (head_eval,) + first_difference(mine, want)
        assert lib.aurora_prove(h, hash=la.HASH_BLAKE2B) == want
        lib.aurora_instance_warm(h)
        assert lib.aurora_prove(h) == want
    finally:
        lib.aurora_instance_free(h)
    assert python_prove(lib, torch, device, W, inst) == want


def flipped(inst):
    bad = dict(inst)
    z = inst["z"].copy()
    z[inst["num_inputs"] + 11, z.shape[1] - 1] ^= np.uint64(1)
    bad["z"] = z
    return bad


def check_unsatisfied_assignment(lib, torch, device, W):
    """one word of one auxiliary element flipped: both provers emit the model's transcript for that assignment"""
    good, _, inst = model(W, 6, 3, 5)
    bad = flipped(inst)
    want = M.prove(W, bad)
    assert want != good
    for head_eval in (1, 0):
        with options(lib, IOPX_HEAD_EVAL=head_eval):
            mine = native_prove(lib, W, bad)
            assert mine == want, (head_eval,) + first_difference(mine, want)
    mine = python_prove(lib, torch, device, W, bad)
    assert mine == want, first_difference(mine, want)


def check_fractal_operators_refused(lib, torch, device, W):
    ops = aurora_ops(lib, torch, device, W)
    for name in ("div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine", "rational_sumcheck_constraint"):
        with pytest.raises(NotImplementedError, match=NAME[W]):
            getattr(ops, name)(None, None, None, None, None, None)
    from libiop_amd import domains
    plain = domains.DeviceOps(lib, torch, device, domain_field(W))
    for name in ("rowcheck", "mul"):
        with pytest.raises(NotImplementedError, match=NAME[W]):
            getattr(plain, name)(None, None, None, None, None)
    vecs, coef, constant = [seeded("ops affine %d" % k, 100, W) for k in range(3)], seeded("ops affine coef", 3, W), seeded("ops affine constant", 1, W)
    got = ops.download(ops.lincomb_affine([ops.upload(v) for v in vecs], coef, constant[0], 100))
    assert np.array_equal(got, xor_all([scaled(v, c) for v, c in zip(vecs, coef)]) ^ constant)


def check_native_refusals(lib, W):
    import libiop_amd as la
    f = NAME[W]
    want, _, inst = model(W, 7, 0)
    h = lib.aurora_instance(field_code(W), inst["matrices"], inst["num_variables"], 0, inst["z"])
    comm = lib.comm_create_replay(0, 1)
    try:
        with pytest.raises(ValueError, match="%s has no distributed prover: pass no communicator" % f):
            lib.aurora_prove_dist(h, comm)
        with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over %s" % f):
            lib.fractal_index(h)
        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over %s" % f):
            lib.fractal_prove(h)
        for hh in (la.HASH_POSEIDON_STARKWARE, la.HASH_POSEIDON_HIGH_ALPHA):
            with pytest.raises(ValueError, match="%s proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only" % f):
                lib.aurora_prove(h, hash=hh)
        with pytest.raises(ValueError, match="security_parameter 100 is not supported"):
            lib.aurora_prove(h, 100)
        with pytest.raises(ValueError, match="codeword domain dimension 41: the %s transforms take domains of dimension up to 40" % f):
            lib.aurora_prove(h, 128, 34, 2)
        with pytest.raises(ValueError, match="iopx_aurora_example_instance_create: only the FRI-only SNARK is built over %s" % f):      # kept as it was
            lib.aurora_example_instance(field_code(W), 128, 3, 127, SEED)
        assert lib.aurora_prove(h) == want          # the instance still proves after the refusals
    finally:
        lib.comm_destroy(comm)
        lib.aurora_instance_free(h)


def check_other_fields_unchanged(lib, torch, device):
    """after proofs over gf128 and gf256 in this process: gf192, gf64 and edwards Fr against the oracle's prover, alt_bn128 Fr against its model"""
    import aurora_cases
    import bn128_aurora_model as BM
    import libiop_amd as la
    for W in WORDS:
        want, _, inst = model(W, 6, 3, 5)
        assert native_prove(lib, W, inst) == want
    aurora_cases.check_transcript_equals_oracle(lib, torch, device, "gf192", 6, 3, SEED, rs_extra=3, localization=2)
    for code, ocode, log_n, k, rs_extra, loc in ((la.FIELD_GF192, oracle.FIELD_GF192, 6, 3, 3, 2), (la.FIELD_GF64, oracle.FIELD_GF64, 6, 3, 5, 2),
                                                 (la.FIELD_EDWARDS_FR, oracle.FIELD_EDWARDS, 7, 7, 2, 3)):
        n = 1 << log_n
        h = lib.aurora_example_instance(code, n, k, n - 1, SEED)
        try:
            assert lib.aurora_prove(h, 128, rs_extra, loc) == oracle.aurora_prove(ocode, log_n, k, SEED, rs_extra=rs_extra, localization=loc), code
        finally:
            lib.aurora_instance_free(h)
    h = lib.aurora_example_instance(la.FIELD_ALT_BN128_FR, 64, 3, 63, SEED)
    try:
        assert lib.aurora_prove(h, 128, 3, 2) == BM.prove_example(BM.ALT_BN128_FR, BM.BLAKE2B, 6, 3, 3, 2, SEED)
    finally:
        lib.aurora_instance_free(h)


# ---- the recorded digests (tools/make_gfx_aurora_digests.py) ----
def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfx_aurora.json")) as f:
        return {e["field"]: e for e in json.load(f)["aurora"]}


def digest_instance(W):
    pin = golden_digests()[NAME[W]]
    return pin, M.example(W, pin["log_n"], pin["num_inputs"], pin["seed"])


def check_native_digest(lib, W):
    pin, inst = digest_instance(W)
    mine = native_prove(lib, W, inst)
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])


def check_python_digest(lib, torch, device, W):
    pin, inst = digest_instance(W)
    mine = python_prove(lib, torch, device, W, inst)
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])
