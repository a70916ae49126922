"""Cases past the launch caps of the GF(2^64) arm: the protocol-layer entries (libiop_amd/csrc/gfx_ops.h over gf64) at the smallest sizes where their grid-stride loops
take a second trip (16384 workgroups of 256 lanes: 2^22 elements with one element per lane, 2^23 with two), and the LDE of
libiop_amd/csrc/gf64.hip with more cosets than one staging group holds.  Run by tests/test_gpu_gf64_large.py on the MI355X; every function
takes the Library under test, so the emulation can run them by hand (1 - 90 s each).  tests/test_gf64_large_emu.py checks the host-side
reference below against the oracle's functions at m = 12 and runs the cases the emulation affords in a second.

The oracle's own virtual-oracle functions and its inversion take minutes at 2^24 elements.  The reference here is built whole-vector from
oracle.gf_mul, oracle.gf_inv on short vectors and XOR:
  - a vanishing polynomial Z_S is affine over GF(2): its values over a domain are the subset sums of Z_S(shift) and Z_S(shift + basis[k]) -
    Z_S(shift), each a product of (x + s) over the elements of S, spread by doubling (v -> v, v + t_k);
  - the same doubling gives the domain's elements x_j, and x_j^|H| is log2 |H| squarings;
  - 1 / Z_H takes one value per coset of H: those are inverted and repeated;
  - the non-zero arm of sumcheck_g is multiplied back instead of dividing by x_j.
Every comparison is byte equality of whole vectors."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import gf64_aurora_cases as C
import gf64_cases as G
import oracle

BIT63 = C.BIT63
CAP_ODD = (1 << 23) + 3         # one trip and a 3-element tail with two elements per lane, two trips with one; an odd length
CAP_M = 24                      # two trips with two elements per lane, four with one
CAP_ROWS = (1 << 22) + 3        # the entries that take one element per lane


# ---- host-side reference ----
def mul(a, b):
    """oracle.gf_mul of two long vectors, in slices on a few threads (the call releases the interpreter lock)"""
    n = a.shape[0]
    if n < (1 << 18):
        return oracle.gf_mul(a, b)
    out = np.empty_like(a)
    step = 1 << 20
    def part(lo):
        out[lo:lo + step] = oracle.gf_mul(a[lo:lo + step], b[lo:lo + step])
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(part, range(0, n, step)))
    return out


def scaled(v, c):
    return mul(v, np.full((v.shape[0], 1), int(np.asarray(c).reshape(-1)[0]), dtype=np.uint64))


def spread(v0, terms):
    """v0 + sum_{bit k of j} terms[k] for every j < 2^len(terms)"""
    v = np.array([[int(v0)]], dtype=np.uint64)
    for t in terms:
        v = np.concatenate([v, v ^ np.uint64(int(t))])
    return v


def subset_points(basis, shift):
    """the elements of span(basis) + shift; at most 2^12 of them are ever asked for"""
    return spread(int(np.asarray(shift).reshape(-1)[0]), [int(b[0]) for b in basis])


def vanishing_at(points, sub_basis, sub_shift):
    """Z_S(x) = prod_{s in S} (x + s), S = span(sub_basis) + sub_shift, at each x of the (short) vector `points`"""
    acc = np.ones_like(points)
    for s in subset_points(sub_basis, sub_shift):
        acc = oracle.gf_mul(acc, points ^ s)
    return acc


def vanishing_terms(basis, shift, sub_basis, sub_shift):
    """(Z_S(shift), [Z_S(shift + basis[k]) - Z_S(shift)]): the affine map's value at the origin of the domain and its linear part on the basis"""
    s0 = int(np.asarray(shift).reshape(-1)[0])
    points = np.array([[s0]] + [[s0 ^ int(b[0])] for b in basis], dtype=np.uint64)
    z = vanishing_at(points, sub_basis, sub_shift)
    return int(z[0, 0]), [int(v) ^ int(z[0, 0]) for v in z[1:, 0]]


def vanishing_over_domain(basis, shift, sub_basis, sub_shift):
    return spread(*vanishing_terms(basis, shift, sub_basis, sub_shift))


def domain_elements(basis, shift):
    return subset_points(basis, shift)


def ref_rowcheck(az, bz, cz, basis, shift, h, cshift):
    z0, terms = vanishing_terms(basis, shift, basis[:h], cshift)
    assert not any(terms[:h])                                           # Z_H is constant on the cosets of H
    zinv = np.repeat(oracle.gf_inv(spread(z0, terms[h:])), 1 << h, axis=0)
    return mul(mul(az, bz) ^ cz, zinv)


def ref_fz(fw, f1v, basis, shift, ib, ishift):
    return mul(fw, vanishing_over_domain(basis, shift, ib, ishift)) ^ f1v


def ref_sumcheck_zero(f, h, basis, shift, sb, sshift):
    return f ^ mul(vanishing_over_domain(basis, shift, sb, sshift), h)


def sumcheck_constant(sb, mu):
    """eps^-1 mu, eps the product of the non-zero elements of span(sb) (sumcheck.tcc:52-54)"""
    eps = np.ones((1, 1), dtype=np.uint64)
    for s in subset_points(sb, 0)[1:]:
        eps = oracle.gf_mul(eps, s.reshape(1, 1))
    return oracle.gf_mul(oracle.gf_inv(eps), np.asarray(mu, dtype=np.uint64).reshape(1, 1))


def assert_sumcheck_nonzero(got, f, h, basis, shift, sb, sshift, mu):
    """got = f + Z_H h + c x^(|H| - 1) with 1 / 0 = 0, checked without inverting x: (got + f + Z_H h) x = x^|H| c, and the term is 0 where x is"""
    term = got ^ ref_sumcheck_zero(f, h, basis, shift, sb, sshift)
    x = domain_elements(basis, shift)
    xh = x
    for _ in range(sb.shape[0]):
        xh = mul(xh, xh)
    assert np.array_equal(mul(term, x), scaled(xh, sumcheck_constant(sb, mu)))
    zero = x[:, 0] == 0
    assert int(zero.sum()) == (1 if int(np.asarray(shift).reshape(-1)[0]) == 0 else 0)
    assert not term[zero].any(), "the term at x = 0 is not 0"
    assert term[~zero].all()                                            # c x^(|H| - 1) is non-zero away from 0: the arm did run


# ---- device placements ----
def both_placements(lib, inputs, out_count, call, label=None):
    """C.on_device with the library's profile around each call: the entry launched its kernel once at either placement, under the name of the
    placement's form (`label` on the 16-byte boundary, `label` + "_w64" 8 bytes past it)"""
    if label is None:
        return C.on_device(lib, inputs, out_count, call)
    launches = []
    def counted(p, o):
        lib.profile_begin()
        call(p, o)
        launches.append(C.launches(lib.profile_report(), label))
    got = C.on_device(lib, inputs, out_count, counted)
    assert launches == [(1, 0), (0, 1)], (label, launches)
    return got


def one_placement(lib, inputs, out_count, call, init=None):
    with C.Device(lib) as dev:
        ptrs = [dev.put(a) for a in inputs]
        out = dev.put(init) if init is not None else dev.empty(8 * max(out_count, 1))
        call(ptrs, out)
        return dev.get(out, out_count)


# ---- 1. the entries of gfx_ops.h over gf64 past their caps ----
def check_add(lib, n=CAP_ODD):
    a, b = G.seeded("large add a", n), G.seeded("large add b", n)
    got = both_placements(lib, [a, b], n, lambda p, o: lib.field_add_dev(p[0], p[1], o, n, words=1), "k64_add")
    assert np.array_equal(got, a ^ b)


def check_lincomb(lib, n=CAP_ODD):
    num = 3
    vecs = [G.seeded("large lincomb %d" % k, n) for k in range(num)]
    coef = G.seeded("large lincomb coef", num)
    coef[2, 0] |= np.uint64(BIT63)
    constant = G.elem(int(G.seeded("large lincomb constant", 1)[0, 0]))
    want = C.xor_all([scaled(v, c) for v, c in zip(vecs, coef)])
    got = both_placements(lib, vecs, n, lambda p, o: lib.lincomb_dev(p, coef, n, o, words=1), "k64_lincomb")
    assert np.array_equal(got, want)
    got = both_placements(lib, vecs, n, lambda p, o: lib.lincomb_affine_dev(p, coef, constant, n, o, words=1), "k64_lincomb")
    assert np.array_equal(got, want ^ constant.reshape(1, 1))


def check_lincheck(lib, n=CAP_ODD):
    fz, p1, p2 = (G.seeded("large lincheck " + t, n) for t in ("fz", "p1", "p2"))
    mz = [G.seeded("large lincheck mz %d" % k, n) for k in range(2)]
    r = G.seeded("large lincheck r", 2)
    want = mul(scaled(mz[0], r[0]) ^ scaled(mz[1], r[1]), p1) ^ mul(fz, p2)
    got = both_placements(lib, [fz, p1, p2] + mz, n, lambda p, o: lib.lincheck_dev(p[0], p[3:], r, p[1], p[2], n, o, words=1), "k64_lincheck")
    assert np.array_equal(got, want)


def ref_pow_table(count, base, init):
    """tab[2^k .. 2^(k+1)) = tab[0 .. 2^k) base^(2^k)"""
    tab = np.asarray(init, dtype=np.uint64).reshape(1, 1)
    sq = np.asarray(base, dtype=np.uint64).reshape(1, 1)
    while tab.shape[0] < count:
        tab = np.concatenate([tab, scaled(tab, sq)])
        sq = oracle.gf_mul(sq, sq)
    return tab[:count]


def check_pow_table(lib, count=CAP_ODD):
    base = G.elem(int(G.seeded("large pow base", 1)[0, 0]) | BIT63)
    init = G.elem(int(G.seeded("large pow init", 1)[0, 0]))
    got = one_placement(lib, [], count, lambda p, o: lib.pow_table_dev(o, count, base, init, words=1))
    assert np.array_equal(got, ref_pow_table(count, base, init))


def check_spmv(lib, rows=CAP_ROWS, cols=1 << 16):
    rng = np.random.default_rng(0x5364)
    lengths = rng.integers(1, 3, size=rows)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, cols, size=int(row_ptr[-1])).astype(np.uint32)
    coef, vec = G.seeded("large spmv coef", col.shape[0]), G.seeded("large spmv vec", cols)
    want = np.bitwise_xor.reduceat(mul(coef, vec[col]), row_ptr[:-1].astype(np.int64), axis=0)          # no row is empty
    got = one_placement(lib, [row_ptr, col, coef, vec], rows, lambda p, o: lib.spmv_dev(p[0], p[1], p[2], rows, p[3], o, words=1))
    assert np.array_equal(got, want)


def poly_mul_sparse(a, b):
    """a (long) times b (few non-zero coefficients), schoolbook"""
    out = np.zeros((a.shape[0] + b.shape[0] - 1, 1), dtype=np.uint64)
    for i in range(b.shape[0]):
        if b[i, 0]:
            out[i:i + a.shape[0]] ^= scaled(a, b[i])
    return out


def check_poly_div_vanishing(lib, M=CAP_ROWS):
    basis, shift = G.std_basis(6), G.elem(BIT63 | 0x80)
    N = 64
    n_coeffs = N + M
    Z = C._vanishing_coefficients(basis, shift)
    assert Z.shape[0] == N + 1 and int(Z[N, 0]) == 1
    poly = G.seeded("large polydiv", n_coeffs)
    got = one_placement(lib, [poly], M, lambda p, o: lib.poly_div_vanishing_dev(p[0], n_coeffs, basis, shift, o, words=1))
    remainder = poly ^ poly_mul_sparse(got, Z)                          # Q Z + R = P
    assert not remainder[N:].any(), "the remainder has degree >= |H|"


def check_rowcheck(lib, m=CAP_M, h=12):
    basis, shift = C.codeword_domain(m)
    n = 1 << m
    cshift = G.elem(BIT63 >> 1)
    az, bz, cz = (G.seeded("large rowcheck " + t, n) for t in "abc")
    got = both_placements(lib, [az, bz, cz], n, lambda p, o: lib.rowcheck_dev(p[0], p[1], p[2], basis, shift, h, cshift, o, words=1), "k64_rowcheck")
    assert np.array_equal(got, ref_rowcheck(az, bz, cz, basis, shift, h, cshift))


def check_fz(lib, m=CAP_M, input_dim=4):
    basis, shift = C.codeword_domain(m)
    n = 1 << m
    ib, ishift = basis[:input_dim], G.elem(BIT63 | 9)
    fw, f1v = G.seeded("large fz w", n), G.seeded("large fz 1v", n)
    got = both_placements(lib, [fw, f1v], n, lambda p, o: lib.fz_dev(p[0], p[1], basis, shift, ib, ishift, o, words=1), "k64_fz")
    assert np.array_equal(got, ref_fz(fw, f1v, basis, shift, ib, ishift))


SUMCHECK_ARMS = ["zero sum", "non-zero sum", "non-zero sum, unshifted"]


def check_sumcheck_g(lib, arm, m=CAP_M, summation_dim=2):
    """summation_dim = 2 keeps the reference at two squarings of the whole vector; the kernel's work per element does not depend on it"""
    shifted = arm != SUMCHECK_ARMS[2]
    basis, shift = C.codeword_domain(m, shifted)
    n = 1 << m
    sb, sshift = basis[:summation_dim], G.elem(BIT63 | 0x40)
    f, h = G.seeded("large sumcheck f", n), G.seeded("large sumcheck h", n)
    if arm == SUMCHECK_ARMS[0]:
        got = both_placements(lib, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, G.elem(0), o, words=1), "k64_sumcheck_g_zero_sum")
        assert np.array_equal(got, ref_sumcheck_zero(f, h, basis, shift, sb, sshift))
    else:
        mu = G.elem(int(G.seeded("large sumcheck mu", 1)[0, 0]) | BIT63)
        got = both_placements(lib, [f, h], n, lambda p, o: lib.sumcheck_g_dev(p[0], p[1], basis, shift, sb, sshift, mu, o, words=1), "k64_sumcheck_g")
        assert_sumcheck_nonzero(got, f, h, basis, shift, sb, sshift, mu)


# ---- the reference itself, against the oracle's functions (CPU suite, m = 12) ----
def check_reference_against_oracle(m=12):
    n = 1 << m
    mu = G.elem(int(G.seeded("large sumcheck mu", 1)[0, 0]) | BIT63)
    for shifted in (True, False):
        basis, shift = C.codeword_domain(m, shifted)
        assert np.array_equal(domain_elements(basis, shift), oracle.all_subset_sums(basis, shift))
        a, b, c = (G.seeded("reference " + t, n) for t in "abc")
        for input_dim in (0, 4, 6):
            ib, ishift = basis[:input_dim], G.elem(BIT63 | 9)
            assert np.array_equal(ref_fz(a, b, basis, shift, ib, ishift), oracle.fz_additive(a, b, basis, shift, ib, ishift)), input_dim
        for h in (0, 5, m):
            cshift = G.elem(BIT63 >> 1)
            assert np.array_equal(ref_rowcheck(a, b, c, basis, shift, h, cshift), oracle.rowcheck_additive(a, b, c, basis, shift, h, cshift)), h
        for sdim in (0, 2, 6):
            sb, sshift = basis[:sdim], G.elem(BIT63 | 0x40)
            assert np.array_equal(ref_sumcheck_zero(a, b, basis, shift, sb, sshift), oracle.sumcheck_g_additive(a, b, basis, shift, sb, sshift, G.elem(0))), sdim
            want = oracle.sumcheck_g_additive(a, b, basis, shift, sb, sshift, mu)
            assert_sumcheck_nonzero(want, a, b, basis, shift, sb, sshift, mu)
            bad = want.copy()
            bad[n - 1, 0] ^= np.uint64(1)
            try:
                assert_sumcheck_nonzero(bad, a, b, basis, shift, sb, sshift, mu)
            except AssertionError:
                pass
            else:
                raise AssertionError("one flipped bit passed the multiplied-back check")
    base, init = G.elem(int(G.seeded("large pow base", 1)[0, 0]) | BIT63), G.elem(int(G.seeded("large pow init", 1)[0, 0]))
    want = np.empty((37, 1), dtype=np.uint64)
    cur = init.reshape(1, 1)
    for l in range(37):
        want[l] = cur[0]
        cur = oracle.gf_mul(cur, base.reshape(1, 1))
    assert np.array_equal(ref_pow_table(37, base, init), want)
    big = G.seeded("reference mul", (1 << 20) + 5)
    assert np.array_equal(mul(big, big[::-1].copy()), oracle.gf_mul(big, big[::-1].copy()))          # the sliced product is the whole one


# ---- 3. the LDE with more cosets than one staging group ----
LDE_D, LDE_M, LDE_BEGIN, LDE_COUNT = 13, 26, 3, 4096 + 5
LDE_GROUP = 4096                # cosets of 2^13 in one staging block of 2^25 elements; the second group is partial


def count_mismatch(lib, d_a, d_b, nbytes):
    with C.Device(lib) as dev:
        d_count = dev.put(np.zeros((1, 1), dtype=np.uint64))
        lib._check(lib.c.iopx_count_mismatch_dev(ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), ctypes.c_size_t(nbytes), ctypes.c_void_p(d_count)))
        return int(dev.get(d_count, 1)[0, 0])


def check_lde_groups(lib, d=LDE_D, m=LDE_M, begin=LDE_BEGIN, count=LDE_COUNT, group=LDE_GROUP):
    basis, shift = G.std_basis(m), G.elem(BIT63 | 0x1234567 | (1 << m))
    coeffs = G.seeded("lde groups", 1 << d)
    nd = 1 << d
    assert group < count < 2 * group
    with C.Device(lib) as dev:
        dc = dev.put(coeffs)
        whole, parts = dev.empty(8 * count * nd), dev.empty(8 * count * nd)
        lib.profile_begin()
        lib.additive_LDE_gf64_dev(dc, nd, basis, shift, begin, count, whole)
        prof = lib.profile_report()
        assert prof.get("k64_bfly_upper", (0,))[0] >= 1, "no upper pass: the staged path did not run"
        assert prof["k64_bfly_edge"][0] == 2, "the call did not take two groups"
        # (a) Horner at sampled positions of the first and last coset of each group
        rng = np.random.default_rng(0x4c4445)
        for coset in (0, group - 1, group, count - 1):
            block = dev.get(whole + 8 * coset * nd, nd)
            for pos in [0, nd - 1] + [int(v) for v in rng.integers(1, nd - 1, size=2)]:
                j = ((begin + coset) << d) + pos
                x = int(shift[0])
                for k in range(m):
                    if (j >> k) & 1:
                        x ^= int(basis[k, 0])
                assert int(block[pos, 0]) == int(oracle.poly_eval(coeffs, G.elem(x))[0]), (coset, pos)
        # (b) the same block from two calls that each stay within one group
        lib.profile_begin()
        lib.additive_LDE_gf64_dev(dc, nd, basis, shift, begin, group, parts)
        lib.additive_LDE_gf64_dev(dc, nd, basis, shift, begin + group, count - group, parts + 8 * group * nd)
        assert lib.profile_report()["k64_bfly_edge"][0] == 2, "a one-group call took more than one group"
        assert count_mismatch(lib, whole, parts, 8 * count * nd) == 0
        # the count sees a difference: one word of the second group changed
        lib.h2d(parts + 8 * (group * nd + 17), np.array([[int(dev.get(parts + 8 * (group * nd + 17), 1)[0, 0]) ^ 1]], dtype=np.uint64))
        assert count_mismatch(lib, whole, parts, 8 * count * nd) == 1
