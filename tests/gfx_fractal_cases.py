"""Cases for what the Fractal prover needs over GF(2^64), GF(2^128) and GF(2^256) (include/libiop_amd_fractal.h): the batch division, point - x and
c - Z_S(x) over a domain, the rational combination and the rational sumcheck's constraint oracle, parametrised by the words per element W in {1, 2, 4},
and the native and Python Fractal provers over gf64 under IOPX_GFX_FRACTAL=1.  Shared by tests/test_gfx_fractal_emu.py (CPU emulation) and
tests/test_gpu_gfx_fractal.py (MI355X): every function takes the Library under test.

Every comparison is byte equality.  Expected values of the kernels come from oracle.gf_mul, oracle.gf_inv, oracle.all_subset_sums and XOR only; Z_S(x)
is the plain product of (x + s) over the elements s of S, and the constraint oracle is held to out * Z_K(x) = D (p + eps^-1 mu x^(|K| - 1)) + N, which
needs no division (Z_K != 0 makes the quotient unique).  Expected transcripts are the oracle's own Fractal prover's over gf64."""
import hashlib
import json
import os

import numpy as np
import pytest

import gf64_aurora_cases as G64
import gfx_aurora_cases as C
import gfx_aurora_model as M
import gfx_batch_cases as B
import gfx_head_cases as H
import oracle

WORDS = B.WORDS
NAME = B.NAME
STEM = B.STEM
OPTION = "IOPX_GFX_FRACTAL"
KERNELS = ("div", "domain_offsets", "vanishing_evals", "rational_combine", "rational_sumcheck_constraint")
DIV_SIZES = (0, 1, 255, 256, 257, 256 * 16 + 3)
OFFSETS_DIMS = (0, 1, 8, 9, 13)
VANISHING_SHAPES = tuple((m, d) for m in (0, 5, 9) for d in sorted({0, 1, 4, m}) if d <= m)
RATIONAL_SIZES = (1, 100, 1 << 10)
CONSTRAINT_SHAPES = tuple((m, k) for m in (1, 6, 7, 10) for k in sorted({0, 1, 5, 6, 7, m}) if k <= m)
SEED = 0x2205
NATIVE_TUPLES = [(6, 3, 3, 2), (7, 15, 3, 2), (7, 15, 2, 3)]        # (log_n, inputs, rs_extra, localization) at SEED
PYTHON_TUPLES = [(6, 3, 3, 2), (7, 15, 3, 2)]
DIGEST_SIZES = (10, 14)


def seeded(tag, n, W):
    return C.seeded("fractal " + tag, n, W)


def zero(W):
    return M.elem(W, 0)


def one(W):
    return M.elem(W, 1)


def ones(n, W):
    return np.ascontiguousarray(np.broadcast_to(one(W), (n, W)))


def label(W, kernel, w64):
    return STEM[W] + kernel + ("_w64" if w64 else "")


def rows_of(prof, W, kernel):
    """the profile's rows of one kernel of the field, both forms"""
    return {k: v for k, v in prof.items() if k in (label(W, kernel, False), label(W, kernel, True))}


def run(lib, W, inputs, offsets, out_counts, call):
    """call(pointers of the inputs (None stays None), pointers of the outputs) with vector i placed offsets[i] bytes past a 16-byte boundary (inputs
    first, then outputs); (the outputs, the profile)"""
    with C.Device(lib, W) as dev:
        ptrs = []
        for a, off in zip(inputs, offsets):
            dev.off = off
            ptrs.append(None if a is None else dev.put(a))
        outs = []
        for n, off in zip(out_counts, offsets[len(inputs):]):
            dev.off = off
            outs.append(dev.empty(8 * W * max(n, 1)))
        lib.profile_begin()
        call(ptrs, outs)
        prof = lib.profile_report()
        return [dev.get(o, n) for o, n in zip(outs, out_counts)], prof


def assert_one_row(prof, W, kernel, w64, nbytes, why):
    rows = rows_of(prof, W, kernel)
    assert list(rows) == [label(W, kernel, w64)], (rows, why)
    assert rows[label(W, kernel, w64)][0] == 1 and rows[label(W, kernel, w64)][2] == nbytes, (rows, nbytes, why)


def placements(vectors):
    """every vector on the boundary, every vector 8 bytes past one, and each vector alone off it"""
    alone = [tuple(8 if i == j else 0 for i in range(vectors)) for j in range(vectors)]
    return [(0,) * vectors, (8,) * vectors] + alone


# ---- the batch division ----
def inverses(den):
    """1 / den row by row, zero where den is zero"""
    nz = den.any(axis=1)
    safe = den.copy()
    safe[~nz] = one(den.shape[1])
    inv = oracle.gf_inv(safe) if den.shape[0] else safe
    inv[~nz] = 0
    return inv


def div_expected(num, den):
    inv = inverses(den)
    return inv if num is None else oracle.gf_mul(num, inv) if den.shape[0] else inv


def div_run(lib, W, num, den, offsets=(0, 0, 0)):
    n = den.shape[0]
    (got,), prof = run(lib, W, [num, den], offsets, [n], lambda p, o: lib.field_div_dev(p[0], p[1], o[0], n, words=W))
    return got, prof


def check_div(lib, W, n):
    """num given and NULL, at every placement: the quotients, the form of the launch (the 64-bit-word form exactly when a vector of the launch is off the
    16-byte boundary) and its declared bytes"""
    den, num = seeded("div den %d" % n, n, W), seeded("div num %d" % n, n, W)
    for with_num in (True, False):
        want = div_expected(num if with_num else None, den)
        for offs in placements(3):
            got, prof = div_run(lib, W, num if with_num else None, den, offs)
            assert np.array_equal(got, want), (NAME[W], n, with_num, offs)
            if n:
                w64 = bool(offs[1] or offs[2] or (with_num and offs[0]))
                assert_one_row(prof, W, "div", w64, n * 8 * W * (6 if with_num else 5), (n, with_num, offs))
            else:
                assert not rows_of(prof, W, "div")


def check_div_strides(lib, W):
    """2^13 elements under IOPX_GFX_OPS_MAX_BLOCKS = 2 and 3: a lane walks 16 (11) slots of one element, 8 (6) of gf64's pairs, and at 3 blocks the last
    stride is ragged; zero denominators at position 0, at the last position, at a lane's first and last stride in either form, and everywhere"""
    n = 1 << 13
    den, num = seeded("div stride den", n, W), seeded("div stride num", n, W)
    assert den.any(axis=1).all()
    for cap in (2, 3):
        T = cap * 256
        holes = den.copy()
        for j in (0, n - 1, 5, 5 + T * ((n - 6) // T), 10, 11, 2 * (5 + T * ((n // 2 - 6) // T)), 2 * (5 + T * ((n // 2 - 6) // T)) + 1):
            holes[j] = 0
        with C.options(lib, IOPX_GFX_OPS_MAX_BLOCKS=cap):
            inv = inverses(holes)                                # the reference's inversions once per cap
            want = {True: oracle.gf_mul(num, inv), False: inv}
            runs = [(holes, with_num, offs, want[with_num]) for with_num in (True, False) for offs in ((0, 0, 0), (8, 8, 8))]
            runs.append((np.zeros_like(den), True, (8, 8, 8), np.zeros_like(den)))
            for d, with_num, offs, expected in runs:
                got, prof = div_run(lib, W, num if with_num else None, d, offs)
                assert np.array_equal(got, expected), (NAME[W], cap, with_num, offs, bool(d.any()))
                assert list(rows_of(prof, W, "div")) == [label(W, "div", bool(offs[0]))]


def check_div_inversions(lib, W):
    """the two ways a workgroup's root is inverted (IOPX_GFX_DIV_INVERSION = 1: the Fermat power, 2: binary Euclid) give the same quotients: several
    workgroups with their own roots, and one of a single element"""
    for n in (1, 257, 256 * 16 * 3 + 5):
        den, num = seeded("div inversion den %d" % n, n, W), seeded("div inversion num %d" % n, n, W)
        den[n // 2] = 0
        want = div_expected(num, den)
        for way in (1, 2):
            with C.options(lib, IOPX_GFX_DIV_INVERSION=way):
                for offs in ((0, 0, 0), (8, 8, 8)):
                    got, _ = div_run(lib, W, num, den, offs)
                    assert np.array_equal(got, want), (NAME[W], n, way, offs)


def check_div_refusals(lib, W):
    n = 64
    with C.Device(lib, W) as dev:
        a, b, c = dev.put(seeded("div refused a", n, W)), dev.put(seeded("div refused b", n, W)), dev.empty(8 * W * n)
        for args in ((a, b, b), (a, b, a), (None, b, b)):
            with pytest.raises(ValueError, match="the quotient buffer holds the running products: it cannot alias an input"):
                lib.field_div_dev(*args, n, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.field_div_dev(a, 0, c, n, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.field_div_dev(a, b, 0, n, words=W)
        lib.field_div_dev(a, 0, 0, 0, words=W)                  # nothing to do


# ---- point - x and c - Z_S(x) over a domain ----
def domain(m, W, kind="standard"):
    """(basis, shift): the standard basis with a shift outside its span, or a seeded basis with a seeded shift"""
    if kind == "standard":
        return oracle.standard_basis(m, W), M.elem(W, C.top(W) | 0x1234567 | (1 << m))
    return seeded("basis %d" % m, m, W), seeded("shift %d" % m, 1, W)[0]


def check_domain_offsets(lib, W, m):
    n = 1 << m
    for kind in ("standard", "seeded"):
        basis, shift = domain(m, W, kind)
        xs = oracle.all_subset_sums(basis, shift)
        inside = xs[(5 * n) // 7]
        for tag, point in (("outside", seeded("point %d" % m, 1, W)[0]), ("zero", zero(W)), ("inside", inside)):
            want = xs ^ point
            if tag == "inside":
                assert np.flatnonzero(~want.any(axis=1)).tolist() == [(5 * n) // 7]
            for off in C.OFFSETS:
                (got,), prof = run(lib, W, [], (off,), [n], lambda p, o: lib.domain_offsets_dev(basis, shift, point, o[0], words=W))
                assert np.array_equal(got, want), (NAME[W], m, kind, tag, off)
                assert_one_row(prof, W, "domain_offsets", bool(off), n * 8 * W, (m, kind, tag, off))


def check_vanishing_evals(lib, W, m, dim):
    """the vanishing subspace spanned by a prefix of the domain's basis and by unrelated vectors, with a non-zero shift: constant + prod (x + s)"""
    n = 1 << m
    for kind in ("standard", "seeded"):
        basis, shift = domain(m, W, kind)
        xs = oracle.all_subset_sums(basis, shift)
        constant = seeded("vanishing constant %d %d" % (m, dim), 1, W)[0]
        for tag, vb in (("prefix", basis[:dim]), ("unrelated", seeded("vanishing basis %d %d" % (m, dim), dim, W))):
            vshift = seeded("vanishing shift %d %d %s" % (m, dim, tag), 1, W)[0]
            want = H.vanishing_over(xs, oracle.all_subset_sums(vb, vshift)) ^ constant
            for off in C.OFFSETS:
                (got,), prof = run(lib, W, [], (off,), [n], lambda p, o: lib.vanishing_evals_dev(basis, shift, vb, vshift, constant, o[0], words=W))
                assert np.array_equal(got, want), (NAME[W], m, dim, kind, tag, off)
                assert_one_row(prof, W, "vanishing_evals", bool(off), n * 8 * W, (m, dim, kind, tag, off))


def check_domain_refusals(lib, W):
    basis, shift = domain(5, W)
    big = oracle.standard_basis(41, W) if W > 1 else np.arange(1, 42, dtype=np.uint64).reshape(41, 1)
    with C.Device(lib, W) as dev:
        out = dev.empty(8 * W * 32)
        with pytest.raises(ValueError, match="domain dimension too large"):
            lib.domain_offsets_dev(big, shift, shift, out, words=W)
        with pytest.raises(ValueError, match="domain dimension too large"):
            lib.vanishing_evals_dev(big, shift, basis[:2], shift, shift, out, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.domain_offsets_dev(basis, shift, shift, 0, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.vanishing_evals_dev(basis, shift, basis[:2], shift, shift, 0, words=W)


# ---- the rational combination ----
def rational_expected(Ns, Ds, coef):
    W = coef.shape[1]
    numer = np.zeros_like(Ns[0])
    denom = Ds[0].copy()
    for d in Ds[1:]:
        denom = oracle.gf_mul(denom, d)
    for i, nmr in enumerate(Ns):
        cur = oracle.gf_mul(nmr, np.ascontiguousarray(np.broadcast_to(coef[i], nmr.shape)))
        for k, d in enumerate(Ds):
            if k != i:
                cur = oracle.gf_mul(cur, d)
        numer = numer ^ cur
    return numer, denom


def rational_call(lib, W, num, coef, n):
    return lambda p, o: lib.rational_combine_dev(p[:num], p[num:], coef, n, o[0], o[1], words=W)


def check_rational_combine(lib, W, num, n):
    Ns = [seeded("rational N %d %d %d" % (num, n, i), n, W) for i in range(num)]
    Ds = [seeded("rational D %d %d %d" % (num, n, i), n, W) for i in range(num)]
    coef = seeded("rational c %d %d" % (num, n), num, W)
    want = rational_expected(Ns, Ds, coef)
    vectors = 2 * num + 2
    for offs in [(0,) * vectors, (8,) * vectors, (0,) * (vectors - 1) + (8,), (0,) * (num - 1) + (8,) + (0,) * (num + 2)]:
        got, prof = run(lib, W, Ns + Ds, offs, [n, n], rational_call(lib, W, num, coef, n))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (NAME[W], num, n, offs)
        assert_one_row(prof, W, "rational_combine", bool(any(offs)), n * 8 * W * vectors, (num, n, offs))


def check_rational_refusals(lib, W):
    n = 16
    with C.Device(lib, W) as dev:
        v = [dev.put(seeded("rational refused %d" % i, n, W)) for i in range(5)]
        oN, oD = dev.empty(8 * W * n), dev.empty(8 * W * n)
        fn = getattr(lib.c, "iopx_rational_combine_%s_dev" % NAME[W])
        coef = np.ascontiguousarray(seeded("rational refused c", 5, W))
        for num in (0, 5):
            ptrs = (C.VP * 5)(*v)
            with pytest.raises(ValueError, match="Expected same number of evaluations as in registration."):
                lib._check(fn(ptrs, ptrs, num, coef.ctypes.data_as(C.U64P), n, C.VP(oN), C.VP(oD)))
        with pytest.raises(ValueError, match="null oracle"):
            lib.rational_combine_dev([v[0], 0], [v[1], v[2]], coef[:2], n, oN, oD, words=W)
        with pytest.raises(ValueError, match="null oracle"):
            lib.rational_combine_dev([v[0], v[1]], [v[2], 0], coef[:2], n, oN, oD, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.rational_combine_dev([v[0]], [v[1]], coef[:1], n, 0, oD, words=W)


# ---- the rational sumcheck's constraint oracle ----
def power_of_two(xs, k):
    """x^(2^k) row by row"""
    for _ in range(k):
        xs = oracle.gf_mul(xs, xs)
    return xs


def constraint_setup(W, m, k, kind, mu):
    n = 1 << m
    basis, shift = domain(m, W, kind)
    kshift = zero(W) if kind == "standard" else seeded("summation shift %d %d" % (m, k), 1, W)[0]
    xs = oracle.all_subset_sums(basis, shift)
    assert xs.any(axis=1).all(), "the codeword domain holds zero"
    Z = H.vanishing_over(xs, oracle.all_subset_sums(basis[:k], kshift))
    assert Z.any(axis=1).all(), "the codeword domain meets K"
    eps = H.product(oracle.all_subset_sums(basis[:k], zero(W))[1:], W)
    c = oracle.gf_mul(oracle.gf_inv(eps.reshape(1, W)), mu.reshape(1, W))[0]
    xinv = oracle.gf_inv(xs)
    p, N, D = (seeded("constraint %s %d %d" % (t, m, k), n, W) for t in "pND")
    middle = oracle.gf_mul(oracle.gf_mul(power_of_two(xs, k), xinv), np.ascontiguousarray(np.broadcast_to(c, xs.shape)))
    rhs = oracle.gf_mul(D, p ^ middle) ^ N
    return basis, shift, kshift, xinv, p, N, D, Z, rhs


def constraint_call(lib, W, basis, shift, k, kshift, mu):
    return lambda ptr, o: lib.rational_sumcheck_constraint_dev(ptr[0], ptr[1], ptr[2], ptr[3], basis, shift, k, kshift, mu, o[0], words=W)


def check_constraint(lib, W, m, k):
    n = 1 << m
    for kind in ("standard", "seeded"):
        for mu in (zero(W), seeded("claimed sum %d %d" % (m, k), 1, W)[0]):
            basis, shift, kshift, xinv, p, N, D, Z, rhs = constraint_setup(W, m, k, kind, mu)
            for offs in [(0,) * 5, (8,) * 5, (0, 0, 0, 8, 0), (0, 0, 0, 0, 8)]:
                (got,), prof = run(lib, W, [p, N, D, xinv], offs, [n], constraint_call(lib, W, basis, shift, k, kshift, mu))
                assert np.array_equal(oracle.gf_mul(got, Z), rhs), (NAME[W], m, k, kind, bool(mu.any()), offs)
                assert_one_row(prof, W, "rational_sumcheck_constraint", bool(any(offs)), n * 8 * W * 5, (m, k, kind, offs))


def check_constraint_refusals(lib, W):
    m, k = 5, 2
    n = 1 << m
    basis, shift = domain(m, W)
    dependent = basis.copy()
    dependent[1] = dependent[0]
    with C.Device(lib, W) as dev:
        v = dev.put(seeded("constraint refused", n, W))
        out = dev.empty(8 * W * n)
        with pytest.raises(ValueError, match="the summation domain must be spanned by a prefix of the codeword domain's basis"):
            lib.rational_sumcheck_constraint_dev(v, v, v, v, basis, shift, m + 1, zero(W), zero(W), out, words=W)
        big = oracle.standard_basis(41, W) if W > 1 else np.arange(1, 42, dtype=np.uint64).reshape(41, 1)
        with pytest.raises(ValueError, match="the summation domain must be spanned by a prefix of the codeword domain's basis"):
            lib.rational_sumcheck_constraint_dev(v, v, v, v, big, shift, 2, zero(W), zero(W), out, words=W)
        with pytest.raises(ValueError, match="the summation domain's basis is linearly dependent"):
            lib.rational_sumcheck_constraint_dev(v, v, v, v, dependent, shift, k, zero(W), zero(W), out, words=W)
        with pytest.raises(ValueError, match="the codeword domain intersects the summation domain"):
            lib.rational_sumcheck_constraint_dev(v, v, v, v, basis, zero(W), k, zero(W), zero(W), out, words=W)
        for args in ((0, v, v, v), (v, 0, v, v), (v, v, 0, v), (v, v, v, 0)):
            with pytest.raises(ValueError, match="null argument"):
                lib.rational_sumcheck_constraint_dev(*args, basis, shift, k, zero(W), zero(W), out, words=W)


def check_constraint_table_turnover(lib, W):
    """the first pair of domains again after 70 others have gone through the entry (the library keeps the tables of 64 pairs of domains)"""
    m, k = 6, 2
    n = 1 << m
    mu = seeded("turnover sum", 1, W)[0]
    basis, shift, kshift, xinv, p, N, D, Z, rhs = constraint_setup(W, m, k, "standard", mu)
    others = [M.elem(W, C.top(W) | ((t + 1) << 8)) for t in range(70)]
    with C.Device(lib, W) as dev:
        pp, pN, pD, px, out = dev.put(p), dev.put(N), dev.put(D), dev.put(xinv), dev.empty(8 * W * n)
        for s in [shift] + others + [shift]:
            lib.rational_sumcheck_constraint_dev(pp, pN, pD, px, basis, s, k, kshift, mu, out, words=W)
            if s is shift:
                assert np.array_equal(oracle.gf_mul(dev.get(out, n), Z), rhs), NAME[W]


# ---- the native prover over gf64 under IOPX_GFX_FRACTAL=1 ----
def first_difference(mine, ref):
    return next((i for i, (a, b) in enumerate(zip(mine, ref)) if a != b), min(len(mine), len(ref))), len(mine), len(ref)


def flip_middle_bit(t):
    b = bytearray(t)
    b[len(b) // 2] ^= 1
    return bytes(b)


def native_index_and_prove(lib, log_n, k, rs_extra, loc, proofs=1, warm=False, profile=False):
    import libiop_amd as la
    n = 1 << log_n
    inst = lib.aurora_example_instance(la.FIELD_GF64, n, k, n - 1, SEED)
    try:
        with C.options(lib, **{OPTION: 1}):
            roots = lib.fractal_index(inst, 128, rs_extra, loc)
            if warm:
                lib.aurora_instance_warm(inst, fractal=True, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
            out = []
            for _ in range(proofs):
                if profile:
                    lib.profile_begin()
                out.append(lib.fractal_prove(inst, 128, rs_extra, loc))
            prof = lib.profile_report() if profile else None
        return [bytes(r) for r in roots], out, prof
    finally:
        lib.aurora_instance_free(inst)


_ORACLE = {}


def oracle_proof(case):
    """the oracle's (transcript, index roots): computed once per tuple and shared"""
    if case not in _ORACLE:
        log_n, k, rs_extra, loc = case
        _ORACLE[case] = oracle.fractal_prove(oracle.FIELD_GF64, log_n, k, SEED, rs_extra=rs_extra, localization=loc)
    return _ORACLE[case]


def check_native_prover(lib, case):
    log_n, k, rs_extra, loc = case
    ref, ref_roots = oracle_proof(case)
    roots, (mine,), _ = native_index_and_prove(lib, *case)
    assert roots == ref_roots, "index Merkle roots differ"
    assert mine == ref, first_difference(mine, ref)
    assert oracle.fractal_verify(oracle.FIELD_GF64, log_n, k, SEED, mine, roots, rs_extra=rs_extra, localization=loc)
    assert not oracle.fractal_verify(oracle.FIELD_GF64, log_n, k, SEED, flip_middle_bit(mine), roots, rs_extra=rs_extra, localization=loc)


def check_native_second_proof_and_warm(lib):
    case = NATIVE_TUPLES[0]
    ref, ref_roots = oracle_proof(case)
    roots, proofs, _ = native_index_and_prove(lib, *case, proofs=2)
    assert roots == ref_roots and proofs[0] == ref and proofs[1] == ref
    roots, proofs, _ = native_index_and_prove(lib, *case, warm=True)
    assert roots == ref_roots and proofs[0] == ref


def check_native_hand_built(lib):
    """gf64_aurora_cases.hand_built_system through iopx_aurora_instance_create: the oracle's bytes; with one bit of the assignment flipped the same index
    roots, the oracle's bytes for that assignment, and the oracle's verifier rejects"""
    import libiop_amd as la
    matrices, z, k, rs_extra, loc = G64.hand_built_system()
    bad = z.copy()
    bad[k + 17, 0] ^= np.uint64(1 << 63)                         # auxiliary[17]
    nv = z.shape[0]
    good_ref, good_roots = oracle.fractal_prove_csr(oracle.FIELD_GF64, matrices, nv, k, z, rs_extra=rs_extra, localization=loc)
    bad_ref, bad_roots = oracle.fractal_prove_csr(oracle.FIELD_GF64, matrices, nv, k, bad, rs_extra=rs_extra, localization=loc)
    assert good_roots == bad_roots and good_ref != bad_ref
    for assignment, ref, accepted in ((z, good_ref, True), (bad, bad_ref, False)):
        inst = lib.aurora_instance(la.FIELD_GF64, matrices, nv, k, assignment)
        try:
            with C.options(lib, **{OPTION: 1}):
                roots = [bytes(r) for r in lib.fractal_index(inst, 128, rs_extra, loc)]
                mine = lib.fractal_prove(inst, 128, rs_extra, loc)
        finally:
            lib.aurora_instance_free(inst)
        assert roots == good_roots
        assert mine == ref, first_difference(mine, ref)
        assert oracle.fractal_verify_csr(oracle.FIELD_GF64, matrices, nv, k, assignment[:k], mine, roots, rs_extra=rs_extra, localization=loc) == accepted


def check_native_profile(lib):
    """one proof shows each of the five kernels under gf64's stem and no kernel of another field's"""
    _, _, prof = native_index_and_prove(lib, *NATIVE_TUPLES[0], profile=True)
    for kernel in KERNELS:
        assert rows_of(prof, 1, kernel), (kernel, sorted(prof))
    foreign = [k for k in prof if k.startswith(("k128_", "k256_")) or k.endswith(("_gf192", "_fp3")) or k.startswith("k_bn_")]
    assert not foreign, foreign


def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gf64_fractal.json")) as f:
        return {e["log_n"]: e for e in json.load(f)["fractal"] if e["field"] == "gf64" and e["seed"] == SEED}


def check_native_digest(lib, log_n):
    pin = golden_digests()[log_n]
    assert pin["accepted"]
    roots, (mine,), _ = native_index_and_prove(lib, log_n, pin["num_inputs"], pin["rs_extra"], pin["localization"])
    assert [r.hex() for r in roots] == pin["index_roots"]
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])


# ---- the Python prover over GF64FractalOps ----
def check_python_prover(lib, torch, device, case):
    from libiop_amd import domains, fractal, r1cs
    log_n, k, rs_extra, loc = case
    n = 1 << log_n
    ops = domains.GF64FractalOps(lib, torch, device, domains.GF64())
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, k, n - 1, SEED)
    params = fractal.FractalParameters(ops.field, cs, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
    prover_index, (roots, messages) = fractal.fractal_snark_indexer(ops, cs, params)
    mine = fractal.fractal_snark_prover(ops, prover_index, cs, primary, auxiliary, params).serialize()
    ref, ref_roots = oracle_proof(case)
    assert messages == [] and [bytes(r) for r in roots] == ref_roots
    assert mine == ref, first_difference(mine, ref)


# ---- what stays refused ----
def check_refusals(lib, torch, device):
    """option off: today's messages over gf64; gf128 and gf256 with the option on as well; GF64AuroraOps.div still raises; with the option on a
    communicator keeps its refusal"""
    import libiop_amd as la
    from libiop_amd import domains
    inst = lib.aurora_example_instance(la.FIELD_GF64, 64, 3, 63, SEED)
    comm = lib.comm_create_replay(0, 1)
    try:
        with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over gf64"):
            lib.fractal_index(inst)
        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over gf64"):
            lib.fractal_prove(inst)
        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over gf64"):
            lib.aurora_instance_warm(inst, fractal=True)
        with C.options(lib, **{OPTION: 1}):
            with pytest.raises(ValueError, match="gf64 has no distributed prover"):
                lib.fractal_index_dist(inst, comm)
            with pytest.raises(ValueError, match="gf64 has no distributed prover"):
                lib.fractal_prove_dist(inst, comm)
            with pytest.raises(ValueError, match="security_parameter 100 is not supported"):
                lib.fractal_index(inst, 100)
            with pytest.raises(AssertionError, match="no index for these parameters"):
                lib.fractal_prove(inst)
    finally:
        lib.comm_destroy(comm)
        lib.aurora_instance_free(inst)
    for W in (2, 4):
        g = M.example(W, 6, 3, 5)
        h = lib.aurora_instance(C.field_code(W), g["matrices"], g["num_variables"], g["num_inputs"], g["z"])
        try:
            for value in (0, 1):
                with C.options(lib, **{OPTION: value}):
                    with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over " + NAME[W]):
                        lib.fractal_index(h)
                    with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over " + NAME[W]):
                        lib.fractal_prove(h)
        finally:
            lib.aurora_instance_free(h)
    ops = domains.GF64AuroraOps(lib, torch, device, domains.GF64())
    for name in ("div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine", "rational_sumcheck_constraint"):
        with pytest.raises(NotImplementedError, match=r"gf64: DeviceOps\.%s has no GF\(2\^64\) entry" % name):
            getattr(ops, name)()
    plain = domains.DeviceOps(lib, torch, device, domains.GF64())
    assert type(plain) is domains.GF64DeviceOps
    with pytest.raises(NotImplementedError, match=r"gf64: DeviceOps\.div has no GF\(2\^64\) entry"):
        plain.div()


def check_other_fields_unchanged(lib, torch, device):
    """gf192 and edwards Fr Fractal transcripts after gf64 Fractal proofs in this process: one case each of tests/fractal_cases.py"""
    import fractal_cases
    fractal_cases.check_transcript_equals_oracle(lib, torch, device, "gf192", 6, 3, SEED)
    fractal_cases.check_transcript_equals_oracle(lib, torch, device, "edwards_Fr", 6, 3, SEED)
