"""Cases for the GF(2^128) arm (libiop_amd/csrc/gf128.hip): product and inverse, additive FFT / IFFT / LDE, FRI fold and domain chain,
LDT combination, the 64-bit and 128-bit access paths, and the generic Merkle / query-response path on 16-byte elements.  Shared by
tests/test_gf128_emu.py (CPU emulation), tests/test_gpu_gf128.py (MI355X) and tests/test_gf128_binding.py: every function takes the Library
under test.  Expected values come from `oracle` at run time, except the product, which is also checked against the shift-and-xor model
below.  The cases mirror tests/gf64_cases.py at two words per element.

Elements are (n, 2) uint64 arrays: libff gf128's layout, two little-endian words, x^128 + x^7 + x^2 + x + 1."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import oracle

W = 2
MASK64 = (1 << 64) - 1
MASK = (1 << 128) - 1
# 0, 1, the reduction polynomial's tail, x^63, x^64 (the word boundary), x^127, all ones, and operands whose products reach bits 248 - 254
EDGE = [0, 1, 0x87, 3, 1 << 63, 1 << 64, (1 << 64) + 1, 1 << 127, (1 << 127) + 1, MASK, (1 << 127) | (1 << 121) | 1, (1 << 127) | (1 << 126) | (1 << 64)]
U64P = ctypes.POINTER(ctypes.c_uint64)
NAMES = ["IOPX_GF128_TILE_BITS", "IOPX_GF128_P1_COLS", "IOPX_GF128_P2_COLS", "IOPX_GF128_P2_TOP"]
TILE_BITS = 11                                   # the default (and largest) IOPX_GF128_TILE_BITS


def model_mul(a, b):
    """shift-and-xor product modulo x^128 + x^7 + x^2 + x + 1, Python integers only"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 128:
            a ^= (1 << 128) | 0x87
    return r


def clmul(a, b):
    """the unreduced carry-less product"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
    return r


def seeded(tag, count):
    seed = int.from_bytes(hashlib.sha256(b"gf128 " + tag.encode()).digest()[:8], "little")
    return np.random.default_rng(seed).integers(0, MASK64, size=(count, 2), dtype=np.uint64, endpoint=True)


def ints(a):
    return [int(r[0]) | (int(r[1]) << 64) for r in np.asarray(a, dtype=np.uint64).reshape(-1, 2)]


def col(values):
    return np.array([[v & MASK64, v >> 64] for v in values], dtype=np.uint64).reshape(-1, 2)


def elem(v):
    return np.array([v & MASK64, v >> 64], dtype=np.uint64)


def std_basis(m):
    return oracle.standard_basis(m, W)


def high_basis(m):
    """x^(64 - m // 2 + i), i < m: the vectors straddle the word boundary (for m >= 2 at least one is >= x^64)"""
    return col([1 << (64 - m // 2 + i) for i in range(m)])


def fft_shifts(m):
    return [("0", 0), ("1<<m", 1 << m), ("bit127", (1 << 127) | (0xABCDEF << 64) | 0x1234567)]


def derived_domains(shift):
    """the derived domains of fri_domains_additive(standard_basis(12), shift, [1, 2, 3]): non-standard bases of dimension 11, 9, 6"""
    return oracle.fri_domains_additive(std_basis(12), elem(shift), [1, 2, 3])


def fft_domains():
    """(name, basis, shift) of every FFT / IFFT case: gf64_cases.fft_domains() with shifts that have a high word, plus bases with vectors >= x^64"""
    out = []
    for m in list(range(0, 13)) + [14]:
        for sname, s in fft_shifts(m):
            out.append(("std m=%d shift=%s" % (m, sname), std_basis(m), elem(s)))
    for i, (b, s) in enumerate(derived_domains((1 << 127) | (7 << 64) | 5)):
        out.append(("derived %d" % i, b, s))
    for m in (2, 7, 12):
        out.append(("high m=%d" % m, high_basis(m), elem((1 << 127) | (3 << 100) | 0x99)))
    return out


def coeff_counts(m):
    n = 1 << m
    d = max(m - 2, 0)
    return sorted({c for c in (0, 1, 2, 3, (1 << d) - 1, 1 << d, (1 << d) + 1, n) if 0 <= c <= n})


# ---- 1. product and inverse ----
def mul_pairs():
    a = [x for x in EDGE for _ in EDGE] + ints(seeded("mul a", 2048))
    b = [y for _ in EDGE for y in EDGE] + ints(seeded("mul b", 2048))
    return a, b


def check_product(lib):
    a, b = mul_pairs()
    assert any(clmul(x, y) >> 248 for x, y in zip(a[:len(EDGE) ** 2], b)), "no edge pair reaches bits 248 - 254: the second fold step is not exercised"
    assert model_mul(1 << 127, 2) == 0x87
    want = [model_mul(x, y) for x, y in zip(a, b)]
    got = lib.gf128_mul(col(a), col(b))
    assert ints(got) == want
    assert np.array_equal(got, oracle.gf_mul(col(a), col(b)))
    for x, y, w in list(zip(a, b, want))[:len(EDGE) ** 2 + 64]:
        assert ints(lib.gf128_host_mul(elem(x), elem(y))) == [w], (hex(x), hex(y))
    for count in (1, 63, 64, 65, 1000):
        assert ints(lib.gf128_mul(col(a[:count]), col(b[:count]))) == want[:count], count


def check_inverse(lib):
    vals = [v for v in EDGE if v] + [v for v in ints(seeded("inv", 256)) if v]
    inv = lib.gf128_inv(col(vals))
    assert np.array_equal(inv, oracle.gf_inv(col(vals)))
    assert [model_mul(v, i) for v, i in zip(vals, ints(inv))] == [1] * len(vals)
    assert ints(lib.gf128_inv(col([0]))) == [0]                  # a^(2^128 - 2), as the gf192 vector entry
    for count in (1, 63, 64, 65):
        assert np.array_equal(lib.gf128_inv(col(vals[:count])), inv[:count]), count
    for v in vals[:24]:
        assert model_mul(v, ints(lib.gf128_inverse_host(elem(v)))[0]) == 1
    with pytest.raises(ValueError, match="inverse of zero"):
        lib.gf128_inverse_host(elem(0))


# ---- 2. / 4. FFT and IFFT ----
def check_fft(lib, max_m=None):
    """max_m: only the domains of dimension <= max_m (for runs that cost more per element); the default takes them all"""
    ran = 0
    assert any(int(b[:, 1].max(initial=0)) for _, b, _ in fft_domains()) and any(int(s[1]) for _, _, s in fft_domains())
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        if max_m is not None and m > max_m:
            continue
        for count in coeff_counts(m):
            coeffs = seeded("fft %s %d" % (name, count), count)
            got = lib.additive_FFT_gf128(coeffs, basis, shift)
            assert np.array_equal(got, oracle.additive_fft(coeffs, basis, shift)), (name, count)
            if m <= 8:
                assert np.array_equal(got, oracle.naive_fft(coeffs, basis, shift)), (name, count)
            ran += 1
    assert ran == sum(len(coeff_counts(b.shape[0])) for _, b, _ in fft_domains() if max_m is None or b.shape[0] <= max_m)
    assert max_m is not None or ran > 250


def check_ifft(lib):
    ran = 0
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        evals = seeded("ifft %s" % name, 1 << m)
        got = lib.additive_IFFT_gf128(evals, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft(evals, basis, shift)), name
        assert np.array_equal(lib.additive_FFT_gf128(got, basis, shift), evals), name       # FFT o IFFT = id
        coeffs = seeded("roundtrip %s" % name, 1 << m)
        assert np.array_equal(lib.additive_IFFT_gf128(lib.additive_FFT_gf128(coeffs, basis, shift), basis, shift), coeffs), name
        ran += 1
    assert ran == 14 * 3 + 3 + 3


def check_ifft_in_place_and_known_degree(lib):
    for m in (0, 5, 11):
        basis, shift = std_basis(m), elem((1 << 127) | 9)
        n = 1 << m
        evals = seeded("in place %d" % m, n)
        d = lib.malloc(16 * n)
        try:
            lib.h2d(d, evals)
            lib.additive_IFFT_dev(d, basis, shift, d, words=2)
            out = np.empty((n, 2), dtype=np.uint64)
            lib.d2h(out, d)
        finally:
            lib.free(d)
        assert np.array_equal(out, oracle.additive_ifft(evals, basis, shift)), m
    basis, shift = derived_domains((5 << 64) | 77)[0]
    evals = seeded("known degree", 1 << 11)
    for degree in (1, 2, 33, 64, 700, 2048):
        got = lib.IFFT_of_known_degree_gf128(evals, degree, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft_known_degree(evals, degree, basis, shift)), degree


# gf64_cases.SCHEDULES with the tile bits reduced by one where the value would exceed the gf128 maximum (12 -> 11)
SCHEDULES = [
    # (options, m): which kernels the transform of 2^m coefficients then takes
    ({"IOPX_GF128_TILE_BITS": 11}, 9),                                                                   # defaults: one k128_phase1 pass, k128_bfly_edge alone with 4 tiles per workgroup
    ({"IOPX_GF128_TILE_BITS": 4, "IOPX_GF128_P1_COLS": 1, "IOPX_GF128_P2_COLS": 1, "IOPX_GF128_P2_TOP": 1}, 5),    # one chunked phase-1 level, one k128_bfly_upper pass
    ({"IOPX_GF128_TILE_BITS": 4, "IOPX_GF128_P1_COLS": 1, "IOPX_GF128_P2_COLS": 1, "IOPX_GF128_P2_TOP": 1}, 9),    # several chunks per level, two upper passes, strided tiles (h > c)
    ({"IOPX_GF128_TILE_BITS": 5, "IOPX_GF128_P1_COLS": 0, "IOPX_GF128_P2_COLS": 0, "IOPX_GF128_P2_TOP": 0}, 10),   # single-column tiles, no natural-order runs in the last pass
    ({"IOPX_GF128_TILE_BITS": 6, "IOPX_GF128_P1_COLS": 3, "IOPX_GF128_P2_COLS": 4, "IOPX_GF128_P2_TOP": 3}, 11),   # wide columns: c limited by h in the phase-1 chunks
    ({"IOPX_GF128_TILE_BITS": 3, "IOPX_GF128_P1_COLS": 1, "IOPX_GF128_P2_COLS": 1, "IOPX_GF128_P2_TOP": 2}, 7),    # the smallest tile: rows of 2^2, c_top = tile - 1
]


def check_schedules(lib):
    """Each pass kind of the schedule at the smallest m where it applies, reached through the tuning options (looked up when a plan is built),
    as gf64_cases.check_schedules: full transforms, the LDE with staged coset groups (n_coeffs = 2^(m-2)) and the IFFT under each setting."""
    ran = 0
    try:
        for opts, m in SCHEDULES:
            for k in NAMES:
                lib.clear_option(k)
            for k, v in opts.items():
                lib.set_option(k, v)
            lib.clear_plans()
            for basis, shift in ((std_basis(m), elem((1 << 127) | 3)), tuple(derived_domains(5 << 64)[0]) if m == 11 else (high_basis(m), elem(1 << 70))):
                n = 1 << m
                for count in (n, n - 1, (n >> 2), (n >> 2) + 1):
                    coeffs = seeded("sched %d %d" % (m, count), count)
                    assert np.array_equal(lib.additive_FFT_gf128(coeffs, basis, shift), oracle.additive_fft(coeffs, basis, shift)), (opts, m, count)
                evals = seeded("sched ifft %d" % m, n)
                assert np.array_equal(lib.additive_IFFT_gf128(evals, basis, shift), oracle.additive_ifft(evals, basis, shift)), (opts, m)
                ran += 1
    finally:
        for k in NAMES:
            lib.clear_option(k)
        lib.clear_plans()
    assert ran == 2 * len(SCHEDULES)


# ---- 3. LDE coset ranges ----
def _lde(lib, dc, n_coeffs, basis, shift, begin, count, do, d):
    lib.additive_LDE_dev(dc, n_coeffs, basis, shift, begin, count, do, words=2)
    out = np.empty((count << d, 2), dtype=np.uint64)
    lib.d2h(out, do)
    return out


def check_lde_ranges(lib):
    m, d = 12, 7
    basis, shift = std_basis(m), elem((1 << 127) | 0x55)
    coeffs = seeded("lde", (1 << d) - 3)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(16 << d), lib.malloc(16 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 1), (5, 3), (31, 1), (0, 32)):
            assert np.array_equal(_lde(lib, dc, coeffs.shape[0], basis, shift, begin, count, do, d), full[begin << d:(begin + count) << d]), (begin, count)
        for begin, count in ((32, 1), (31, 2), (0, 0), (0, 33)):
            with pytest.raises(ValueError, match="outside the 32 cosets"):
                lib.additive_LDE_dev(dc, coeffs.shape[0], basis, shift, begin, count, do, words=2)
    finally:
        lib.free(dc)
        lib.free(do)


def check_lde_upper_pass_whole(lib):
    """2^(T+1) coefficients, the smallest count whose plan has a k128_bfly_upper pass with the default tile T, onto m = T + 3: every coset range
    against the oracle's transform, whole; the ranges of more than one coset go through the block-order staging (one group)"""
    d = TILE_BITS + 1
    m = d + 2
    basis, shift = std_basis(m), elem((1 << 127) | 0x55)
    coeffs = seeded("lde upper", 1 << d)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(16 << d), lib.malloc(16 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 4), (1, 3), (3, 1)):
            lib.profile_begin()
            out = _lde(lib, dc, coeffs.shape[0], basis, shift, begin, count, do, d)
            assert lib.profile_report().get("k128_bfly_upper", (0,))[0] >= 1, "the plan has no upper pass"
            assert np.array_equal(out, full[begin << d:(begin + count) << d]), (begin, count)
    finally:
        lib.free(dc)
        lib.free(do)


# ---- the two access paths ----
def _ran(report, stem):
    """(launches of the 128-bit instantiations, launches of the 64-bit ones) of the kernels whose profile name starts with `stem`"""
    wide = sum(v[0] for k, v in report.items() if k.startswith(stem) and not k.endswith("_w64"))
    narrow = sum(v[0] for k, v in report.items() if k.startswith(stem) and k.endswith("_w64"))
    return wide, narrow


def check_alignment(lib):
    """One FFT, one LDE range, one fold and one LDT combination with all buffers 16-byte aligned, then with the input, then the output, at
    a device address 8 mod 16 (16 bytes more, offset by 8): on the aligned call the profile shows 128-bit instantiations only; on the other
    two the kernel that touches the misaligned buffer (k128_pad_copy for a transform's input, k128_bfly_edge for its output, the fold and the
    combination themselves) ran as its 64-bit instantiation, while passes between aligned temporaries keep the 128-bit one.  All equal the oracle."""
    m, d = 9, 7
    n = 1 << m
    basis, shift, x = std_basis(m), elem((1 << 127) | 0x31), elem((9 << 64) | 4)
    coeffs = seeded("align coeffs", n)
    evals = [seeded("align evals %d" % k, n) for k in range(3)]
    degrees, coef = [n, n - 3, n // 2], seeded("align coef", 6)
    want = {
        "fft": oracle.additive_fft(coeffs, basis, shift),
        "lde": oracle.additive_fft(coeffs[:1 << d], basis, shift)[2 << d:4 << d],
        "fold": oracle.fri_fold_additive(evals[0], basis, shift, 4, x),
        "ldt": oracle.ldt_combine_additive(evals, degrees, coef, basis, shift),
    }
    raw = [lib.malloc(16 * n + 16) for _ in range(4)]            # three inputs, one output
    try:
        assert all(p % 16 == 0 for p in raw), "the allocator is expected to hand out 16-byte aligned blocks"
        for off_in, off_out in ((0, 0), (8, 0), (0, 8)):
            ins, out = [p + off_in for p in raw[:3]], raw[3] + off_out
            calls = {
                "fft": (coeffs, "k128_pad_copy" if off_in else "k128_bfly_edge", lambda: lib.additive_FFT_dev(ins[0], n, basis, shift, out, words=2), n),
                "lde": (coeffs, "k128_pad_copy" if off_in else "k128_bfly_edge", lambda: lib.additive_LDE_dev(ins[0], 1 << d, basis, shift, 2, 2, out, words=2), 2 << d),
                "fold": (evals[0], "k128_fri_fold", lambda: lib.fri_fold_dev(ins[0], basis, shift, 4, x, out, words=2), n // 4),
                "ldt": (None, "k128_ldt_combine", lambda: lib.ldt_combine_dev(ins, degrees, coef, basis, shift, out, words=2), n),
            }
            for name, (src, stem, call, n_out) in calls.items():
                if src is None:
                    for p, e in zip(ins, evals):
                        lib.h2d(p, e)
                else:
                    lib.h2d(ins[0], src)
                lib.profile_begin()
                call()
                got = np.empty((n_out, 2), dtype=np.uint64)
                lib.d2h(got, out)
                report = lib.profile_report()
                wide, narrow = _ran(report, stem)
                assert np.array_equal(got, want[name]), (name, off_in, off_out)
                if off_in == 0 and off_out == 0:
                    assert wide >= 1 and _ran(report, "k128_")[1] == 0, (name, report)
                else:
                    assert narrow >= 1 and wide == 0, (name, off_in, off_out, wide, narrow)
    finally:
        for p in raw:
            lib.free(p)


# ---- 5. fold ----
def fold_domains():
    return [("std", std_basis(10), elem((1 << 127) | 0x77))] + [("derived %d" % i, b, s) for i, (b, s) in enumerate(derived_domains((0x1234 << 64) | 0x1234))]


def check_fold(lib):
    x = seeded("fold x", 1)[0]
    ran = 0
    for name, basis, shift in fold_domains():
        m = basis.shape[0]
        f = seeded("fold %s" % name, 1 << m)
        for eta in list(range(0, 6)) + [m]:
            got = lib.evaluate_next_f_i_over_entire_domain_gf128(f, basis, shift, 1 << eta, x)
            assert np.array_equal(got, oracle.fri_fold_additive(f, basis, shift, 1 << eta, x)), (name, eta)
            if eta == 0:
                assert np.array_equal(got, f)
            if eta == m:        # the interpolant of f on the whole domain, at x
                coeffs = oracle.additive_ifft(f, basis, shift)
                assert np.array_equal(got, oracle.poly_eval(coeffs, x).reshape(1, 2)), name
            ran += 1
    assert ran == 4 * 7
    # x on the domain: the fold returns f there (fri_aux.tcc:77-86)
    basis, shift = std_basis(6), elem(1 << 100)
    f = seeded("fold on domain", 64)
    xs = oracle.all_subset_sums(basis, shift)[13]
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf128(f, basis, shift, 4, xs), oracle.fri_fold_additive(f, basis, shift, 4, xs))
    dep = std_basis(6).copy()
    dep[1] = dep[0]
    with pytest.raises(ValueError, match="linearly dependent"):
        lib.evaluate_next_f_i_over_entire_domain_gf128(f, dep, shift, 4, x)


def check_fold_chain(lib):
    """[2, 2, 1] on an LDE of 2^6 coefficients onto m = 11: every folded codeword stays below its degree bound"""
    basis, shift = std_basis(11), elem((1 << 127) | 1)
    f = lib.additive_FFT_gf128(seeded("chain", 1 << 6), basis, shift)
    domains = lib.fri_additive_domains_gf128(basis, shift, [2, 2, 1])
    bound = 1 << 6
    for i, eta in enumerate([2, 2, 1]):
        b, s = domains[i]
        f = lib.evaluate_next_f_i_over_entire_domain_gf128(f, b, s, 1 << eta, seeded("chain x %d" % i, 1)[0])
        bound >>= eta
        nb, ns = domains[i + 1]
        coeffs = lib.additive_IFFT_gf128(f, nb, ns)
        assert coeffs[:bound].any() and not coeffs[bound:].any(), i


# ---- 6. domain chain ----
def check_domain_chain(lib):
    basis, shift = std_basis(12), elem((1 << 127) | 0xABC)
    for loc in ([1, 2, 2], [3, 1]):
        got = lib.fri_additive_domains_gf128(basis, shift, loc)
        want = oracle.fri_domains_additive(basis, shift, loc)
        assert len(got) == len(loc) + 1
        for (gb, gs), (wb, ws) in zip(got[1:], want):
            assert np.array_equal(gb, wb) and np.array_equal(gs.reshape(-1), ws.reshape(-1)), loc
    with pytest.raises(ValueError, match="exceed the domain dimension"):
        lib.fri_additive_domains_gf128(std_basis(3), shift, [2, 2])


# ---- 7. LDT combination ----
LDT_CASES = [
    ("one maximal", [2048]),
    ("seven mixed", [2048, 2047, 2047, 1024, 2046, 2048, 1025]),
    ("bump not a power of two", [1000, 233, 1000 - 7]),
]


def check_ldt(lib):
    m = 11
    for basis, shift in ((std_basis(m), elem((1 << 127) | 0xF0F)), tuple(derived_domains(3 << 64)[0])):
        for name, degrees in LDT_CASES:
            evals = [seeded("ldt %s %d" % (name, k), 1 << m) for k in range(len(degrees))]
            coef = seeded("ldt coef " + name, 2 * len(degrees))
            got = lib.ldt_combine_gf128(evals, degrees, coef, basis, shift)
            assert np.array_equal(got, oracle.ldt_combine_additive(evals, degrees, coef, basis, shift)), name


# ---- 8. pins of the generic paths on 16-byte elements (these pass without the gf128 kernels) ----
def check_merkle_and_queries(lib):
    for num_oracles in (1, 5):
        oracles = [seeded("merkle %d %d" % (num_oracles, k), 64) for k in range(num_oracles)]
        for coset in (1, 2, 4):
            assert np.array_equal(lib.merkle_tree(oracles, coset), oracle.merkle_build(oracles, coset)), (num_oracles, coset)
        ptrs = [lib.malloc(16 * 64) for _ in oracles]
        try:
            for p, o in zip(ptrs, oracles):
                lib.h2d(p, o)
            positions = [0, 63, 17, 17, 32]
            got = np.asarray(lib.query_responses_dev(ptrs, 16, 64, positions)).reshape(len(positions), num_oracles, 2)
            assert np.array_equal(got, np.array([[o[p] for o in oracles] for p in positions], dtype=np.uint64))
        finally:
            for p in ptrs:
                lib.free(p)


# ---- 9. host and device forms, argument checks ----
def check_host_and_device_forms(lib):
    m, basis, shift = 9, std_basis(9), elem(1 << 100)
    n = 1 << m
    coeffs, x = seeded("forms", n - 5), elem((0xDEADBEEF << 64) | 0x12345)
    d_in, d_out = lib.malloc(16 * n), lib.malloc(16 * n)
    try:
        lib.h2d(d_in, coeffs)
        lib.additive_FFT_dev(d_in, coeffs.shape[0], basis, shift, d_out, words=2)
        evals = np.empty((n, 2), dtype=np.uint64)
        lib.d2h(evals, d_out)
        assert np.array_equal(evals, lib.additive_FFT_gf128(coeffs, basis, shift))
        lib.additive_IFFT_dev(d_out, basis, shift, d_in, words=2)
        back = np.empty((n, 2), dtype=np.uint64)
        lib.d2h(back, d_in)
        assert np.array_equal(back, lib.additive_IFFT_gf128(evals, basis, shift))
        lib.fri_fold_dev(d_out, basis, shift, 8, x, d_in, words=2)
        folded = np.empty((n // 8, 2), dtype=np.uint64)
        lib.d2h(folded, d_in)
        assert np.array_equal(folded, lib.evaluate_next_f_i_over_entire_domain_gf128(evals, basis, shift, 8, x))
        lib.h2d(d_in, evals)
        lib.field_add_dev(d_in, d_out, d_out, n, words=2)            # a + a = 0
        lib.d2h(back, d_out)
        assert not back.any()
    finally:
        lib.free(d_in)
        lib.free(d_out)


def check_argument_checks(lib):
    """each refusal carries the gf64 twin's message"""
    c = lib.c
    basis, shift, x = std_basis(4), elem(0), elem(7)
    b1, s1, x1 = basis[:, :1].copy(), shift[:1].copy(), x[:1].copy()
    f = seeded("checks", 16)
    fp = f.ctypes.data_as(U64P)
    big, big1 = std_basis(41), oracle.standard_basis(41, 1)
    arg = lambda g, two, one: (two if g == "gf128" else one).ctypes.data_as(U64P)
    bp, sp, xp, gp = (lambda g: arg(g, basis, b1)), (lambda g: arg(g, shift, s1)), (lambda g: arg(g, x, x1)), (lambda g: arg(g, big, big1))
    calls = [
        ("null basis/shift", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 0, None, 4, sp(g), None)),
        ("null buffer", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 3, bp(g), 4, sp(g), None)),
        ("null buffer", lambda g: getattr(c, "iopx_add_ifft_%s_dev" % g)(None, bp(g), 4, sp(g), None)),
        ("null basis/shift", lambda g: getattr(c, "iopx_add_ifft_%s" % g)(fp, bp(g), 4, None, fp)),
        ("exceed the domain size", lambda g: getattr(c, "iopx_add_fft_%s" % g)(fp, 17, bp(g), 4, sp(g), fp)),
        ("too large", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 0, gp(g), 41, sp(g), None)),
        ("too large", lambda g: getattr(c, "iopx_add_ifft_%s_dev" % g)(None, gp(g), 41, sp(g), None)),
        ("too large", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(None, gp(g), 41, sp(g), 2, xp(g), None)),
        ("null argument", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(None, bp(g), 4, sp(g), 2, xp(g), None)),
        ("not a power of two", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(ctypes.c_void_p(16), bp(g), 4, sp(g), 3, xp(g), ctypes.c_void_p(16))),
        ("exceeds the domain size", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(ctypes.c_void_p(16), bp(g), 4, sp(g), 32, xp(g), ctypes.c_void_p(16))),
        ("null argument", lambda g: getattr(c, "iopx_fri_domains_%s" % g)(None, 4, sp(g), None, 0, None, None)),
        ("null argument", lambda g: getattr(c, "iopx_ldt_combine_%s_dev" % g)(None, 1, None, None, bp(g), 4, sp(g), None)),
        ("null argument", lambda g: getattr(c, "iopx_%s_host_mul" % g)(None, None, None)),
        ("null argument", lambda g: getattr(c, "iopx_%s_inverse_host" % g)(None, None)),
        ("null argument", lambda g: getattr(c, "iopx_%s_mul_dev" % g)(None, None, None, 3)),
        ("null argument", lambda g: getattr(c, "iopx_%s_inv_dev" % g)(None, None, 3)),
    ]
    for text, call in calls:
        msgs = []
        for g in ("gf64", "gf128"):
            with pytest.raises(ValueError, match=text) as e:
                lib._check(call(g))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf128(f, basis, shift, 3, x)
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf128(f, basis, shift, 32, x)
    dep = std_basis(4).copy()
    dep[2] = dep[0] ^ dep[1]
    with pytest.raises(ValueError, match="additive FFT: basis vectors are linearly dependent"):
        lib.additive_FFT_gf128(f, dep, shift)
    # the size-zero and size-one edge cases are accepted as the twin accepts them
    assert np.array_equal(lib.additive_FFT_gf128(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_IFFT_gf128(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_FFT_gf128(f[:0], basis, shift), np.zeros((16, 2), dtype=np.uint64))
    assert np.array_equal(lib.additive_FFT_gf128(f[:1], basis, shift), np.repeat(f[:1], 16, axis=0))
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf128(f, basis, shift, 1, x), f)


# ---- 10. the other fields are unchanged ----
def check_wordless_calls_unchanged(lib):
    """the eight `_dev` methods that took a words= keyword, called without it: gf192, as before"""
    m = 6
    n = 1 << m
    basis, shift = oracle.standard_basis(m, 3), np.array([1 << m, 0, 7], dtype=np.uint64)
    rng = np.random.default_rng(128)
    coeffs = rng.integers(0, MASK64, size=(n, 3), dtype=np.uint64, endpoint=True)
    other = rng.integers(0, MASK64, size=(n, 3), dtype=np.uint64, endpoint=True)
    x = rng.integers(0, MASK64, size=3, dtype=np.uint64, endpoint=True)
    coef = rng.integers(0, MASK64, size=(4, 3), dtype=np.uint64, endpoint=True)
    d = [lib.malloc(24 * n) for _ in range(3)]

    def back(p, count=n):
        out = np.empty((count, 3), dtype=np.uint64)
        lib.d2h(out, p)
        return out
    try:
        lib.h2d(d[0], coeffs)
        lib.additive_FFT_dev(d[0], n, basis, shift, d[1])
        evals = back(d[1])
        assert np.array_equal(evals, oracle.additive_fft(coeffs, basis, shift))
        lib.additive_LDE_dev(d[0], n // 4, basis, shift, 1, 2, d[2])
        assert np.array_equal(back(d[2], n // 2), oracle.additive_fft(coeffs[:n // 4], basis, shift)[n // 4:3 * n // 4])
        lib.additive_IFFT_dev(d[1], basis, shift, d[2])
        assert np.array_equal(back(d[2]), coeffs)
        lib.fri_fold_dev(d[1], basis, shift, 4, x, d[2])
        assert np.array_equal(back(d[2], n // 4), oracle.fri_fold_additive(evals, basis, shift, 4, x))
        lib.h2d(d[2], other)
        lib.ldt_combine_dev([d[1], d[2]], [n, n - 5], coef, basis, shift, d[0])
        assert np.array_equal(back(d[0]), oracle.ldt_combine_additive([evals, other], [n, n - 5], coef, basis, shift))
        lib.gf192_mul_dev(d[1], d[2], d[0], n)
        assert np.array_equal(back(d[0]), oracle.gf_mul(evals, other))
        lib.field_inv_dev(d[1], d[0], n)
        assert np.array_equal(back(d[0]), oracle.gf_inv(evals))
        lib.field_add_dev(d[1], d[2], d[0], n)
        assert np.array_equal(back(d[0]), evals ^ other)
    finally:
        for p in d:
            lib.free(p)


def check_fri_snark_other_fields_unchanged(lib, torch, device):
    """the FRI SNARK over GF192, GF64 and EdwardsFr still produces its old bytes"""
    from libiop_amd import domains, fri, r1cs
    dim, rs_extra, loc, interactions, queries = 8, 2, 2, 1, 6
    for code, cls, ops_cls in ((oracle.FIELD_GF192, domains.GF192, domains.DeviceOps), (oracle.FIELD_GF64, domains.GF64, domains.GF64DeviceOps),
                               (oracle.FIELD_EDWARDS, domains.EdwardsFr, domains.DeviceOps)):
        ops = domains.DeviceOps(lib, torch, device, cls())
        assert type(ops) is ops_cls
        params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
        coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (dim - rs_extra))
        mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=ops.upload(coeffs)).serialize()
        assert mine == oracle.fri_snark_prove(code, dim, rs_extra, loc, interactions, queries, 5), cls.__name__


# ---- 11. FRI-only SNARK ----
FRI_SNARK_TUPLES = [(8, 2, 2, 1, 6), (10, 2, 1, 1, 4), (12, 3, 3, 2, 8)]      # (dim, rs_extra, loc, interactions, queries)
GF64_SIZES = [2272, 3648, 6088]


@functools.lru_cache(maxsize=None)
def model_bytes(words, t):
    """the model's transcript of tuple t with seed 5, computed once and shared by the tests that compare with it"""
    import gf128_fri_snark_model as M
    return M.prove(words, *t, seed=5)


def check_model_reproduces_oracle():
    """the trust condition of tests/gf128_fri_snark_model.py: at one and three words it is the oracle's prover, byte for byte"""
    import gf128_fri_snark_model as M
    for words, code in ((1, oracle.FIELD_GF64), (3, oracle.FIELD_GF192)):
        for t, size in zip(FRI_SNARK_TUPLES, GF64_SIZES):
            ref = oracle.fri_snark_prove(code, *t, 5)
            assert words != 1 or len(ref) == size
            assert model_bytes(words, t) == ref, (words, t)


def check_fri_snark(lib, torch, device, trust=True):
    """fri.fri_snark_prover over domains.GF128 and the native prover against the model, byte for byte, and against each other.  trust: first
    hold the model to its trust condition (the CPU leg does; the GPU leg relies on it)"""
    import libiop_amd
    from libiop_amd import domains, fri, host, r1cs
    if trust:
        check_model_reproduces_oracle()
    field = domains.GF128()
    hc, ohc = host.Blake2bHashchain(), oracle.Hashchain()
    for n in (1, 2, 5):
        assert np.array_equal(field.squeeze(hc, n), ohc.squeeze(n, 2)), n
    ops = domains.DeviceOps(lib, torch, device, field)
    assert type(ops) is domains.GF128DeviceOps
    for t in FRI_SNARK_TUPLES:
        dim, rs_extra, loc, interactions, queries = t
        params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
        coeffs = r1cs.seeded_elements(field, 5, 1 << (dim - rs_extra))
        want = model_bytes(2, t)
        d_coeffs = ops.upload(coeffs)
        mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=d_coeffs).serialize()
        assert mine == want, (t, next((i for i, (a, b) in enumerate(zip(mine, want)) if a != b), min(len(mine), len(want))), len(mine), len(want))
        nat = lib.fri_snark_prove(libiop_amd.FIELD_GF128, d_coeffs.data_ptr(), coeffs.shape[0], dim, rs_extra, loc, interactions, queries)
        assert nat == want, t
        assert nat == mine, t
    with pytest.raises(NotImplementedError, match="gf128"):
        ops.rowcheck(None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="gf128"):
        ops.mul(None, None)


def check_native_refusals(lib, torch, device):
    """Aurora instances over field 5, Poseidon and a communicator are refused by name; the FRI prover still proves afterwards"""
    import libiop_amd
    from libiop_amd import domains, r1cs
    with pytest.raises(ValueError, match="only the FRI-only SNARK is built over gf128"):
        lib.aurora_example_instance(libiop_amd.FIELD_GF128, 16, 3, 15, 1)
    ops = domains.DeviceOps(lib, torch, device, domains.GF128())
    t = FRI_SNARK_TUPLES[0]
    coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (t[0] - t[1]))
    d_coeffs = ops.upload(coeffs)
    with pytest.raises(ValueError, match="gf128 proves with BLAKE2b"):
        lib.fri_snark_prove(libiop_amd.FIELD_GF128, d_coeffs.data_ptr(), coeffs.shape[0], *t, hash=libiop_amd.HASH_POSEIDON_HIGH_ALPHA)
    with pytest.raises(ValueError, match="gf128 has no distributed prover"):
        lib.fri_snark_prove(libiop_amd.FIELD_GF128, d_coeffs.data_ptr(), coeffs.shape[0], *t, comm=ctypes.c_void_p(16))
    assert lib.fri_snark_prove(libiop_amd.FIELD_GF128, d_coeffs.data_ptr(), coeffs.shape[0], *t) == model_bytes(2, t)
