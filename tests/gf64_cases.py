"""Cases for the GF(2^64) arm (libiop_amd/csrc/gf64.hip): product and inverse, additive FFT / IFFT / LDE, FRI fold and domain chain,
LDT combination, and the generic Merkle / query-response path on 8-byte elements.  Shared by tests/test_gf64_emu.py (CPU emulation) and
tests/test_gpu_gf64.py (MI355X): every function takes the Library under test.  Expected values come from `oracle` at run time, except the
product, which is also checked against the shift-and-xor model below.

Elements are (n, 1) uint64 arrays: libff gf64's layout, x^64 + x^4 + x^3 + x + 1."""
import ctypes
import hashlib

import numpy as np
import pytest

import oracle

W = 1
MASK = (1 << 64) - 1
EDGE = [0, 1, 0x1B, 3, 1 << 63, (1 << 63) + 1, MASK, 0x8000000000000001]
U64P = ctypes.POINTER(ctypes.c_uint64)


def model_mul(a, b):
    """shift-and-xor product modulo x^64 + x^4 + x^3 + x + 1, Python integers only"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 64:
            a ^= (1 << 64) | 0x1B
    return r


def seeded(tag, count):
    seed = int.from_bytes(hashlib.sha256(b"gf64 " + tag.encode()).digest()[:8], "little")
    return np.random.default_rng(seed).integers(0, MASK, size=(count, 1), dtype=np.uint64, endpoint=True)


def col(values):
    return np.array([[v] for v in values], dtype=np.uint64).reshape(-1, 1)


def elem(v):
    return np.array([v], dtype=np.uint64)


def std_basis(m):
    return oracle.standard_basis(m, W)


def fft_shifts(m):
    return [("0", 0), ("1<<m", 1 << m), ("bit63", (1 << 63) | 0x1234567)]


def derived_domains(shift):
    """the derived domains of fri_domains_additive(standard_basis(12), shift, [1, 2, 3]): non-standard bases of dimension 11, 9, 6"""
    return oracle.fri_domains_additive(std_basis(12), elem(shift), [1, 2, 3])


def fft_domains():
    """(name, basis, shift) of every FFT / IFFT case"""
    out = []
    for m in list(range(0, 13)) + [14, 16]:
        for sname, s in fft_shifts(m):
            out.append(("std m=%d shift=%s" % (m, sname), std_basis(m), elem(s)))
    for i, (b, s) in enumerate(derived_domains((1 << 63) | 5)):
        out.append(("derived %d" % i, b, s))
    return out


def coeff_counts(m):
    n = 1 << m
    d = max(m - 2, 0)
    return sorted({c for c in (0, 1, 2, 3, (1 << d) - 1, 1 << d, (1 << d) + 1, n) if 0 <= c <= n})


# ---- 1. product and inverse ----
def mul_pairs():
    a = [x for x in EDGE for _ in EDGE] + [int(v) for v in seeded("mul a", 4096)[:, 0]]
    b = [y for _ in EDGE for y in EDGE] + [int(v) for v in seeded("mul b", 4096)[:, 0]]
    return a, b


def check_product(lib):
    a, b = mul_pairs()
    want = [model_mul(x, y) for x, y in zip(a, b)]
    got = lib.gf64_mul(col(a), col(b))
    assert [int(v) for v in got[:, 0]] == want
    assert np.array_equal(got, oracle.gf_mul(col(a), col(b)))
    for x, y, w in zip(a, b, want):
        assert int(lib.gf64_host_mul(elem(x), elem(y))[0]) == w, (hex(x), hex(y))


def check_inverse(lib):
    vals = [v for v in EDGE if v] + [int(v) for v in seeded("inv", 512)[:, 0] if v]
    inv = lib.gf64_inv(col(vals))
    assert np.array_equal(inv, oracle.gf_inv(col(vals)))
    assert [model_mul(v, int(i)) for v, i in zip(vals, inv[:, 0])] == [1] * len(vals)
    assert int(lib.gf64_inv(col([0]))[0, 0]) == 0                 # a^(2^64 - 2), as the gf192 vector entry
    for v in vals[:24]:
        assert model_mul(v, int(lib.gf64_inverse_host(elem(v))[0])) == 1
    with pytest.raises(ValueError, match="inverse of zero"):
        lib.gf64_inverse_host(elem(0))


# ---- 2. / 4. FFT and IFFT ----
def check_fft(lib, max_m=None):
    """max_m: only the domains of dimension <= max_m (for runs that cost more per element); the default takes them all"""
    ran = 0
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        if max_m is not None and m > max_m:
            continue
        for count in coeff_counts(m):
            coeffs = seeded("fft %s %d" % (name, count), count)
            got = lib.additive_FFT_gf64(coeffs, basis, shift)
            assert np.array_equal(got, oracle.additive_fft(coeffs, basis, shift)), (name, count)
            if m <= 8:
                assert np.array_equal(got, oracle.naive_fft(coeffs, basis, shift)), (name, count)
            ran += 1
    assert ran == sum(len(coeff_counts(b.shape[0])) for _, b, _ in fft_domains() if max_m is None or b.shape[0] <= max_m)
    assert ran > 250


def check_ifft(lib):
    ran = 0
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        evals = seeded("ifft %s" % name, 1 << m)
        got = lib.additive_IFFT_gf64(evals, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft(evals, basis, shift)), name
        assert np.array_equal(lib.additive_FFT_gf64(got, basis, shift), evals), name        # FFT o IFFT = id
        coeffs = seeded("roundtrip %s" % name, 1 << m)
        assert np.array_equal(lib.additive_IFFT_gf64(lib.additive_FFT_gf64(coeffs, basis, shift), basis, shift), coeffs), name
        ran += 1
    assert ran == 15 * 3 + 3


def check_ifft_in_place_and_known_degree(lib):
    for m in (0, 5, 11):
        basis, shift = std_basis(m), elem((1 << 63) | 9)
        n = 1 << m
        evals = seeded("in place %d" % m, n)
        d = lib.malloc(8 * n)
        try:
            lib.h2d(d, evals)
            lib.additive_IFFT_gf64_dev(d, basis, shift, d)
            out = np.empty((n, 1), dtype=np.uint64)
            lib.d2h(out, d)
        finally:
            lib.free(d)
        assert np.array_equal(out, oracle.additive_ifft(evals, basis, shift)), m
    basis, shift = derived_domains(77)[0]
    evals = seeded("known degree", 1 << 11)
    for degree in (1, 2, 33, 64, 700, 2048):
        got = lib.IFFT_of_known_degree_gf64(evals, degree, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft_known_degree(evals, degree, basis, shift)), degree


SCHEDULES = [
    # (options, m): which kernels the transform of 2^m coefficients then takes
    ({"IOPX_GF64_TILE_BITS": 12}, 9),                                                               # defaults: one k64_phase1 pass, k64_bfly_edge alone with 8 tiles per workgroup
    ({"IOPX_GF64_TILE_BITS": 4, "IOPX_GF64_P1_COLS": 1, "IOPX_GF64_P2_COLS": 1, "IOPX_GF64_P2_TOP": 1}, 5),    # one chunked phase-1 level, one k64_bfly_upper pass
    ({"IOPX_GF64_TILE_BITS": 4, "IOPX_GF64_P1_COLS": 1, "IOPX_GF64_P2_COLS": 1, "IOPX_GF64_P2_TOP": 1}, 9),    # several chunks per level, two upper passes, strided tiles (h > c)
    ({"IOPX_GF64_TILE_BITS": 5, "IOPX_GF64_P1_COLS": 0, "IOPX_GF64_P2_COLS": 0, "IOPX_GF64_P2_TOP": 0}, 10),   # single-column tiles, no natural-order runs in the last pass
    ({"IOPX_GF64_TILE_BITS": 6, "IOPX_GF64_P1_COLS": 3, "IOPX_GF64_P2_COLS": 4, "IOPX_GF64_P2_TOP": 3}, 11),   # wide columns: c limited by h in the phase-1 chunks
    ({"IOPX_GF64_TILE_BITS": 3, "IOPX_GF64_P1_COLS": 1, "IOPX_GF64_P2_COLS": 1, "IOPX_GF64_P2_TOP": 2}, 7),    # the smallest tile: rows of 2^2, c_top = tile - 1
]


def check_schedules(lib):
    """Each pass kind of the schedule at the smallest m where it applies, reached through the tuning options (looked up when a plan is built):
    IOPX_GF64_TILE_BITS = T bounds every tile; with m <= T the transform is one k64_phase1 pass and k64_bfly_edge alone (2^(T-m) tiles per
    workgroup); with m > T phase 1 takes one k64_phase1 pass per run of T - P1_COLS - 1 network steps of each level j < m - T and a final pass
    for the rest, phase 2 takes k64_bfly_upper passes of T - P2_COLS pair bits down to bit T - P2_TOP and k64_bfly_edge for the low ones.
    Full transforms, the LDE with staged coset groups (n_coeffs = 2^(m-2)) and the IFFT run under each setting."""
    names = ["IOPX_GF64_TILE_BITS", "IOPX_GF64_P1_COLS", "IOPX_GF64_P2_COLS", "IOPX_GF64_P2_TOP"]
    ran = 0
    try:
        for opts, m in SCHEDULES:
            for k in names:
                lib.clear_option(k)
            for k, v in opts.items():
                lib.set_option(k, v)
            lib.clear_plans()
            for basis, shift in ((std_basis(m), elem((1 << 63) | 3)), tuple(derived_domains(5)[0]) if m == 11 else (std_basis(m), elem(0))):
                n = 1 << m
                for count in (n, n - 1, (n >> 2), (n >> 2) + 1):
                    coeffs = seeded("sched %d %d" % (m, count), count)
                    assert np.array_equal(lib.additive_FFT_gf64(coeffs, basis, shift), oracle.additive_fft(coeffs, basis, shift)), (opts, m, count)
                evals = seeded("sched ifft %d" % m, n)
                assert np.array_equal(lib.additive_IFFT_gf64(evals, basis, shift), oracle.additive_ifft(evals, basis, shift)), (opts, m)
                ran += 1
    finally:
        for k in names:
            lib.clear_option(k)
        lib.clear_plans()
    assert ran == 2 * len(SCHEDULES)


# ---- the single access path ----
K64_ARM_ROWS = {"k64_build_ltab", "k64_pow_direct", "k64_pad_copy", "k64_fill", "k64_phase1", "k64_phase1_inv", "k64_bfly_upper",
                "k64_bfly_upper_inv", "k64_bfly_edge", "k64_bfly_edge_inv", "k64_fri_fold", "k64_ldt_combine", "k64_mul", "k64_inv"}


def check_placement_and_profile(lib):
    """2^5 elements under the second geometry of SCHEDULES (three phase-1 launches of which two are the chunks of level 0, one k64_bfly_upper
    pass, k64_bfly_edge), every device buffer at an address 8 mod 16, the profile on: FFT and IFFT as a round trip, the LDE of the same
    coefficients onto cosets [1, 3) of the four of a domain of dimension 7 (the staged group), folds with cosets of 2, 4 (one launch each)
    and 16 (two launches), and an LDT combination of one maximal and two submaximal oracles of one exponent.  Every result equals the
    oracle's; a one-word element has one access path, so every k64_ row of the profile is one of the arm's plain names and none ends
    in _w64 wherever the buffers lie."""
    names = ["IOPX_GF64_TILE_BITS", "IOPX_GF64_P1_COLS", "IOPX_GF64_P2_COLS", "IOPX_GF64_P2_TOP"]
    m, big = 5, 7
    n = 1 << m
    basis, shift, x = std_basis(big), elem((1 << 63) | 0x51), elem(int(seeded("place x", 1)[0, 0]))
    b5 = basis[:m]
    coeffs = seeded("place coeffs", n)
    evals = [seeded("place evals %d" % k, n) for k in range(3)]
    degrees, coef = [n, n - 3, n - 3], seeded("place coef", 6)
    raw = [lib.malloc(8 * (2 << m) + 16) for _ in range(4)]
    at = [p + (8 - p) % 16 for p in raw]
    assert all(p % 16 == 8 for p in at)

    def read(p, count):
        out = np.empty((count, 1), dtype=np.uint64)
        lib.d2h(out, p)
        return out

    try:
        for k, v in zip(names, (4, 1, 1, 1)):
            lib.set_option(k, v)
        lib.clear_plans()
        lib.profile_begin()
        lib.h2d(at[0], coeffs)
        lib.additive_FFT_gf64_dev(at[0], n, b5, shift, at[3])
        assert np.array_equal(read(at[3], n), oracle.additive_fft(coeffs, b5, shift))
        lib.additive_IFFT_gf64_dev(at[3], b5, shift, at[1])
        assert np.array_equal(read(at[1], n), coeffs)
        lib.additive_LDE_gf64_dev(at[0], n, basis, shift, 1, 2, at[3])
        assert np.array_equal(read(at[3], 2 << m), oracle.additive_fft(coeffs, basis, shift)[1 << m:3 << m])
        lib.h2d(at[0], evals[0])
        for coset in (2, 4, 16):
            lib.evaluate_next_f_i_over_entire_domain_gf64_dev(at[0], b5, shift, coset, x, at[3])
            assert np.array_equal(read(at[3], n // coset), oracle.fri_fold_additive(evals[0], b5, shift, coset, x)), coset
        for p, e in zip(at, evals):
            lib.h2d(p, e)
        lib.ldt_combine_gf64_dev(at[:3], degrees, coef, b5, shift, at[3])
        assert np.array_equal(read(at[3], n), oracle.ldt_combine_additive(evals, degrees, coef, b5, shift))
        report = lib.profile_report()
    finally:
        for k in names:
            lib.clear_option(k)
        lib.clear_plans()
        for p in raw:
            lib.free(p)
    rows = {k: v[0] for k, v in report.items() if k.startswith("k64_")}
    assert set(rows) <= K64_ARM_ROWS, sorted(set(rows) - K64_ARM_ROWS)
    assert not [k for k in report if k.endswith("_w64")], sorted(report)
    # FFT + LDE forward, one IFFT; the LDE's upper pass and last pass take its two cosets in one launch
    want = {"k64_pad_copy": 2, "k64_phase1": 6, "k64_bfly_upper": 2, "k64_bfly_edge": 2, "k64_bfly_edge_inv": 1, "k64_bfly_upper_inv": 1,
            "k64_phase1_inv": 3, "k64_fri_fold": 4, "k64_ldt_combine": 1}
    assert {k: rows.get(k, 0) for k in want} == want, rows


# ---- 3. LDE coset ranges ----
def check_lde_ranges(lib):
    m, d = 12, 7
    basis, shift = std_basis(m), elem((1 << 63) | 0x55)
    coeffs = seeded("lde", (1 << d) - 3)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(8 << d), lib.malloc(8 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 1), (5, 3), (31, 1), (0, 32)):
            lib.additive_LDE_gf64_dev(dc, coeffs.shape[0], basis, shift, begin, count, do)
            out = np.empty((count << d, 1), dtype=np.uint64)
            lib.d2h(out, do)
            assert np.array_equal(out, full[begin << d:(begin + count) << d]), (begin, count)
        for begin, count in ((32, 1), (31, 2), (0, 0), (0, 33)):
            with pytest.raises(ValueError, match="outside the 32 cosets"):
                lib.additive_LDE_gf64_dev(dc, coeffs.shape[0], basis, shift, begin, count, do)
    finally:
        lib.free(dc)
        lib.free(do)


def check_lde_upper_pass_whole(lib):
    """2^13 coefficients, the smallest count whose plan has a k64_bfly_upper pass with the default tile, onto m = 15: every coset range of the four
    against the oracle's transform, whole; the ranges of more than one coset go through the block-order staging (one group)"""
    m, d = 15, 13
    basis, shift = std_basis(m), elem((1 << 63) | 0x55)
    coeffs = seeded("lde upper", 1 << d)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(8 << d), lib.malloc(8 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 4), (1, 3), (3, 1)):
            lib.profile_begin()
            lib.additive_LDE_gf64_dev(dc, coeffs.shape[0], basis, shift, begin, count, do)
            assert lib.profile_report().get("k64_bfly_upper", (0,))[0] >= 1, "the plan has no upper pass"
            out = np.empty((count << d, 1), dtype=np.uint64)
            lib.d2h(out, do)
            assert np.array_equal(out, full[begin << d:(begin + count) << d]), (begin, count)
    finally:
        lib.free(dc)
        lib.free(do)


# ---- 5. fold ----
def fold_domains():
    return [("std", std_basis(10), elem((1 << 63) | 0x77))] + [("derived %d" % i, b, s) for i, (b, s) in enumerate(derived_domains(0x1234))]


def check_fold(lib):
    x = elem(int(seeded("fold x", 1)[0, 0]))
    ran = 0
    for name, basis, shift in fold_domains():
        m = basis.shape[0]
        f = seeded("fold %s" % name, 1 << m)
        for eta in list(range(0, 6)) + [m]:
            got = lib.evaluate_next_f_i_over_entire_domain_gf64(f, basis, shift, 1 << eta, x)
            assert np.array_equal(got, oracle.fri_fold_additive(f, basis, shift, 1 << eta, x)), (name, eta)
            if eta == 0:
                assert np.array_equal(got, f)
            if eta == m:        # the interpolant of f on the whole domain, at x
                coeffs = oracle.additive_ifft(f, basis, shift)
                assert np.array_equal(got, oracle.poly_eval(coeffs, x).reshape(1, 1)), name
            ran += 1
    assert ran == 4 * 7
    # x on the domain: the fold returns f there (fri_aux.tcc:77-86)
    basis, shift = std_basis(6), elem(1 << 20)
    f = seeded("fold on domain", 64)
    xs = oracle.all_subset_sums(basis, shift)[13]
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf64(f, basis, shift, 4, xs), oracle.fri_fold_additive(f, basis, shift, 4, xs))
    dep = std_basis(6).copy()
    dep[1] = dep[0]
    with pytest.raises(ValueError, match="linearly dependent"):
        lib.evaluate_next_f_i_over_entire_domain_gf64(f, dep, shift, 4, x)


def check_fold_chain(lib):
    """[2, 2, 1] on an LDE of 2^6 coefficients onto m = 11: every folded codeword stays below its degree bound"""
    m, basis, shift = 11, std_basis(11), elem((1 << 63) | 1)
    f = lib.additive_FFT_gf64(seeded("chain", 1 << 6), basis, shift)
    domains = lib.fri_additive_domains_gf64(basis, shift, [2, 2, 1])
    bound = 1 << 6
    for i, eta in enumerate([2, 2, 1]):
        b, s = domains[i]
        f = lib.evaluate_next_f_i_over_entire_domain_gf64(f, b, s, 1 << eta, elem(int(seeded("chain x %d" % i, 1)[0, 0])))
        bound >>= eta
        nb, ns = domains[i + 1]
        coeffs = lib.additive_IFFT_gf64(f, nb, ns)
        assert coeffs[:bound].any() and not coeffs[bound:].any(), i


# ---- 6. domain chain ----
def check_domain_chain(lib):
    basis, shift = std_basis(12), elem((1 << 63) | 0xABC)
    for loc in ([1, 2, 2], [3, 1]):
        got = lib.fri_additive_domains_gf64(basis, shift, loc)
        want = oracle.fri_domains_additive(basis, shift, loc)
        assert len(got) == len(loc) + 1
        for (gb, gs), (wb, ws) in zip(got[1:], want):
            assert np.array_equal(gb, wb) and np.array_equal(gs.reshape(-1), ws.reshape(-1)), loc
    with pytest.raises(ValueError, match="exceed the domain dimension"):
        lib.fri_additive_domains_gf64(std_basis(3), shift, [2, 2])


# ---- 7. LDT combination ----
LDT_CASES = [
    ("one maximal", [2048]),
    ("seven mixed", [2048, 2047, 2047, 1024, 2046, 2048, 1025]),
    ("bump not a power of two", [1000, 233, 1000 - 7]),
]


def check_ldt(lib):
    m = 11
    for basis, shift in ((std_basis(m), elem((1 << 63) | 0xF0F)), tuple(derived_domains(3)[0])):
        for name, degrees in LDT_CASES:
            evals = [seeded("ldt %s %d" % (name, k), 1 << m) for k in range(len(degrees))]
            coef = seeded("ldt coef " + name, 2 * len(degrees))
            got = lib.ldt_combine_gf64(evals, degrees, coef, basis, shift)
            assert np.array_equal(got, oracle.ldt_combine_additive(evals, degrees, coef, basis, shift)), name


# ---- 8. pins of the generic paths on 8-byte elements (these pass without the gf64 kernels) ----
def check_merkle_and_queries(lib):
    for num_oracles in (1, 5):
        oracles = [seeded("merkle %d %d" % (num_oracles, k), 64) for k in range(num_oracles)]
        for coset in (1, 2, 4, 8):
            assert np.array_equal(lib.merkle_tree(oracles, coset), oracle.merkle_build(oracles, coset)), (num_oracles, coset)
        ptrs = [lib.malloc(8 * 64) for _ in oracles]
        try:
            for p, o in zip(ptrs, oracles):
                lib.h2d(p, o)
            positions = [0, 63, 17, 17, 32]
            got = np.asarray(lib.query_responses_dev(ptrs, 8, 64, positions)).reshape(len(positions), num_oracles)
            assert np.array_equal(got, np.array([[int(o[p, 0]) for o in oracles] for p in positions], dtype=np.uint64))
        finally:
            for p in ptrs:
                lib.free(p)


# ---- 9. host and device forms, argument checks ----
def check_host_and_device_forms(lib):
    m, basis, shift = 9, std_basis(9), elem(1 << 40)
    n = 1 << m
    coeffs, x = seeded("forms", n - 5), elem(0xDEADBEEF12345)
    d_in, d_out = lib.malloc(8 * n), lib.malloc(8 * n)
    try:
        lib.h2d(d_in, coeffs)
        lib.additive_FFT_gf64_dev(d_in, coeffs.shape[0], basis, shift, d_out)
        evals = np.empty((n, 1), dtype=np.uint64)
        lib.d2h(evals, d_out)
        assert np.array_equal(evals, lib.additive_FFT_gf64(coeffs, basis, shift))
        lib.additive_IFFT_gf64_dev(d_out, basis, shift, d_in)
        back = np.empty((n, 1), dtype=np.uint64)
        lib.d2h(back, d_in)
        assert np.array_equal(back, lib.additive_IFFT_gf64(evals, basis, shift))
        lib.evaluate_next_f_i_over_entire_domain_gf64_dev(d_out, basis, shift, 8, x, d_in)
        folded = np.empty((n // 8, 1), dtype=np.uint64)
        lib.d2h(folded, d_in)
        assert np.array_equal(folded, lib.evaluate_next_f_i_over_entire_domain_gf64(evals, basis, shift, 8, x))
    finally:
        lib.free(d_in)
        lib.free(d_out)


def check_argument_checks(lib):
    """each refusal carries the gf192 twin's message"""
    c = lib.c
    basis, shift, x = std_basis(4), elem(0), elem(7)
    bp, sp, xp = basis.ctypes.data_as(U64P), shift.ctypes.data_as(U64P), x.ctypes.data_as(U64P)
    f = seeded("checks", 16)
    fp = f.ctypes.data_as(U64P)
    big = std_basis(41)
    calls = [
        ("null basis/shift", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 0, None, 4, sp, None)),
        ("null buffer", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 3, bp, 4, sp, None)),
        ("null buffer", lambda g: getattr(c, "iopx_add_ifft_%s_dev" % g)(None, bp, 4, sp, None)),
        ("null basis/shift", lambda g: getattr(c, "iopx_add_ifft_%s" % g)(fp, bp, 4, None, fp)),
        ("exceed the domain size", lambda g: getattr(c, "iopx_add_fft_%s" % g)(fp, 17, bp, 4, sp, fp)),
        ("too large", lambda g: getattr(c, "iopx_add_fft_%s_dev" % g)(None, 0, big.ctypes.data_as(U64P), 41, sp, None)),
        ("too large", lambda g: getattr(c, "iopx_add_ifft_%s_dev" % g)(None, big.ctypes.data_as(U64P), 41, sp, None)),
        ("too large", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(None, big.ctypes.data_as(U64P), 41, sp, 2, xp, None)),
        ("null argument", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(None, bp, 4, sp, 2, xp, None)),
        ("not a power of two", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(ctypes.c_void_p(8), bp, 4, sp, 3, xp, ctypes.c_void_p(8))),
        ("exceeds the domain size", lambda g: getattr(c, "iopx_fri_fold_add_%s_dev" % g)(ctypes.c_void_p(8), bp, 4, sp, 32, xp, ctypes.c_void_p(8))),
        ("null argument", lambda g: getattr(c, "iopx_fri_domains_%s" % g)(None, 4, sp, None, 0, None, None)),
        ("null argument", lambda g: getattr(c, "iopx_ldt_combine_%s_dev" % g)(None, 1, None, None, bp, 4, sp, None)),
        ("null argument", lambda g: getattr(c, "iopx_%s_host_mul" % g)(None, None, None)),
        ("null argument", lambda g: getattr(c, "iopx_%s_inverse_host" % g)(None, None)),
    ]
    for text, call in calls:
        msgs = []
        for g in ("gf192", "gf64"):
            with pytest.raises(ValueError, match=text) as e:
                lib._check(call(g))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf64(f, basis, shift, 3, x)
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf64(f, basis, shift, 32, x)
    dep = std_basis(4).copy()
    dep[2] = dep[0] ^ dep[1]
    with pytest.raises(ValueError, match="additive FFT: basis vectors are linearly dependent"):
        lib.additive_FFT_gf64(f, dep, shift)
    # the size-zero and size-one edge cases are accepted as the twin accepts them
    assert np.array_equal(lib.additive_FFT_gf64(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_IFFT_gf64(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_FFT_gf64(f[:0], basis, shift), np.zeros((16, 1), dtype=np.uint64))
    assert np.array_equal(lib.additive_FFT_gf64(f[:1], basis, shift), np.repeat(f[:1], 16, axis=0))
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf64(f, basis, shift, 1, x), f)


# ---- 11. FRI-only SNARK ----
FRI_SNARK_TUPLES = [((8, 2, 2, 1, 6), 2272), ((10, 2, 1, 1, 4), 3648), ((12, 3, 3, 2, 8), 6088)]      # (dim, rs_extra, loc, interactions, queries), bytes


def check_fri_snark(lib, torch, device):
    """fri.fri_snark_prover over domains.GF64 against the oracle's prover, byte for byte, and accepted by the oracle's verifier"""
    from libiop_amd import domains, fri, r1cs
    ops = domains.DeviceOps(lib, torch, device, domains.GF64())
    assert type(ops) is domains.GF64DeviceOps
    for (dim, rs_extra, loc, interactions, queries), size in FRI_SNARK_TUPLES:
        params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
        coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (dim - rs_extra))
        mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=ops.upload(coeffs)).serialize()
        ref = oracle.fri_snark_prove(oracle.FIELD_GF64, dim, rs_extra, loc, interactions, queries, 5)
        assert len(ref) == size
        assert mine == ref, (dim, next((i for i, (a, b) in enumerate(zip(mine, ref)) if a != b), min(len(mine), len(ref))), len(mine), len(ref))
        assert oracle.fri_snark_verify(oracle.FIELD_GF64, dim, rs_extra, loc, interactions, queries, mine)
    with pytest.raises(NotImplementedError, match="gf64"):
        ops.rowcheck(None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="gf64"):
        ops.mul(None, None)


def check_fri_snark_other_fields_unchanged(lib, torch, device):
    """the same function over GF192 and EdwardsFr still produces its old bytes"""
    from libiop_amd import domains, fri, r1cs
    dim, rs_extra, loc, interactions, queries = 8, 2, 2, 1, 6
    for code, cls in ((oracle.FIELD_GF192, domains.GF192), (oracle.FIELD_EDWARDS, domains.EdwardsFr)):
        ops = domains.DeviceOps(lib, torch, device, cls())
        assert type(ops) is domains.DeviceOps
        params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
        coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (dim - rs_extra))
        mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=ops.upload(coeffs)).serialize()
        assert mine == oracle.fri_snark_prove(code, dim, rs_extra, loc, interactions, queries, 5), cls.__name__
