"""Cases for the GF(2^256) arm (libiop_amd/csrc/gf256.hip): product and inverse, additive FFT / IFFT / LDE, FRI fold and domain chain,
LDT combination, the 64-bit and 128-bit access paths, the generic Merkle / query-response path on 32-byte binary elements, the refusals and
the dispatch between the two four-word fields.  Shared by tests/test_gf256_emu.py (CPU emulation), tests/test_gpu_gf256.py (MI355X),
tests/test_gf256_memory.py and tests/test_gf256_binding.py: every function takes the Library under test.  Expected values come from `oracle`
at four words at run time, except the product, which is also checked against the shift-and-xor model below.  The cases mirror
tests/gf128_cases.py at four words per element, with every dimension at or below the default tile bits + 2.

Elements are (n, 4) uint64 arrays: libff gf256's layout, four little-endian words, x^256 + x^10 + x^5 + x^2 + 1."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import oracle

W = 4
MASK64 = (1 << 64) - 1
MASK = (1 << 256) - 1
TAIL = 0x425                                    # x^10 + x^5 + x^2 + 1
TOP = 1 << 255
# 0, 1, the reduction polynomial's tail, x^255, all ones, and bits on each side of the word boundaries 63/64, 127/128 and 191/192
EDGE = [0, 1, TAIL, 3, 1 << 63, 1 << 64, (1 << 63) | (1 << 64), 1 << 127, 1 << 128, (1 << 127) | (1 << 128), 1 << 191, 1 << 192,
        (1 << 191) | (1 << 192), TOP, TOP + 1, MASK]
# x^255 * x^(247 + j) = x^(502 + j): bit 246 + j of the product's upper half H, j = 0 .. 8.  These are the bits that H x^10 pushes past bit 255
# (the second fold); the tenth, bit 255 of H, is never set: a product of two 256-bit polynomials has degree at most 510.
TOP_PAIRS = [(TOP, 1 << (247 + j)) for j in range(9)] + [(MASK, MASK), (TOP | (1 << 254), MASK)]
U64P = ctypes.POINTER(ctypes.c_uint64)
NAMES = ["IOPX_GF256_TILE_BITS", "IOPX_GF256_P1_COLS", "IOPX_GF256_P2_COLS", "IOPX_GF256_P2_TOP"]
TILE_BITS = 10                                   # the default IOPX_GF256_TILE_BITS (the largest is 11)
P1_COLS, P2_COLS, P2_TOP = 2, 3, 2               # the other defaults


def model_mul(a, b):
    """shift-and-xor product modulo x^256 + x^10 + x^5 + x^2 + 1, Python integers only"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 256:
            a ^= (1 << 256) | TAIL
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


def reduce_model(c):
    """a 511-bit carry-less product reduced by 0x425, bit by bit from the top"""
    for i in range(c.bit_length() - 1, 255, -1):
        if (c >> i) & 1:
            c ^= ((1 << 256) | TAIL) << (i - 256)
    return c


def seeded(tag, count):
    seed = int.from_bytes(hashlib.sha256(b"gf256 " + tag.encode()).digest()[:8], "little")
    return np.random.default_rng(seed).integers(0, MASK64, size=(count, W), dtype=np.uint64, endpoint=True)


def ints(a):
    return [sum(int(r[k]) << (64 * k) for k in range(W)) for r in np.asarray(a, dtype=np.uint64).reshape(-1, W)]


def col(values):
    return np.array([[(v >> (64 * k)) & MASK64 for k in range(W)] for v in values], dtype=np.uint64).reshape(-1, W)


def elem(v):
    return np.array([(v >> (64 * k)) & MASK64 for k in range(W)], dtype=np.uint64)


def std_basis(m):
    return oracle.standard_basis(m, W)


def high_basis(m):
    """m vectors spread over the four words, one of them x^255 (for m >= 2), none of them a standard basis vector's neighbour"""
    return col([1 << (255 - (i * 255) // max(m - 1, 1)) if m > 1 else 1 << 200 for i in range(m)])


def fft_shifts(m):
    return [("0", 0), ("1<<m", 1 << m), ("bit255", TOP | (0xABCDEF << 192) | (0x55 << 128) | (7 << 64) | 0x1234567)]


@functools.lru_cache(maxsize=None)
def _derived(shift):
    return oracle.fri_domains_additive(std_basis(12), elem(shift), [1, 2, 3])


def derived_domains(shift):
    """the derived domains of fri_domains_additive(standard_basis(12), shift, [1, 2, 3]): non-standard bases of dimension 11, 9, 6"""
    return _derived(shift)


def fft_domains():
    """(name, basis, shift) of every FFT / IFFT case: every m from 0 to the default tile bits + 1 on the standard basis with shifts that
    reach bit 255, the derived bases, and bases with vectors in every word"""
    out = []
    for m in range(0, TILE_BITS + 2):
        for sname, s in fft_shifts(m):
            out.append(("std m=%d shift=%s" % (m, sname), std_basis(m), elem(s)))
    for i, (b, s) in enumerate(derived_domains(TOP | (7 << 64) | 5)):
        out.append(("derived %d" % i, b, s))
    for m in (2, 7, 11):
        out.append(("high m=%d" % m, high_basis(m), elem(TOP | (3 << 100) | 0x99)))
    return out


def coeff_counts(m):
    n = 1 << m
    return sorted({c for c in (0, 1, n // 2 + 1, n) if 0 <= c <= n})


# ---- 1. product and inverse ----
def mul_pairs():
    a = [x for x in EDGE for _ in EDGE] + [x for x, _ in TOP_PAIRS] + ints(seeded("mul a", 1024))
    b = [y for _ in EDGE for y in EDGE] + [y for _, y in TOP_PAIRS] + ints(seeded("mul b", 1024))
    return a, b


def check_product(lib):
    a, b = mul_pairs()
    fixed = len(EDGE) ** 2 + len(TOP_PAIRS)
    for j in range(9):
        assert clmul(*TOP_PAIRS[j]) == 1 << (502 + j)
    assert clmul(MASK, MASK).bit_length() == 511             # bit 511 (bit 255 of H) is out of reach
    assert model_mul(TOP, 2) == TAIL
    want = [model_mul(x, y) for x, y in zip(a, b)]
    assert want[:fixed] == [reduce_model(clmul(x, y)) for x, y in zip(a[:fixed], b)]
    got = lib.gf256_mul(col(a), col(b))
    assert ints(got) == want
    assert np.array_equal(got, oracle.gf_mul(col(a), col(b)))
    assert ints(oracle.gf_mul(col([TOP]), col([2]))) == [TAIL]
    for x, y, w in list(zip(a, b, want))[:fixed + 32]:
        assert ints(lib.gf256_host_mul(elem(x), elem(y))) == [w], (hex(x), hex(y))
    for count in (1, 63, 64, 65, 1000):
        assert ints(lib.gf256_mul(col(a[:count]), col(b[:count]))) == want[:count], count
    # squaring through a * a, on the device and through the host twin
    sq = EDGE + ints(seeded("square", 128))
    want_sq = [model_mul(x, x) for x in sq]
    assert ints(lib.gf256_mul(col(sq), col(sq))) == want_sq
    for x, w in zip(sq[:len(EDGE) + 8], want_sq):
        assert ints(lib.gf256_host_mul(elem(x), elem(x))) == [w], hex(x)


def check_inverse(lib):
    vals = [v for v in EDGE if v] + [v for v in ints(seeded("inv", 128)) if v]
    inv = lib.gf256_inv(col(vals))
    assert np.array_equal(inv, oracle.gf_inv(col(vals)))
    assert [model_mul(v, i) for v, i in zip(vals, ints(inv))] == [1] * len(vals)
    assert ints(lib.gf256_inv(col([0]))) == [0]                  # a^(2^256 - 2), as the gf192 vector entry
    for count in (1, 63, 64, 65):
        assert np.array_equal(lib.gf256_inv(col(vals[:count])), inv[:count]), count
    for v in vals[:24]:
        assert model_mul(v, ints(lib.gf256_inverse_host(elem(v)))[0]) == 1
    with pytest.raises(ValueError, match="inverse of zero"):
        lib.gf256_inverse_host(elem(0))


# ---- 2. / 4. FFT and IFFT ----
def check_fft(lib, max_m=None):
    """max_m: only the domains of dimension <= max_m (for runs that cost more per element); the default takes them all"""
    ran = 0
    assert any(int(b[:, 3].max(initial=0)) for _, b, _ in fft_domains()) and any(int(s[3]) >> 63 for _, _, s in fft_domains())
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        if max_m is not None and m > max_m:
            continue
        for count in coeff_counts(m):
            coeffs = seeded("fft %s %d" % (name, count), count)
            got = lib.additive_FFT_gf256(coeffs, basis, shift)
            assert np.array_equal(got, oracle.additive_fft(coeffs, basis, shift)), (name, count)
            if m <= 6:
                assert np.array_equal(got, oracle.naive_fft(coeffs, basis, shift)), (name, count)
            ran += 1
    assert ran == sum(len(coeff_counts(b.shape[0])) for _, b, _ in fft_domains() if max_m is None or b.shape[0] <= max_m)
    assert max_m is not None or ran > 150


def check_ifft(lib):
    ran = 0
    for name, basis, shift in fft_domains():
        m = basis.shape[0]
        evals = seeded("ifft %s" % name, 1 << m)
        got = lib.additive_IFFT_gf256(evals, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft(evals, basis, shift)), name
        assert np.array_equal(lib.additive_FFT_gf256(got, basis, shift), evals), name       # FFT o IFFT = id
        ran += 1
    assert ran == (TILE_BITS + 2) * 3 + 3 + 3


def check_ifft_in_place_and_known_degree(lib):
    for m in (0, 5, TILE_BITS + 1):
        basis, shift = std_basis(m), elem(TOP | 9)
        n = 1 << m
        evals = seeded("in place %d" % m, n)
        d = lib.malloc(32 * n)
        try:
            lib.h2d(d, evals)
            lib.additive_IFFT_dev(d, basis, shift, d, words=4)
            out = np.empty((n, W), dtype=np.uint64)
            lib.d2h(out, d)
        finally:
            lib.free(d)
        assert np.array_equal(out, oracle.additive_ifft(evals, basis, shift)), m
    basis, shift = derived_domains((5 << 64) | 77)[0]
    evals = seeded("known degree", 1 << 11)
    for degree in (1, 2, 33, 64, 700, 2048):
        got = lib.IFFT_of_known_degree_gf256(evals, degree, basis, shift)
        assert np.array_equal(got, oracle.additive_ifft_known_degree(evals, degree, basis, shift)), degree


def schedule_model(d, T, p1_cols, p2_cols, p2_top):
    """the pass structure of a plan of dimension d (DESIGN §5.11's schedule): (phase-1 passes as (c, h, A), upper passes as (c, h, A),
    whether the last pass stands alone)"""
    p1, cp = [], min(p1_cols, T - 2)
    for j in range(d):
        if d - j <= T:
            p1.append((min(T - (d - j), j), j, d - j))
            break
        top = d - 1
        while True:
            h = max(j, top + 1 - (T - cp))
            p1.append((min(cp, h), h, top + 1 - h))
            if h == j:
                break
            top = h
    if d <= T:
        return p1, [], True
    c_top = min(p2_top, T - 1)
    a_low = T - c_top
    c = min(p2_cols, a_low)
    upper, top = [], d - 1
    while top >= a_low:
        h = max(a_low, top + 1 - (T - c))
        upper.append((c, h, top + 1 - h))
        top = h - 1
    return p1, upper, False


# gf128_cases.SCHEDULES at this field's default tile: (options, m, what the row is there for: a predicate on the modelled passes)
SCHEDULES = [
    ({"IOPX_GF256_TILE_BITS": 10}, 8, "defaults: one phase-1 pass, the last pass alone with 4 tiles per workgroup",
     lambda p1, up: len(p1) == 1 and not up),
    ({"IOPX_GF256_TILE_BITS": 4, "IOPX_GF256_P1_COLS": 1, "IOPX_GF256_P2_COLS": 1, "IOPX_GF256_P2_TOP": 1}, 5, "one chunked phase-1 level, one upper pass",
     lambda p1, up: len(p1) > 1 and len(up) == 1),
    ({"IOPX_GF256_TILE_BITS": 4, "IOPX_GF256_P1_COLS": 1, "IOPX_GF256_P2_COLS": 1, "IOPX_GF256_P2_TOP": 1}, 9, "several chunks per level, two upper passes, strided tiles (h > c)",
     lambda p1, up: len(up) == 2 and any(h > c for c, h, _ in up) and sum(1 for _, h, _ in p1 if h == 0) >= 1 and len(p1) > 9),
    ({"IOPX_GF256_TILE_BITS": 5, "IOPX_GF256_P1_COLS": 0, "IOPX_GF256_P2_COLS": 0, "IOPX_GF256_P2_TOP": 0}, 10, "single-column tiles, no natural-order runs in the last pass",
     lambda p1, up: all(c == 0 for c, _, _ in up) and len(up) == 1),
    ({"IOPX_GF256_TILE_BITS": 6, "IOPX_GF256_P1_COLS": 3, "IOPX_GF256_P2_COLS": 4, "IOPX_GF256_P2_TOP": 3}, 11, "wide columns: c limited by h in the phase-1 chunks",
     lambda p1, up: any(c < 3 and A < 6 for c, _, A in p1) and any(c == 3 for c, _, _ in p1)),
    ({"IOPX_GF256_TILE_BITS": 3, "IOPX_GF256_P1_COLS": 1, "IOPX_GF256_P2_COLS": 1, "IOPX_GF256_P2_TOP": 2}, 7, "the smallest tile: rows of 2^2, c_top = tile - 1",
     lambda p1, up: len(up) >= 2),
]


def _launches(report, name):
    return report.get(name, (0,))[0]


def check_schedules(lib):
    """Each pass kind of the schedule at the smallest m where it applies, reached through the tuning options (looked up when a plan is built):
    full transforms, the LDE with staged coset groups (n_coeffs = 2^(m-2)) and the IFFT under each setting against the oracle, and the
    profile of one full-size transform against the modelled pass structure — the intended kernels ran, as often as the schedule says."""
    ran = 0
    try:
        for opts, m, why, intended in SCHEDULES:
            for k in NAMES:
                lib.clear_option(k)
            for k, v in opts.items():
                lib.set_option(k, v)
            lib.clear_plans()
            p1, upper, alone = schedule_model(m, opts["IOPX_GF256_TILE_BITS"], opts.get("IOPX_GF256_P1_COLS", P1_COLS), opts.get("IOPX_GF256_P2_COLS", P2_COLS),
                                              opts.get("IOPX_GF256_P2_TOP", P2_TOP))
            assert intended(p1, upper), (why, p1, upper)
            for basis, shift in ((std_basis(m), elem(TOP | 3)), tuple(derived_domains(5 << 64)[0]) if m == 11 else (high_basis(m), elem(1 << 70))):
                n = 1 << m
                for count in (n, n - 1, (n >> 2), (n >> 2) + 1):
                    coeffs = seeded("sched %d %d" % (m, count), count)
                    if count == n:
                        lib.profile_begin()
                    got = lib.additive_FFT_gf256(coeffs, basis, shift)
                    if count == n:
                        rep = lib.profile_report()
                        assert _launches(rep, "k256_phase1") == len(p1), (why, rep)
                        assert _launches(rep, "k256_bfly_upper") == len(upper), (why, rep)
                        assert _launches(rep, "k256_bfly_edge") == 1 and _launches(rep, "k256_pad_copy") == 1, (why, rep)
                        assert not any(k.endswith("_w64") or k.startswith("k128_") for k in rep), rep
                    assert np.array_equal(got, oracle.additive_fft(coeffs, basis, shift)), (opts, m, count)
                evals = seeded("sched ifft %d" % m, n)
                lib.profile_begin()
                got = lib.additive_IFFT_gf256(evals, basis, shift)
                rep = lib.profile_report()
                assert _launches(rep, "k256_phase1_inv") == len(p1) and _launches(rep, "k256_bfly_upper_inv") == len(upper) and _launches(rep, "k256_bfly_edge_inv") == 1, (why, rep)
                assert np.array_equal(got, oracle.additive_ifft(evals, basis, shift)), (opts, m)
                ran += 1
    finally:
        for k in NAMES:
            lib.clear_option(k)
        lib.clear_plans()
    assert ran == 2 * len(SCHEDULES)


# ---- 3. LDE coset ranges ----
def _lde(lib, dc, n_coeffs, basis, shift, begin, count, do, d):
    lib.additive_LDE_dev(dc, n_coeffs, basis, shift, begin, count, do, words=4)
    out = np.empty((count << d, W), dtype=np.uint64)
    lib.d2h(out, do)
    return out


def check_lde_ranges(lib):
    m, d = 12, 7
    basis, shift = std_basis(m), elem(TOP | 0x55)
    coeffs = seeded("lde", (1 << d) - 3)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(32 << d), lib.malloc(32 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 1), (5, 3), (31, 1), (0, 32)):
            assert np.array_equal(_lde(lib, dc, coeffs.shape[0], basis, shift, begin, count, do, d), full[begin << d:(begin + count) << d]), (begin, count)
        for begin, count in ((32, 1), (31, 2), (0, 0), (0, 33)):
            with pytest.raises(ValueError, match="outside the 32 cosets"):
                lib.additive_LDE_dev(dc, coeffs.shape[0], basis, shift, begin, count, do, words=4)
    finally:
        lib.free(dc)
        lib.free(do)


def check_lde_upper_pass_whole(lib):
    """2^(T+1) coefficients, the smallest count whose plan has a k256_bfly_upper pass with the default tile T, onto m = T + 2: every coset range
    against the oracle's transform, whole; the range of two cosets goes through the block-order staging, the single ones run direct"""
    d = TILE_BITS + 1
    m = d + 1
    basis, shift = std_basis(m), elem(TOP | 0x55)
    coeffs = seeded("lde upper", 1 << d)
    full = oracle.additive_fft(coeffs, basis, shift)
    dc, do = lib.malloc(32 << d), lib.malloc(32 << m)
    try:
        lib.h2d(dc, coeffs)
        for begin, count in ((0, 2), (0, 1), (1, 1)):
            lib.profile_begin()
            out = _lde(lib, dc, coeffs.shape[0], basis, shift, begin, count, do, d)
            assert lib.profile_report().get("k256_bfly_upper", (0,))[0] >= 1, "the plan has no upper pass"
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
    a device address 8 mod 16: on the aligned call the profile shows 128-bit instantiations only; on the other two the kernel that touches
    the misaligned buffer (k256_pad_copy for a transform's input, k256_bfly_edge for its output, the fold and the combination themselves) ran
    as its 64-bit instantiation and only as that, while passes between aligned temporaries keep the 128-bit one.  All equal the oracle."""
    m, d = 9, 7
    n = 1 << m
    basis, shift, x = std_basis(m), elem(TOP | 0x31), elem((9 << 192) | 4)
    coeffs = seeded("align coeffs", n)
    evals = [seeded("align evals %d" % k, n) for k in range(3)]
    degrees, coef = [n, n - 3, n // 2], seeded("align coef", 6)
    want = {
        "fft": oracle.additive_fft(coeffs, basis, shift),
        "lde": oracle.additive_fft(coeffs[:1 << d], basis, shift)[2 << d:4 << d],
        "fold": oracle.fri_fold_additive(evals[0], basis, shift, 4, x),
        "ldt": oracle.ldt_combine_additive(evals, degrees, coef, basis, shift),
    }
    raw = [lib.malloc(32 * n + 16) for _ in range(4)]            # three inputs, one output
    try:
        assert all(p % 16 == 0 for p in raw), "the allocator is expected to hand out 16-byte aligned blocks"
        for off_in, off_out in ((0, 0), (8, 0), (0, 8)):
            ins, out = [p + off_in for p in raw[:3]], raw[3] + off_out
            calls = {
                "fft": (coeffs, "k256_pad_copy" if off_in else "k256_bfly_edge", lambda: lib.additive_FFT_dev(ins[0], n, basis, shift, out, words=4), n),
                "lde": (coeffs, "k256_pad_copy" if off_in else "k256_bfly_edge", lambda: lib.additive_LDE_dev(ins[0], 1 << d, basis, shift, 2, 2, out, words=4), 2 << d),
                "fold": (evals[0], "k256_fri_fold", lambda: lib.fri_fold_dev(ins[0], basis, shift, 4, x, out, words=4), n // 4),
                "ldt": (None, "k256_ldt_combine", lambda: lib.ldt_combine_dev(ins, degrees, coef, basis, shift, out, words=4), n),
            }
            for name, (src, stem, call, n_out) in calls.items():
                if src is None:
                    for p, e in zip(ins, evals):
                        lib.h2d(p, e)
                else:
                    lib.h2d(ins[0], src)
                lib.profile_begin()
                call()
                got = np.empty((n_out, W), dtype=np.uint64)
                lib.d2h(got, out)
                report = lib.profile_report()
                wide, narrow = _ran(report, stem)
                assert np.array_equal(got, want[name]), (name, off_in, off_out)
                if off_in == 0 and off_out == 0:
                    assert wide >= 1 and _ran(report, "k256_")[1] == 0, (name, report)
                else:
                    assert narrow >= 1 and wide == 0, (name, off_in, off_out, wide, narrow)
                    # only the kernels that touch the misaligned buffer took the 64-bit path
                    assert all(k.startswith(stem) for k in report if k.endswith("_w64")), (name, report)
    finally:
        for p in raw:
            lib.free(p)


# ---- 5. fold ----
def fold_domains():
    return [("std", std_basis(10), elem(TOP | 0x77))] + [("derived %d" % i, b, s) for i, (b, s) in enumerate(derived_domains((0x1234 << 192) | 0x1234))]


def check_fold(lib):
    x = seeded("fold x", 1)[0]
    ran = 0
    for name, basis, shift in fold_domains():
        m = basis.shape[0]
        f = seeded("fold %s" % name, 1 << m)
        for eta in list(range(0, 5)) + [m]:             # cosets of 1, 2, 4, 8, 16 and the whole domain
            got = lib.evaluate_next_f_i_over_entire_domain_gf256(f, basis, shift, 1 << eta, x)
            assert np.array_equal(got, oracle.fri_fold_additive(f, basis, shift, 1 << eta, x)), (name, eta)
            if eta == 0:
                assert np.array_equal(got, f)
            if eta == m:        # the interpolant of f on the whole domain, at x
                coeffs = oracle.additive_ifft(f, basis, shift)
                assert np.array_equal(got, oracle.poly_eval(coeffs, x).reshape(1, W)), name
            ran += 1
    assert ran == 4 * 6
    # x on the domain: the fold returns f there (fri_aux.tcc:77-86)
    basis, shift = std_basis(6), elem(1 << 200)
    f = seeded("fold on domain", 64)
    xs = oracle.all_subset_sums(basis, shift)[13]
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf256(f, basis, shift, 4, xs), oracle.fri_fold_additive(f, basis, shift, 4, xs))
    dep = std_basis(6).copy()
    dep[1] = dep[0]
    with pytest.raises(ValueError, match="linearly dependent"):
        lib.evaluate_next_f_i_over_entire_domain_gf256(f, dep, shift, 4, x)


def check_fold_chain(lib):
    """[2, 2, 1] on an LDE of 2^6 coefficients onto m = 11: every folded codeword stays below its degree bound"""
    basis, shift = std_basis(11), elem(TOP | 1)
    f = lib.additive_FFT_gf256(seeded("chain", 1 << 6), basis, shift)
    domains = lib.fri_additive_domains_gf256(basis, shift, [2, 2, 1])
    bound = 1 << 6
    for i, eta in enumerate([2, 2, 1]):
        b, s = domains[i]
        f = lib.evaluate_next_f_i_over_entire_domain_gf256(f, b, s, 1 << eta, seeded("chain x %d" % i, 1)[0])
        bound >>= eta
        nb, ns = domains[i + 1]
        coeffs = lib.additive_IFFT_gf256(f, nb, ns)
        assert coeffs[:bound].any() and not coeffs[bound:].any(), i


# ---- 6. domain chain ----
def check_domain_chain(lib):
    basis, shift = std_basis(12), elem(TOP | 0xABC)
    for loc in ([1, 2, 2], [3, 1]):
        got = lib.fri_additive_domains_gf256(basis, shift, loc)
        want = oracle.fri_domains_additive(basis, shift, loc)
        assert len(got) == len(loc) + 1
        for (gb, gs), (wb, ws) in zip(got[1:], want):
            assert np.array_equal(gb, wb) and np.array_equal(gs.reshape(-1), ws.reshape(-1)), loc
    with pytest.raises(ValueError, match="exceed the domain dimension"):
        lib.fri_additive_domains_gf256(std_basis(3), shift, [2, 2])


# ---- 7. LDT combination ----
LDT_CASES = [
    ("one maximal", [2048]),
    ("seven mixed", [2048, 2047, 2047, 1024, 2046, 2048, 1025]),
    ("bump not a power of two", [1000, 233, 1000 - 7]),
]


def check_ldt(lib):
    m = 11
    for basis, shift in ((std_basis(m), elem(TOP | 0xF0F)), tuple(derived_domains(3 << 64)[0])):
        for name, degrees in LDT_CASES:
            evals = [seeded("ldt %s %d" % (name, k), 1 << m) for k in range(len(degrees))]
            coef = seeded("ldt coef " + name, 2 * len(degrees))
            got = lib.ldt_combine_gf256(evals, degrees, coef, basis, shift)
            assert np.array_equal(got, oracle.ldt_combine_additive(evals, degrees, coef, basis, shift)), name


# ---- 8. the generic paths on 32-byte binary elements ----
def check_merkle_and_queries(lib):
    for num_oracles in (1, 5):
        oracles = [seeded("merkle %d %d" % (num_oracles, k), 64) for k in range(num_oracles)]
        for coset in (1, 2, 4):
            assert np.array_equal(lib.merkle_tree(oracles, coset), oracle.merkle_build(oracles, coset)), (num_oracles, coset)
        ptrs = [lib.malloc(32 * 64) for _ in oracles]
        try:
            for p, o in zip(ptrs, oracles):
                lib.h2d(p, o)
            positions = [0, 63, 17, 17, 32]
            got = np.asarray(lib.query_responses_dev(ptrs, 32, 64, positions)).reshape(len(positions), num_oracles, W)
            assert np.array_equal(got, np.array([[o[p] for o in oracles] for p in positions], dtype=np.uint64))
        finally:
            for p in ptrs:
                lib.free(p)


# ---- 9. host and device forms, argument checks ----
def check_host_and_device_forms(lib):
    m, basis, shift = 9, std_basis(9), elem(1 << 200)
    n = 1 << m
    coeffs, x = seeded("forms", n - 5), elem((0xDEADBEEF << 192) | 0x12345)
    d_in, d_out = lib.malloc(32 * n), lib.malloc(32 * n)
    try:
        lib.h2d(d_in, coeffs)
        lib.additive_FFT_dev(d_in, coeffs.shape[0], basis, shift, d_out, words=4)
        evals = np.empty((n, W), dtype=np.uint64)
        lib.d2h(evals, d_out)
        assert np.array_equal(evals, lib.additive_FFT_gf256(coeffs, basis, shift))
        lib.additive_IFFT_dev(d_out, basis, shift, d_in, words=4)
        back = np.empty((n, W), dtype=np.uint64)
        lib.d2h(back, d_in)
        assert np.array_equal(back, lib.additive_IFFT_gf256(evals, basis, shift))
        lib.fri_fold_dev(d_out, basis, shift, 8, x, d_in, words=4)
        folded = np.empty((n // 8, W), dtype=np.uint64)
        lib.d2h(folded, d_in)
        assert np.array_equal(folded, lib.evaluate_next_f_i_over_entire_domain_gf256(evals, basis, shift, 8, x))
        lib.h2d(d_in, evals)
        lib.field_add_dev(d_in, d_out, d_out, n, words=4)            # a + a = 0
        lib.d2h(back, d_out)
        assert not back.any()
    finally:
        lib.free(d_in)
        lib.free(d_out)


def check_argument_checks(lib):
    """each refusal carries the gf128 twin's message"""
    c = lib.c
    basis, shift, x = std_basis(4), elem(0), elem(7)
    b2, s2, x2 = basis[:, :2].copy(), shift[:2].copy(), x[:2].copy()
    f = seeded("checks", 16)
    fp = f.ctypes.data_as(U64P)
    big, big2 = std_basis(41), oracle.standard_basis(41, 2)
    arg = lambda g, four, two: (four if g == "gf256" else two).ctypes.data_as(U64P)
    bp, sp, xp, gp = (lambda g: arg(g, basis, b2)), (lambda g: arg(g, shift, s2)), (lambda g: arg(g, x, x2)), (lambda g: arg(g, big, big2))
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
        ("null argument", lambda g: getattr(c, "iopx_%s_add_dev" % g)(None, None, None, 3)),
    ]
    for text, call in calls:
        msgs = []
        for g in ("gf128", "gf256"):
            with pytest.raises(ValueError, match=text) as e:
                lib._check(call(g))
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], msgs
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf256(f, basis, shift, 3, x)
    with pytest.raises(ValueError, match="bad coset size"):
        lib.evaluate_next_f_i_over_entire_domain_gf256(f, basis, shift, 32, x)
    dep = std_basis(4).copy()
    dep[2] = dep[0] ^ dep[1]
    with pytest.raises(ValueError, match="additive FFT: basis vectors are linearly dependent"):
        lib.additive_FFT_gf256(f, dep, shift)
    # the size-zero and size-one edge cases are accepted as the twin accepts them
    assert np.array_equal(lib.additive_FFT_gf256(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_IFFT_gf256(f[:1], std_basis(0), elem(5)), f[:1])
    assert np.array_equal(lib.additive_FFT_gf256(f[:0], basis, shift), np.zeros((16, W), dtype=np.uint64))
    assert np.array_equal(lib.additive_FFT_gf256(f[:1], basis, shift), np.repeat(f[:1], 16, axis=0))
    assert np.array_equal(lib.evaluate_next_f_i_over_entire_domain_gf256(f, basis, shift, 1, x), f)


# ---- 10. the other fields are unchanged: the dispatch guard ----
def check_dispatch_guard(lib, torch, device):
    """Four words with a prime field are still alt_bn128 Fr's operators, with the same refusal from a subclass; two words are still gf128's;
    and a gf128 and a gf192 transform give the oracle's bytes under the profile names they had."""
    from libiop_amd import dist, domains
    assert type(domains.DeviceOps(lib, torch, device, domains.AltBn128Fr())) is domains.AltBn128DeviceOps
    assert type(domains.DeviceOps(lib, torch, device, domains.GF128())) is domains.GF128DeviceOps
    assert type(domains.DeviceOps(lib, torch, device, domains.GF64())) is domains.GF64DeviceOps
    assert type(domains.DeviceOps(lib, torch, device, domains.GF192())) is domains.DeviceOps
    assert type(domains.DeviceOps(lib, torch, device, domains.GF256())) is domains.GF256DeviceOps
    sharded = [getattr(dist, n) for n in dir(dist) if isinstance(getattr(dist, n), type) and issubclass(getattr(dist, n), domains.DeviceOps)
               and getattr(dist, n).__module__ == dist.__name__]
    assert sharded
    for cls in sharded:
        with pytest.raises(NotImplementedError, match="no operators over a four-word field \\(alt_bn128 Fr runs on one GPU"):
            domains.DeviceOps.__init__(object.__new__(cls), lib, torch, device, domains.AltBn128Fr())
        with pytest.raises(NotImplementedError, match="no operators over a two-word field \\(gf128 runs on one GPU"):
            domains.DeviceOps.__init__(object.__new__(cls), lib, torch, device, domains.GF128())
        with pytest.raises(NotImplementedError, match="gf256"):
            domains.DeviceOps.__init__(object.__new__(cls), lib, torch, device, domains.GF256())
    m = 6
    n = 1 << m
    rng = np.random.default_rng(256)
    for words, names in ((2, {"k128_pad_copy": 1, "k128_phase1": 1, "k128_bfly_edge": 1}), (3, GF192_FFT_PROFILE)):
        basis = oracle.standard_basis(m, words)
        shift = rng.integers(0, MASK64, size=words, dtype=np.uint64, endpoint=True)
        coeffs = rng.integers(0, MASK64, size=(n, words), dtype=np.uint64, endpoint=True)
        d = [lib.malloc(8 * words * n) for _ in range(2)]
        try:
            lib.h2d(d[0], coeffs)
            lib.additive_FFT_dev(d[0], n, basis, shift, d[1], words=words)      # a first call builds the plan: its kernels are not the transform's
            lib.profile_begin()
            lib.additive_FFT_dev(d[0], n, basis, shift, d[1], words=words)
            got = np.empty((n, words), dtype=np.uint64)
            lib.d2h(got, d[1])
            rep = lib.profile_report()
        finally:
            for p in d:
                lib.free(p)
        assert np.array_equal(got, oracle.additive_fft(coeffs, basis, shift)), words
        assert {k: v[0] for k, v in rep.items() if k != "k_upload_small"} == names, (words, rep)      # the staged upload of the shift terms aside


# what one gf192 transform of 2^6 coefficients onto 2^6 points reported before the gf256 arm existed
GF192_FFT_PROFILE = {"k_pad_copy": 1, "k_phase1_fwd": 1, "k_bfly_edge_fwd": 1}


# ---- 11. FRI-only SNARK ----
FRI_SNARK_TUPLES = [(8, 2, 2, 1, 6), (10, 2, 1, 1, 4), (12, 3, 3, 2, 8)]      # (dim, rs_extra, loc, interactions, queries)
GF64_SIZES = [2272, 3648, 6088]
GF256_SIZES = [3472, 4632, 11656]


@functools.lru_cache(maxsize=None)
def model_bytes(words, t):
    """the model's transcript of tuple t with seed 5, computed once and shared by the tests that compare with it"""
    import gf128_fri_snark_model as M
    return M.prove(words, *t, seed=5)


def check_model_reproduces_oracle():
    """the trust condition of tests/gf128_fri_snark_model.py: at one and three words it is the oracle's prover, byte for byte"""
    for words, code in ((1, oracle.FIELD_GF64), (3, oracle.FIELD_GF192)):
        for t, size in zip(FRI_SNARK_TUPLES, GF64_SIZES):
            ref = oracle.fri_snark_prove(code, *t, 5)
            assert words != 1 or len(ref) == size
            assert model_bytes(words, t) == ref, (words, t)


def check_fri_snark(lib, torch, device, trust=True, tuples=None):
    """fri.fri_snark_prover over domains.GF256 and the native prover against the model at four words, byte for byte, and against each other.
    trust: first hold the model to its trust condition (the CPU leg does; the GPU leg relies on it).  tuples: indices into FRI_SNARK_TUPLES
    (the test files run one tuple per case)"""
    import libiop_amd
    from libiop_amd import domains, fri, host, r1cs
    if trust:
        check_model_reproduces_oracle()
    field = domains.GF256()
    hc, ohc = host.Blake2bHashchain(), oracle.Hashchain()
    for n in (1, 2, 5):
        assert np.array_equal(field.squeeze(hc, n), ohc.squeeze(n, W)), n
    ops = domains.DeviceOps(lib, torch, device, field)
    assert type(ops) is domains.GF256DeviceOps
    for k in range(len(FRI_SNARK_TUPLES)) if tuples is None else tuples:
        t, size = FRI_SNARK_TUPLES[k], GF256_SIZES[k]
        dim, rs_extra, loc, interactions, queries = t
        params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
        coeffs = r1cs.seeded_elements(field, 5, 1 << (dim - rs_extra))
        want = model_bytes(W, t)
        assert len(want) == size
        d_coeffs = ops.upload(coeffs)
        mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=d_coeffs).serialize()
        assert mine == want, (t, next((i for i, (a, b) in enumerate(zip(mine, want)) if a != b), min(len(mine), len(want))), len(mine), len(want))
        nat = lib.fri_snark_prove(libiop_amd.FIELD_GF256, d_coeffs.data_ptr(), coeffs.shape[0], dim, rs_extra, loc, interactions, queries)
        assert nat == want, t
        assert nat == mine, t
    with pytest.raises(NotImplementedError, match="gf256"):
        ops.rowcheck(None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="gf256"):
        ops.mul(None, None)


def check_native_refusals(lib, torch, device):
    """Aurora instances over field 6, Poseidon and a communicator are refused by name; codes 3, 7 and 9 stay unknown; the FRI prover still
    proves afterwards"""
    import libiop_amd
    from libiop_amd import domains, r1cs
    assert libiop_amd.FIELD_GF256 == 6
    with pytest.raises(ValueError, match="iopx_aurora_example_instance_create: only the FRI-only SNARK is built over gf256"):
        lib.aurora_example_instance(libiop_amd.FIELD_GF256, 16, 3, 15, 1)
    ops = domains.DeviceOps(lib, torch, device, domains.GF256())
    t = FRI_SNARK_TUPLES[0]
    coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (t[0] - t[1]))
    d_coeffs = ops.upload(coeffs)
    with pytest.raises(ValueError, match="gf256 proves with BLAKE2b"):
        lib.fri_snark_prove(libiop_amd.FIELD_GF256, d_coeffs.data_ptr(), coeffs.shape[0], *t, hash=libiop_amd.HASH_POSEIDON_HIGH_ALPHA)
    with pytest.raises(ValueError, match="gf256 has no distributed prover"):
        lib.fri_snark_prove(libiop_amd.FIELD_GF256, d_coeffs.data_ptr(), coeffs.shape[0], *t, comm=ctypes.c_void_p(16))
    for code in (3, 7, 9):
        with pytest.raises(ValueError, match="unknown field"):
            lib.fri_snark_prove(code, d_coeffs.data_ptr(), coeffs.shape[0], *t)
    with pytest.raises(NotImplementedError, match="gf256"):
        ops.rowcheck(None, None, None, None, None)
    with pytest.raises(NotImplementedError, match="gf256"):
        ops.mul(None, None)
    assert lib.fri_snark_prove(libiop_amd.FIELD_GF256, d_coeffs.data_ptr(), coeffs.shape[0], *t) == model_bytes(W, t)
