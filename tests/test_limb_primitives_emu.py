"""The limb primitives of fp3_dev.h (edwards_Fr, seven 29-bit limbs) and bn254_dev.h (alt_bn128 Fr, nine) against their written contracts,
on the CPU: tests/cpp/limb_primitives.cpp exposes them on raw limb vectors (compiled here with the fake HIP header of tests/emu); each is fed
the operands its comment allows — limbs at the stated maximum, values at the stated bound — and both the residue and the PROMISED OUTPUT BOUND
are checked with Python integers."""
import ctypes
import fcntl
import itertools
import os
import subprocess

import numpy as np
import pytest

import limb_bound_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = C.MASK29
P, R = C.FP.P, C.BN.P


@pytest.fixture(scope="module")
def prim():
    src = os.path.join(ROOT, "tests", "cpp", "limb_primitives.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "liblimb_primitives.so")
    deps = [src] + [os.path.join(ROOT, "libiop_amd", "csrc", h) for h in ("fp3_dev.h", "bn254_dev.h")]
    with open(os.path.join(ROOT, "tests", "emu", ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu", "fakehip"),
                                   "-I" + os.path.join(ROOT, "libiop_amd", "csrc"), src, "-o", out + ".tmp"])
            os.replace(out + ".tmp", out)
    return ctypes.CDLL(out)


def limbs(v, count):
    """normalised limbs of v (the top limb takes what is left)"""
    return [(v >> (29 * i)) & M for i in range(count - 1)] + [v >> (29 * (count - 1))]


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def u32(l):
    return np.array(l, dtype=np.uint32)


def call(fn, *args, out=7, dtype=np.uint32):
    o = np.zeros(out, dtype=dtype)
    fn(*[a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a for a in args], o.ctypes.data_as(ctypes.c_void_p))
    return [int(x) for x in o]


def normalised(l):
    return all(x <= M for x in l[:-1])


# ---- edwards_Fr ---------------------------------------------------------------------------------------------------------------------------------
FP_VALUES = [0, 1, P - 1, P, P + 1, 2 * P - 1, (1 << 192) - 1, (1 << 192) - (1 << 29), (1 << 174) - 1, C.patterns(C.FP)["alt_0"], C.patterns(C.FP)["alt_1"]]


def test_fp7_mul_limb_headroom(prim):
    """column sums: limbs up to 2^30 on both sides, or any 32-bit limbs (fp7_bfly says so; fp7_mul's own comment says 2^31) against a
    normalised operand: 7 * (2^32 - 1)(2^29 - 1) + 7 * 2^58 + carry < 2^64.  The residue is exact and the low six limbs are normalised."""
    # the top limbs are kept small: the result's top limb is a 32-bit word, so a b / 2^203 + p must stay below 2^206
    for a, b in (([1 << 30] * 6 + [1 << 20], [1 << 30] * 6 + [1 << 20]), ([(1 << 31) - 1] * 6 + [1 << 20], [M] * 7), ([(1 << 32) - 1] * 6 + [1 << 20], [M] * 7),
                 ([M] * 7, [(1 << 32) - 1] * 6 + [1 << 20]), ([(1 << 32) - 1] * 6 + [1 << 20], limbs(P - 1, 7))):
        r = call(prim.t_fp7_mul, u32(a), u32(b))
        assert normalised(r) and (value(r) << 203) % P == value(a) * value(b) % P, (a, b)
        assert value(r) < value(a) * value(b) // (1 << 203) + P + 1


def test_fp7_mul_value_bound(prim):
    """below 2p with normalised limbs when one value is below 2^192 and the other below p — every caller multiplies data (or a lazily reduced
    value) by a canonical table entry.  (Both at 2^192 give up to 2^181 + p = 2.97 p: the bound the header used to state.)"""
    for a, b in itertools.product(FP_VALUES, [v for v in FP_VALUES if v < P]):
        r = call(prim.t_fp7_mul, u32(limbs(a, 7)), u32(limbs(b, 7)))
        assert normalised(r) and value(r) < 2 * P and (value(r) << 203) % P == a * b % P, (a, b)
    top = (1 << 192) - 1
    assert value(call(prim.t_fp7_mul, u32(limbs(top, 7)), u32(limbs(top, 7)))) >= 2 * P


def test_fp7w_eight_products(prim):
    """eight products of normalised limbs share the column accumulators: 8 * 7 * (2^29 - 1)^2 + 7 * 2^58 + a 35-bit carry is 63 of 64 * 2^58;
    values below 2^192 against values below p give a result below 2p.  A ninth product of all-ones limbs would pass 2^64."""
    group = prim.t_fp7w_max_terms()            # FP7W_MAX_TERMS: the group size of k_lincomb_fp3 / k_ldt_combine_fp / k_lincheck_fp
    assert group >= 8
    for terms in sorted({1, 7, 8, group}):
        a, b = [M] * 7, [M] * 6 + [(1 << 28) - 1]              # all-ones columns; the result (8 a b / 2^203 + p) still fits its 32-bit top limb
        r = call(prim.t_fp7w, u32(a * terms), u32(b * terms), terms)
        assert normalised(r) and (value(r) << 203) % P == terms * value(a) * value(b) % P, terms
        for x, y in (((1 << 192) - 1, P - 1), (P - 1, P - 1), (C.patterns(C.FP)["ones_5"], C.patterns(C.FP)["ones_5"])):
            r = call(prim.t_fp7w, u32(limbs(x, 7) * terms), u32(limbs(y, 7) * terms), terms)
            assert normalised(r) and value(r) < 2 * P and (value(r) << 203) % P == terms * x * y % P, (terms, x, y)
    # the written headroom rule, applied to the group size the kernels were compiled with: `group` products of normalised limbs, the reduction's
    # seven and a 35-bit carry fit a column.  (Nine fail the rule; with this modulus' limbs and a result that fits its 32-bit top limb the
    # worst column of nine is still 0.98 * 2^64, so no output can show it: the rule is what is held.)
    assert (group * 7 + 7) * M * M + (1 << 35) < 1 << 64, "FP7W_MAX_TERMS = %d breaks the headroom rule of fp3_dev.h" % group
    assert 1 << 64 <= (9 * 7 + 7) * M * M


def test_fp7_bfly_three_levels_then_norm_and_pack(prim):
    """no carries for three levels: limbs grow by less than 2^30 per level (the largest limb of the spread 8p is 1.88 * 2^29) and stay below 2^32; values grow by at most 8p per level and
    the packed word is the value itself while it is below 2^192"""
    w = limbs(C.FP.scalar("twiddle"), 7)
    start = (1 << 192) - 24 * P - 1
    for x0, y0 in itertools.product([0, P - 1, (1 << 174) - 1, start], [0, 1, P - 1, start]):
        x, y = u32(limbs(x0, 7)), u32(limbs(y0, 7))
        vx, vy = x0, y0
        for level in range(3):
            t = value(call(prim.t_fp7_mul, u32(w), y))
            assert t < 2 * P
            prim.t_fp7_bfly(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), u32(w).ctypes.data_as(ctypes.c_void_p))
            vx, vy = vx + t, vx + 8 * P - t
            assert (value(x), value(y)) == (vx, vy), "limb-wise: nothing wrapped"
            assert max(max(x), max(y)) < (1 << 29) + (level + 1) * (1 << 30)
            x, y = y.copy(), x.copy()          # the growing difference goes on as the next level's x
            vx, vy = vy, vx
        for arr, v in ((x, vx), (y, vy)):
            assert v < 1 << 192
            words = call(prim.t_fp7_norm_pack, arr, out=6)
            assert sum(wd << (32 * i) for i, wd in enumerate(words)) == v


def test_fp7_canonical_and_cond_sub_at_p(prim):
    for v in FP_VALUES + [2 * P, 7 * P, 2048 * P, (1 << 192) - 8 * P]:
        words = call(prim.t_fp7_canonical, u32(limbs(v, 7)), out=6)
        assert sum(wd << (32 * i) for i, wd in enumerate(words)) == v % P, v
    for v in (0, 1, P - 1, P, P + 1, 2 * P - 1):
        w = u32([(v >> (32 * i)) & 0xFFFFFFFF for i in range(6)])
        prim.t_fp_cond_sub_p(w.ctypes.data_as(ctypes.c_void_p))
        assert sum(int(wd) << (32 * i) for i, wd in enumerate(w)) == (v - P if v >= P else v), v


def test_fp7_unpack_every_bit(prim):
    for bit in range(192):
        for v in (1 << bit, ((1 << 192) - 1) ^ (1 << bit)):
            assert call(prim.t_fp7_unpack, u32([(v >> (32 * i)) & 0xFFFFFFFF for i in range(6)])) == limbs(v, 7), bit


# ---- alt_bn128 Fr -------------------------------------------------------------------------------------------------------------------------------
WEAK = [0, 1, R - 1, R, R + 1, 2 * R - 1, 1 << 253, (1 << 254) - 1, 1 << 254, (1 << 255) - 1, 1 << 255, (1 << 256) - 1, (1 << 256) - (1 << 29),
        C.patterns(C.BN)["alt_0"], C.patterns(C.BN)["alt_1"], C.patterns(C.BN)["ones_7"]]


def test_bn9_dot_limb_headroom(prim):
    """N = 1: both up to 2^30, or 2^31 against normalised; N = 3: one side normalised, the other up to 2^30 — 3 * 9 * 2^59 + 9 * 2^58 is 15.75 of
    16 * 2^60; N = 4: both normalised.  Residues are exact, limbs 0..7 normalised, the value below (sum of products) / 2^261 + r."""
    cases = [(1, [1 << 30] * 9, [1 << 30] * 9), (1, [(1 << 31) - 1] * 9, [M] * 9), (1, [M] * 9, [(1 << 31) - 1] * 9),
             (3, [M] * 27, [1 << 30] * 27), (3, [1 << 30] * 27, [M] * 27), (4, [M] * 36, [M] * 36)]
    for n, a, b in cases:
        r = call(prim.t_bn9_dot, n, u32(a), u32(b), out=9)
        total = sum(value(a[9 * k:9 * k + 9]) * value(b[9 * k:9 * k + 9]) for k in range(n))
        assert normalised(r) and (value(r) << 261) % R == total % R, n
        assert value(r) <= total // (1 << 261) + R
    assert 3 * 9 * (1 << 30) * M + 9 * M * M + (1 << 35) < 1 << 64


def test_bn9_mul_and_sqr_value_bound(prim):
    """inputs below 2^257.5 give a result below 2^255 with normalised limbs; weak (below 2^256) times canonical gives below 2r, which is what
    bn9_store_canonical needs (it subtracts r once)"""
    big = int(2 ** 257.5) - (1 << 205)
    for a, b in itertools.product(WEAK + [big], WEAK + [big]):
        r = call(prim.t_bn9_dot, 1, u32(limbs(a, 9)), u32(limbs(b, 9)), out=9)
        assert normalised(r) and value(r) < 1 << 255 and (value(r) << 261) % R == a * b % R, (a, b)
        if b < R and a < 1 << 256:
            assert value(r) < 2 * R
    for a in WEAK + [big]:
        r = call(prim.t_bn9_sqr, u32(limbs(a, 9)), out=9)
        assert normalised(r) and value(r) < 1 << 255 and (value(r) << 261) % R == a * a % R, a
    a = [1 << 30] * 9                                       # bn9_sqr: limbs up to 2^30
    r = call(prim.t_bn9_sqr, u32(a), out=9)
    assert normalised(r) and (value(r) << 261) % R == value(a) ** 2 % R


def test_bn9_reduce(prim):
    """limbs 0..7 up to 2^32 - 8 (a carry of up to 7 is added to each in 32 bits; limb 8 as large as a sum of a few weak values makes it: below 2^28): same residue, normalised limbs, value
    below 2^254 + q (2^254 - r) with q = v >> 254 — below 2^256 for every sum or difference of weak values (q <= 10)"""
    vecs = [[(1 << 32) - 8] * 8 + [(1 << 28) - 1], [(1 << 32) - 8] * 8 + [0], [0] * 8 + [1 << 22], [M] * 8 + [(1 << 22) - 1], [M] * 8 + [1 << 22]]
    vecs += [limbs(v, 9) for v in WEAK]
    for a in vecs:
        r = call(prim.t_bn9_reduce, u32(a), out=9)
        v = value(a)
        assert normalised(r) and value(r) % R == v % R and value(r) < (1 << 254) + (v >> 254) * ((1 << 254) - R), a


def test_bnw_add_and_sub_of_weak_values(prim):
    """weak in (normalised limbs, below 2^256), weak out; the difference is a + 8r - b with 8r spread so that no limb goes negative"""
    for a, b in itertools.product(WEAK, WEAK):
        s = call(prim.t_bnw_add, u32(limbs(a, 9)), u32(limbs(b, 9)), out=9)
        d = call(prim.t_bnw_sub, u32(limbs(a, 9)), u32(limbs(b, 9)), out=9)
        assert normalised(s) and value(s) < 1 << 256 and value(s) % R == (a + b) % R, (a, b)
        assert normalised(d) and value(d) < 1 << 256 and value(d) % R == (a - b) % R, (a, b)


def test_bn9_store_canonical_needs_below_2r(prim):
    """one conditional subtraction of r: canonical for values below 2r (every product of a weak value and a canonical table entry), decided
    at exactly r.  The header said "below 2^255"; [2r, 2^255) is not reduced — no caller produces it."""
    for y in (0, 1, R - 1, R, R + 1, 2 * R - 1, 1 << 253, (1 << 254) - 1, 1 << 254):
        q = call(prim.t_bn9_store_canonical, u32(limbs(y, 9)), out=4, dtype=np.uint64)
        assert sum(w << (64 * i) for i, w in enumerate(q)) == y % R, y
    for v in WEAK:
        q = call(prim.t_bnw_store, u32(limbs(v, 9)), out=4, dtype=np.uint64)
        assert sum(w << (64 * i) for i, w in enumerate(q)) == v % R, v


def test_bn9_unpack_every_bit(prim):
    for bit in range(256):
        for v in (1 << bit, ((1 << 256) - 1) ^ (1 << bit)):
            q = np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
            assert call(prim.t_bn9_unpack, q, out=9) == limbs(v, 9), bit
