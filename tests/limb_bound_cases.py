"""Prime-field inputs chosen in their STORED form — the Montgomery words the kernels load — for edwards_Fr (x * 2^192 mod p, seven
29-bit limbs on the device, fp3_dev.h) and alt_bn128 Fr (x * 2^256 mod r, nine limbs, bn254_dev.h), shared by test_limb_bounds_emu.py (the CPU
build of the kernels) and test_gpu_limb_bounds.py (the HIP library).  The other prime-field cases of this suite draw plain integers and
convert them (from_int / edwards_to_montgomery / elem), which turns 0-adjacent, p-adjacent and all-ones values into arbitrary-looking limbs;
here the limb patterns themselves are the inputs.

Expected values are computed with Python integers in this file (one exception: the Poseidon cases compare with oracle/poseidon.hpp, the
CPU oracle of this repository, an implementation that shares no arithmetic with the kernels).  Every transform, fold and combination is linear in the data and its
multipliers (twiddles, shift powers, n^-1, 1/2, fold and combination constants) are plain field values, so T(x R) = R T(x): the references
work directly on the stored integers (tests/golden/make_bn128_tiny.py argues the same).  Two references exist for the transforms — Horner /
direct sums (`fft_naive`, `ifft_naive`, n <= 2^8) and a recursive radix-2 (`fft_radix2`, `ifft_radix2`) — and `check_references_agree`
compares them where both run.

Which primitive's boundary each construction aims at is stated beside it; `COUNTS` records how many vectors put a value of [2^253, r) through
each alt_bn128 entry and how many pairs hit each targeted intermediate, and every check asserts the counts it is there for (`counted`), so an
edit of the patterns cannot silently empty them.  `python tests/limb_bound_cases.py` runs everything on the CPU build and prints the counts."""
import collections
import hashlib

import numpy as np

MASK29 = (1 << 29) - 1
COUNTS = collections.Counter()


class counted:
    """with counted({key: minimum, ...}): the block must add at least `minimum` to COUNTS[key]"""
    def __init__(self, minimums):
        self.minimums = minimums

    def __enter__(self):
        self.before = {k: COUNTS[k] for k in self.minimums}

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            for k, need in self.minimums.items():
                assert COUNTS[k] - self.before[k] >= need, "%s: %d cases, at least %d expected" % (k, COUNTS[k] - self.before[k], need)
        return False


class Field:
    def __init__(self, name, P, words, limbs, generator, two_adicity):
        self.name, self.P, self.words, self.limbs, self.generator, self.two_adicity = name, P, words, limbs, generator, two_adicity
        self.bits = P.bit_length()
        self.R = 1 << (64 * words)

    def gen(self, log_n):
        """the generator of the order-2^log_n subgroup (subgroup.tcc:55-59), a plain integer"""
        return pow(self.generator, (self.P - 1) >> log_n, self.P)

    def inv(self, a):
        return pow(a, self.P - 2, self.P)

    def to_words(self, vals):
        out = np.empty((len(vals), self.words), dtype=np.uint64)
        for i, v in enumerate(vals):
            out[i] = [(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(self.words)]
        return out

    def to_ints(self, a):
        nb = 8 * self.words
        b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
        return [int.from_bytes(b[nb * i:nb * i + nb], "little") for i in range(len(b) // nb)]

    def elem(self, v):
        """a plain field value (a shift, a challenge, a coefficient) -> its Montgomery words"""
        return self.to_words([v % self.P * self.R % self.P])[0]

    def scalar(self, tag):
        return int.from_bytes(hashlib.sha256(("limb bounds %s %s" % (self.name, tag)).encode()).digest() * 2, "little") % self.P

    def random_canonical(self, tag, count):
        """seeded canonical stored values over the FULL range [0, p): rejection sampling, no masking of the top word"""
        rng = np.random.default_rng(int.from_bytes(hashlib.sha256(("limb bounds data %s %s" % (self.name, tag)).encode()).digest()[:8], "little"))
        out = []
        while len(out) < count:
            raw = rng.integers(0, np.iinfo(np.uint64).max, size=(2 * (count - len(out)) + 8, self.words), dtype=np.uint64, endpoint=True)
            raw[:, -1] &= np.uint64((1 << (self.bits - 64 * (self.words - 1))) - 1)
            out += [v for v in self.to_ints(raw) if v < self.P]
        return out[:count]


FP = Field("edwards_Fr", 1552511030102430251236801561344621993261920897571225601, 3, 7, 19, 31)
BN = Field("alt_bn128_Fr", 21888242871839275222246405745257275088548364400416034343698204186575808495617, 4, 9, 5, 28)
FIELDS = {"edwards": FP, "bn128": BN}


# ---- value patterns (stored integers, all canonical) ---------------------------------------------------------------------------------------
def patterns(F):
    """name -> stored integer.  What each group aims at:
      0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2      fp_cond_sub_p / bn9_store_canonical at exactly p; fp_sub / bnw_sub at difference 0 and -1;
      2^k - 1, 2^k, p - 2^k (k = 29 j, 32 j, 64 j)   a carry or borrow across one limb (29), one 32-bit word (fp7_unpack / bn9_unpack / *_pack,
                                                      the fp3 add / sub chains) or one stored word (64);
      ones_i    the largest canonical value with limbs 0..i all-ones: full product columns in fp7_mul / fp7w_mac / bn9_dot, the longest carry
                chain in fp7_norm / bn9_norm / bn9_reduce;
      alt_0 / alt_1   alternating 0 / 0x1fffffff limbs: every second column full, every unpack shift next to an all-ones neighbour;
      alt_bn128 only: 2^253 and up to r - 1 — the top of the canonical range, where a sum of two values reaches q = v >> 254 >= 1 in bn9_reduce."""
    P = F.P
    pats = collections.OrderedDict()
    for name, v in (("0", 0), ("1", 1), ("2", 2), ("p-1", P - 1), ("p-2", P - 2), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2)):
        pats[name] = v
    for k in sorted({k for step in (29, 32, 64) for k in range(step, F.bits, step)}):
        pats["2^%d-1" % k], pats["2^%d" % k], pats["p-2^%d" % k] = (1 << k) - 1, 1 << k, P - (1 << k)
    for i in range(F.limbs):
        s = 29 * (i + 1)
        low = (1 << s) - 1
        if low < P:
            pats["ones_%d" % i] = (((P - 1 - low) >> s) << s) + low
    for phase in (0, 1):
        v = sum(MASK29 << (29 * i) for i in range(F.limbs) if i % 2 == phase)
        while v >= P:
            v &= (1 << (29 * ((v.bit_length() - 1) // 29))) - 1         # drop the top limb that is set
        pats["alt_%d" % phase] = v
    if F is BN:
        lo = 1 << 253
        pats["2^253"], pats["2^253-1"], pats["2^253+1"] = lo, lo - 1, lo + 1
        for k in range(1, 8):
            pats["top_%d/8" % k] = lo + k * (P - 1 - lo) // 8
    assert all(0 <= v < P for v in pats.values())
    return pats


def subset(pats, offset, step):
    """every step-th pattern starting at `offset`: rotating selections, so that over the sizes every pattern appears in every layout"""
    names = list(pats)
    return [names[i] for i in range(offset % step, len(names), step)]


# ---- layouts --------------------------------------------------------------------------------------------------------------------------------
def constant(v, n):
    return [v] * n


def even_odd(u, v, n):
    return [u if i % 2 == 0 else v for i in range(n)]


def impulse(v, pos, n):
    out = [0] * n
    out[pos] = v
    return out


def scattered(F, tag, n):
    """a seeded full-range random vector with the patterns written over seeded positions (all of them when n allows)"""
    out = F.random_canonical(tag, n)
    vals = list(patterns(F).values())
    rng = np.random.default_rng(n)
    for pos, v in zip(rng.permutation(n)[:len(vals)], rng.permutation(len(vals))):
        out[int(pos)] = vals[int(v)]
    return out


PAIR_SWEEP_LOG = 14        # 72^2 ordered pairs of alt_bn128 patterns fit n / 2 = 8192


def pair_sweep(F, log_n=PAIR_SWEEP_LOG):
    """x[k] = pattern i, x[k + n/2] = pattern j, k = i m + j: every ordered pair of patterns meets directly in a first-level butterfly of
    the transforms (twiddle 1: t = b, so a + t and a + 8p - t are formed from the stored patterns themselves — fp7_bfly / bnw_add /
    bnw_sub with sum = p, difference = 0 and -1 among the pairs) and in the (a, b) of a fold (fp_add / fp_sub / bnw_add / bnw_sub)."""
    vals = list(patterns(F).values())
    n, m = 1 << log_n, len(vals)
    assert m * m <= n // 2
    out = [0] * n
    for k in range(n // 2):
        i, j = (k // m) % m, k % m
        out[k], out[k + n // 2] = vals[i], vals[j]
    return out


# ---- references: Python integers only ------------------------------------------------------------------------------------------------------
def _pows(F, base, count):
    out = np.empty(count, dtype=object)
    acc = 1
    for i in range(count):
        out[i] = acc
        acc = acc * base % F.P
    return out


def _obj(vals, n):
    a = np.zeros(n, dtype=object)
    a[:len(vals)] = vals
    return a


def fft_naive(F, coeffs, log_n, shift):
    """Horner's rule at every point shift * g^i"""
    x = _pows(F, F.gen(log_n), 1 << log_n) * shift % F.P
    acc = np.zeros(1 << log_n, dtype=object)
    for c in reversed(coeffs):
        acc = (acc * x + c) % F.P
    return list(acc)


def ifft_naive(F, vals, log_n, shift):
    """c_k = n^-1 shift^-k sum_i v_i g^-ik"""
    n = 1 << log_n
    gi, sinv = F.inv(F.gen(log_n)), F.inv(shift)
    v = _obj(vals, n)
    rows = _pows(F, gi, n)
    out = []
    for k in range(n):
        w = _pows(F, rows[k], n) if n <= 16 else rows[(k * np.arange(n)) % n]
        out.append(int((v * w).sum() % F.P) * F.inv(n) % F.P * pow(sinv, k, F.P) % F.P)
    return out


def _rec(F, a, tw):
    if len(a) == 1:
        return a
    e, o = _rec(F, a[0::2], tw[0::2]), _rec(F, a[1::2], tw[0::2])
    t = tw * o % F.P
    return np.concatenate([(e + t) % F.P, (e - t) % F.P])


def fft_radix2(F, coeffs, log_n, shift):
    n = 1 << log_n
    a = _obj(coeffs, n)
    if shift != 1:
        a = a * _pows(F, shift, n) % F.P
    return list(_rec(F, a, _pows(F, F.gen(log_n), max(n // 2, 1))))


def ifft_radix2(F, vals, log_n, shift):
    n = 1 << log_n
    a = _rec(F, _obj(vals, n), _pows(F, F.inv(F.gen(log_n)), max(n // 2, 1))) * F.inv(n) % F.P
    if shift != 1:
        a = a * _pows(F, F.inv(shift), n) % F.P
    return list(a)


def fft_expected(F, coeffs, log_n, shift):
    return fft_naive(F, coeffs, log_n, shift) if log_n <= 6 else fft_radix2(F, coeffs, log_n, shift)


def ifft_expected(F, vals, log_n, shift):
    return ifft_naive(F, vals, log_n, shift) if log_n <= 6 else ifft_radix2(F, vals, log_n, shift)


def lagrange_at(F, points, values, x):
    P = F.P
    for xk, fk in zip(points, values):
        if xk == x % P:
            return fk
    acc = 0
    for k, (xk, fk) in enumerate(zip(points, values)):
        num, den = 1, 1
        for l, xl in enumerate(points):
            if l != k:
                num, den = num * (x - xl) % P, den * (xk - xl) % P
        acc = (acc + fk * num % P * F.inv(den)) % P
    return acc


_FOLD_WEIGHTS = {}


def fold_weights(F, log_n, shift, eta, x):
    """per coset {j + k n / 2^eta}: the Lagrange weights of its points at x, or the index of the point that x is"""
    key = (F.name, log_n, shift, eta, x)
    if key not in _FOLD_WEIGHTS:
        P, n, c = F.P, 1 << log_n, 1 << eta
        q = n // c
        gp = _pows(F, F.gen(log_n), n)
        rows = []
        for j in range(q):
            pts = [shift * int(gp[j + k * q]) % P for k in range(c)]
            if x % P in pts:
                rows.append(pts.index(x % P))
                continue
            w = []
            for k, xk in enumerate(pts):
                num, den = 1, 1
                for l, xl in enumerate(pts):
                    if l != k:
                        num, den = num * (x - xl) % P, den * (xk - xl) % P
                w.append(num * F.inv(den) % P)
            rows.append(w)
        _FOLD_WEIGHTS[key] = rows
    return _FOLD_WEIGHTS[key]


def fold_expected(F, f, log_n, shift, eta, x):
    """the interpolant of f on each coset {j + k n / 2^eta}, at x (fri_aux.tcc:106-249): Lagrange's formula (`lagrange_at`, weights cached)"""
    q = (1 << log_n) >> eta
    out = []
    for j, w in enumerate(fold_weights(F, log_n, shift, eta, x)):
        vals = [f[j + k * q] for k in range(1 << eta)]
        out.append(vals[w] if isinstance(w, int) else sum(a * b for a, b in zip(vals, w)) % F.P)
    return out


def ldt_expected(F, evals, degrees, coeffs, log_n, shift):
    """combined_LDT_virtual_oracle (ldt_reducer_aux.tcc:3-37,104-128): coefficients_ = {1} + random; oracle k is weighted by coefficients_[k],
    the i-th submaximal one also by coefficients_[num + i] x^(max_degree - degree_k)"""
    P = F.P
    n, num = 1 << log_n, len(evals)
    co = [1] + list(coeffs)
    top = max(degrees)
    xs = [shift * int(v) % P for v in _pows(F, F.gen(log_n), n)]
    out = [0] * n
    sub = 0
    for k in range(num):
        bump = None
        if degrees[k] < top:
            bump = (co[num + sub], top - degrees[k])
            sub += 1
        for j in range(n):
            w = co[k] if bump is None else (co[k] + bump[0] * pow(xs[j], bump[1], P)) % P
            out[j] = (out[j] + w * evals[k][j]) % P
    return out


def check_references_agree(F):
    for log_n in range(0, 9):
        n = 1 << log_n
        for shift in (1, F.scalar("reference shift")):
            for vec in (scattered(F, "reference %d" % log_n, n), even_odd(F.P - 1, patterns(F)["ones_0"], n)):
                assert fft_naive(F, vec, log_n, shift) == fft_radix2(F, vec, log_n, shift), (F.name, log_n)
                assert ifft_naive(F, vec, log_n, shift) == ifft_radix2(F, vec, log_n, shift), (F.name, log_n)
                assert ifft_radix2(F, fft_radix2(F, vec[:n // 2 + 1], log_n, shift), log_n, shift) == vec[:n // 2 + 1] + [0] * (n - n // 2 - 1)


# ---- the library's entries, per field ---------------------------------------------------------------------------------------------------------
def _note_top(F, entry, vec):
    if F is BN and any(v >= (1 << 253) for v in vec):
        COUNTS["bn128 [2^253, r) -> " + entry] += 1


def lib_fft(lib, F, coeffs, log_n, shift):
    _note_top(F, "fft", coeffs)
    fn = lib.multiplicative_FFT if F is FP else lib.multiplicative_FFT_bn128
    return F.to_ints(fn(F.to_words(coeffs), log_n, F.elem(shift)))


def lib_ifft(lib, F, vals, shift):
    _note_top(F, "ifft", vals)
    fn = lib.multiplicative_IFFT if F is FP else lib.multiplicative_IFFT_bn128
    return F.to_ints(fn(F.to_words(vals), F.elem(shift)))


def lib_ifft_known_degree(lib, F, vals, degree, shift):
    _note_top(F, "known-degree ifft", vals)
    fn = lib.multiplicative_IFFT_of_known_degree if F is FP else lib.multiplicative_IFFT_of_known_degree_bn128
    return F.to_ints(fn(F.to_words(vals), degree, F.elem(shift)))


def lib_fold(lib, F, f, shift, eta, x):
    _note_top(F, "fold eta %d" % eta, f)
    fn = lib.multiplicative_evaluate_next_f_i if F is FP else lib.multiplicative_evaluate_next_f_i_bn128
    return F.to_ints(fn(F.to_words(f), F.elem(shift), 1 << eta, F.elem(x)))


def lib_ldt(lib, F, evals, degrees, coeffs, log_n, shift):
    for e in evals:
        _note_top(F, "ldt", e)
    rc = np.stack([F.elem(c) for c in coeffs])
    ev = [F.to_words(e) for e in evals]
    if F is FP:
        return F.to_ints(lib.ldt_combine_multiplicative(ev, degrees, rc, log_n, F.elem(F.gen(log_n)), F.elem(shift)))
    return F.to_ints(lib.ldt_combine_bn128(ev, degrees, rc, F.elem(shift)))


def _same(F, got, want, what):
    """exact equality of canonical words"""
    if got != want:
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        raise AssertionError("%s %s: %d of %d outputs differ, first at %s" % (F.name, what, len(bad), len(want), bad[:6]))


# ---- transforms -------------------------------------------------------------------------------------------------------------------------------
def transform_vectors(F, log_n):
    """(name, vector) for one size: constants of every pattern, pattern i on even / pattern i + log_n on odd positions (every ordered pair runs
    at n = 2: check_all_pairs), impulses at 0, 1, n/2, n-1 of a rotating selection, the scattered and the plain full-range random vectors.
    Above 2^8 a rotating quarter of the patterns (the cost is the Python reference's)."""
    pats = patterns(F)
    names = list(pats)
    n = 1 << log_n
    chosen = names if log_n <= 8 else subset(pats, log_n, 4)
    for a in chosen:
        yield "constant %s" % a, constant(pats[a], n)
        b = names[(names.index(a) + log_n) % len(names)]
        yield "even %s odd %s" % (a, b), even_odd(pats[a], pats[b], n)
    for a in subset(pats, log_n, 8):
        for pos in sorted({0, 1, n // 2, n - 1}):
            yield "impulse %s at %d" % (a, pos), impulse(pats[a], pos, n)
    yield "scattered", scattered(F, "transform %d" % log_n, n)
    yield "random", F.random_canonical("transform %d" % log_n, n)


def check_transforms(lib, F, log_n):
    """IFFT and full-length FFT of every vector with shift 1 (no pre-scaling pass: the first butterflies see the stored patterns), and for
    every fifth vector the coset forms (shift != 1: k_*_scale_pow, the two-level n^-1 shift^-i scaling of the last pass), the degree-aware
    FFT (1, n/2 + 1, n - 1 coefficients: the replicate path) and the known-degree IFFT on the strided sub-coset."""
    n = 1 << log_n
    s = F.scalar("coset shift")
    for idx, (name, vec) in enumerate(transform_vectors(F, log_n)):
        _same(F, lib_ifft(lib, F, vec, 1), ifft_expected(F, vec, log_n, 1), "ifft 2^%d, %s" % (log_n, name))
        _same(F, lib_fft(lib, F, vec, log_n, 1), fft_expected(F, vec, log_n, 1), "fft 2^%d, %s" % (log_n, name))
        if idx % 5 == 0 or name in ("scattered", "random"):
            _same(F, lib_ifft(lib, F, vec, s), ifft_expected(F, vec, log_n, s), "coset ifft 2^%d, %s" % (log_n, name))
            for count in sorted({1, n // 2 + 1, n - 1, n}):
                if count >= 1:
                    for shift in (1, s):
                        if count == n and shift == 1:
                            continue
                        _same(F, lib_fft(lib, F, vec[:count], log_n, shift), fft_expected(F, vec[:count], log_n, shift),
                              "fft 2^%d of %d coefficients, shift %s, %s" % (log_n, count, "1" if shift == 1 else "s", name))
            for degree in sorted({1, n // 4 + 1, n}):
                if degree >= 1:
                    k = (degree - 1).bit_length()
                    for shift in (1, s):
                        _same(F, lib_ifft_known_degree(lib, F, vec, degree, shift), ifft_expected(F, vec[::n >> k], k, shift),
                              "known-degree ifft 2^%d, degree %d, %s" % (log_n, degree, name))


def check_all_pairs(lib, F):
    """n = 2: every ordered pair of the patterns other than the powers of two (three of those are kept; the pair sweep of
    check_large_transforms runs all pairs of all patterns) as (a, b) of the single butterfly, forward and inverse (the n^-1 product), shift 1"""
    pats = patterns(F)
    vals = [v for k, v in pats.items() if not k.startswith(("2^", "p-2^")) or k.startswith("2^253")] + [pats["2^29-1"], pats["2^64"], pats["p-2^32"]]
    P, half = F.P, (F.P + 1) // 2
    with counted({"%s butterfly sum = p" % F.name: 4, "%s butterfly difference = 0" % F.name: 20, "%s butterfly difference = -1" % F.name: 4}):
        for a in vals:
            for b in vals:
                _same(F, lib_fft(lib, F, [a, b], 1, 1), [(a + b) % P, (a - b) % P], "fft 2 of (%d, %d)" % (a, b))
                _same(F, lib_ifft(lib, F, [a, b], 1), [(a + b) * half % P, (a - b) * half % P], "ifft 2 of (%d, %d)" % (a, b))
                COUNTS["%s butterfly sum = p" % F.name] += (a + b == P)
                COUNTS["%s butterfly difference = 0" % F.name] += (a == b)
                COUNTS["%s butterfly difference = -1" % F.name] += (a - b == -1)


def targeted_butterflies(F):
    """(a, b, c) with the intermediate t = b c at a bound, for a multiplier c known on the host:
    t in {0, 1, p - 1}; a + t = p as integers (fp_cond_sub_p / bn9_store_canonical decide at exactly p; bn9_reduce at q = 1 from below);
    a - t = 0 and a - t = -1 (the borrow of fp_sub, the 8p / 8r padding of fp7_bfly / bnw_sub with nothing left above it)."""
    P = F.P
    for c in (F.scalar("multiplier"), P - 1, (P + 1) // 2, patterns(F)["ones_0"]):
        ci = F.inv(c)
        for t in (0, 1, P - 1, patterns(F)["ones_1"]):
            b = t * ci % P
            for a, what in ((0, "t"), ((P - t) % P, "sum = p"), (t, "difference = 0"), ((t - 1) % P, "difference = -1"), (P - 1, "a = p - 1")):
                yield a, b, c, t, what


def check_targeted_transforms(lib, F):
    """The size-2 forward transform on the coset of shift c: its pre-scaling multiplies coefficient 1 by c, so the butterfly runs on (a, t).
    The size-4 inverse transform of (e_0, e_1, e_2, e_3) = (a, t g, 0, 0), g the generator of order 4: in a decimation-in-time order the
    second level's odd butterfly multiplies the first-level difference of (e_1, e_3) by g^-1, which is t again (the expectation is the
    plain inverse DFT whatever order the kernel uses)."""
    P = F.P
    names = {0: "0", 1: "1", P - 1: "p - 1"}
    need = {"%s targeted: %s" % (F.name, w): 4 for w in ("sum = p", "difference = 0", "difference = -1", "t = 0", "t = 1", "t = p - 1")}
    with counted(need):
        for a, b, c, t, what in targeted_butterflies(F):
            _same(F, lib_fft(lib, F, [a, b], 1, c), [(a + t) % P, (a - t) % P], "targeted fft 2 (%s)" % what)
            COUNTS["%s targeted: %s" % (F.name, what if what in ("sum = p", "difference = 0", "difference = -1") else "t = %s" % names.get(t, "ones"))] += 1
    for a, t, what in sorted({(a, t, what) for a, b, c, t, what in targeted_butterflies(F)}):
        vec = [a, t * F.gen(2) % P, 0, 0]
        _same(F, lib_ifft(lib, F, vec, 1), ifft_naive(F, vec, 2, 1), "targeted ifft 4 (%s)" % what)


def even_odd_closed_forms(F, u, v, log_n):
    """shift 1, u on even and v on odd positions (u = v: a constant vector).  As evaluations, f(g^i) = (u + v)/2 + (u - v)/2 (-1)^i and
    (-1)^i = (g^i)^(n/2): two coefficients.  As coefficients, P(x) = (u + v x)(x^n - 1)/(x^2 - 1) vanishes on the domain except at x = 1 and -1."""
    P, n, half = F.P, 1 << log_n, (F.P + 1) // 2
    inverse, forward = [0] * n, [0] * n
    inverse[0], inverse[n // 2] = (u + v) * half % P, (u - v) * half % P
    forward[0], forward[n // 2] = (u + v) * (n // 2) % P, (u - v) * (n // 2) % P
    return inverse, forward


def check_large_transforms(lib, F, log_n):
    """Two passes (12, 13), two with the pair sweep (14) and three (19): lazily reduced values are stored between the passes, and the 8p-per-level
    growth of fp7_bfly runs through every level.  Constants and even / odd pairs of the extreme patterns, the full-range random vector; at
    2^19 the recursive radix-2 reference checks one forward transform and the closed forms (compared with it at 2^12) the other three."""
    pats = patterns(F)
    n = 1 << log_n
    s = F.scalar("coset shift")
    top = "ones_%d" % (F.limbs - 2)
    pairs = [("p-1", "p-1"), ("p-1", top), (top, top), ("alt_0", "alt_0"), ("1", "1"), ("0", "p-1"), ("alt_1", "alt_0"), ("(p+1)/2", "(p-1)/2"),
             ("ones_0", "p-2")]
    if log_n == 19:
        u, v = pats["p-1"], pats[top]
        _same(F, lib_ifft(lib, F, constant(u, n), 1), even_odd_closed_forms(F, u, u, log_n)[0], "ifft 2^19, constant p-1")
        _same(F, lib_fft(lib, F, even_odd(u, v, n), log_n, 1), fft_radix2(F, even_odd(u, v, n), log_n, 1), "fft 2^19, even p-1 odd %s" % top)
        _same(F, lib_fft(lib, F, constant(u, n), log_n, 1), even_odd_closed_forms(F, u, u, log_n)[1], "fft 2^19, constant p-1")
        _same(F, lib_ifft(lib, F, even_odd(u, v, n), 1), even_odd_closed_forms(F, u, v, log_n)[0], "ifft 2^19, even p-1 odd %s" % top)
        return
    vecs = [("even %s odd %s" % (a, b), even_odd(pats[a], pats[b], n)) for a, b in pairs] + [("random", F.random_canonical("large %d" % log_n, n))]
    if log_n == PAIR_SWEEP_LOG:
        vecs = [("pair sweep", pair_sweep(F))]
        m = len(pats)
        COUNTS["%s first-level butterflies over all ordered pairs" % F.name] += m * m
    for name, vec in vecs:
        inverse, forward = ifft_radix2(F, vec, log_n, 1), fft_radix2(F, vec, log_n, 1)
        if name.startswith("even") and log_n == 12:
            assert (inverse, forward) == even_odd_closed_forms(F, vec[0], vec[1], log_n), name
        _same(F, lib_ifft(lib, F, vec, 1), inverse, "ifft 2^%d, %s" % (log_n, name))
        _same(F, lib_fft(lib, F, vec, log_n, 1), forward, "fft 2^%d, %s" % (log_n, name))
        _same(F, lib_ifft(lib, F, vec, s), ifft_radix2(F, vec, log_n, s), "coset ifft 2^%d, %s" % (log_n, name))
        _same(F, lib_fft(lib, F, vec[:n // 2 + 1], log_n, s), fft_radix2(F, vec[:n // 2 + 1], log_n, s), "coset fft 2^%d, n/2 + 1, %s" % (log_n, name))


# ---- FRI folds --------------------------------------------------------------------------------------------------------------------------------
def fold_vectors(F, log_n):
    pats = patterns(F)
    names = list(pats)
    n = 1 << log_n
    for a in subset(pats, log_n, 3):
        yield "constant %s" % a, constant(pats[a], n)
        b = names[(names.index(a) + log_n) % len(names)]
        yield "even %s odd %s" % (a, b), even_odd(pats[a], pats[b], n)
        yield "halves %s / %s (a = -b)" % (a, a), [pats[a]] * (n // 2) + [(F.P - pats[a]) % F.P] * (n // 2)
    yield "scattered", scattered(F, "fold %d" % log_n, n)
    yield "random", F.random_canonical("fold %d" % log_n, n)


def check_folds(lib, F, log_n):
    """eta = 1, 2, 3 (the fused kernels) and 4 (four k_*_fold2 launches), the challenge off the domain and on it (x = shift g^3: the multiplier
    x / (shift g^j) is 1 at j = 3).  Constant vectors are a = b in every pair (difference 0: fp_sub without borrow, bnw_sub at exactly 8r);
    the "halves" vectors are a = -b (sum = p as integers: fp_add's fp_cond_sub_p at exactly p, bnw_add / bn9_reduce just above 2^254)."""
    s = F.scalar("fold shift")
    for eta in (1, 2, 3, 4):
        if eta > log_n:
            continue
        for x in (F.scalar("fold x"), s * pow(F.gen(log_n), 3, F.P) % F.P):
            for name, vec in fold_vectors(F, log_n):
                _same(F, lib_fold(lib, F, vec, s, eta, x), fold_expected(F, vec, log_n, s, eta, x), "fold 2^%d eta %d, %s" % (log_n, eta, name))


def check_fold_pair_sweep(lib, F):
    """every ordered pair of patterns as (a, b) = (f[j], f[j + n/2]) of a first-level fold, fused (eta 1) and unfused (eta 4)"""
    vec = pair_sweep(F)
    s, x = F.scalar("fold shift"), F.scalar("fold x")
    m = len(patterns(F))
    COUNTS["%s fold pairs a = b" % F.name] += m
    COUNTS["%s fold pairs a = -b" % F.name] += sum(1 for a in patterns(F).values() if (F.P - a) % F.P in set(patterns(F).values()))
    _same(F, lib_fold(lib, F, vec, s, 1, x), fold_expected(F, vec, PAIR_SWEEP_LOG, s, 1, x), "fold of the pair sweep, eta 1")
    _same(F, lib_fold(lib, F, vec, s, 4, x), fold_expected(F, vec, PAIR_SWEEP_LOG, s, 4, x), "fold of the pair sweep, eta 4")


def check_targeted_folds(lib, F):
    """g[j] = ((a + b) + (a - b) c_j) / 2 with c_j = x / (shift g^j) computed here: per output j the pair is chosen so that the product
    t = (a - b) c_j is 0, 1, p - 1 or an all-ones pattern and the sum u = a + b makes u + t = p (as integers), u - t = 0, or u = 0."""
    P = F.P
    log_n = 6
    n = 1 << log_n
    s, x = F.scalar("fold shift"), F.scalar("fold x")
    half = (P + 1) // 2
    cases = []
    for t in (0, 1, P - 1, patterns(F)["ones_1"]):
        for u, what in (((P - t) % P, "sum = p"), (t, "u = t"), (0, "u = 0"), (P - 1, "u = p - 1")):
            cases.append((t, u, what))
    vec = [0] * n
    for j in range(n // 2):
        t, u, what = cases[j % len(cases)]
        cj = x * F.inv(s * pow(F.gen(log_n), j, P) % P) % P
        d = t * F.inv(cj) % P
        vec[j], vec[j + n // 2] = (u + d) * half % P, (u - d) * half % P
        COUNTS["%s targeted fold: product %s, %s" % (F.name, {0: "0", 1: "1", P - 1: "p - 1"}.get(t, "ones"), what)] += 1
    got = lib_fold(lib, F, vec, s, 1, x)
    _same(F, got, fold_expected(F, vec, log_n, s, 1, x), "targeted fold")
    _same(F, got, [(cases[j % len(cases)][1] + cases[j % len(cases)][0]) * half % P for j in range(n // 2)], "targeted fold (by construction)")


# ---- LDT combination --------------------------------------------------------------------------------------------------------------------------
def check_ldt(lib, F, log_n):
    """Maximal degrees only (no degree-bump multiplier) and two submaximal oracles (the bump path: c + c' shift^e g^(e j), fp_add / bnw_add of a
    coefficient and a product); oracles are pattern constants, even / odd pairs and the scattered vector; 3 and 9 oracles (edwards_Fr
    reduces eight products at a time: fp7w_mac / fp7w_redc with 1, 3, 8 + 1 terms)."""
    P = F.P
    pats = patterns(F)
    n = 1 << log_n
    shift = F.generator
    top = "ones_%d" % (F.limbs - 2)
    for num, degrees in ((3, [n, n, n]), (3, [n, n // 2 + 3, 7]), (9, [n] * 9), (9, [n, 5] + [n] * 6 + [n - 1])):
        for variant in range(3):
            if variant == 0:
                evals = [constant(P - 1, n)] * num
                # coefficients whose TABLE FORM (c 2^11 for edwards_Fr, c 2^5 for alt_bn128: what the kernel multiplies by) is an extreme pattern
                up = F.inv(1 << (11 if F is FP else 5))
                coeffs = [[P - 1, pats[top], pats["alt_0"], pats["ones_0"]][i % 4] * up % P * F.inv(F.R) % P for i in range(2 * num)]
            elif variant == 1:
                evals = [even_odd(pats[top], pats["alt_%d" % (k % 2)], n) for k in range(num)]
                coeffs = [F.scalar("ldt coefficient %d" % i) for i in range(2 * num)]
            else:
                evals = [scattered(F, "ldt %d %d" % (log_n, k), n) for k in range(num)]
                coeffs = [F.scalar("ldt coefficient %d" % i) for i in range(2 * num)]
            _same(F, lib_ldt(lib, F, evals, degrees, coeffs, log_n, shift), ldt_expected(F, evals, degrees, coeffs, log_n, shift),
                  "ldt 2^%d, degrees %s, variant %d" % (log_n, degrees, variant))
    # sums of products that are exactly 0, p - 1 and p: out = f_0 + c_1 f_1 with f_1 = (target - f_0) / c_1 (coefficient 0 is 1)
    c1 = F.scalar("ldt coefficient 0")
    f0 = scattered(F, "ldt target", n)
    for target in (0, P - 1, 1):
        f1 = [(target - a) * F.inv(c1) % P for a in f0]
        _same(F, lib_ldt(lib, F, [f0, f1], [n, n], [c1, 5, 7, 11], log_n, shift), [target] * n, "ldt with every output %d" % target)
        COUNTS["%s ldt sum of products = %s" % (F.name, {0: "0 (= p)", 1: "1"}.get(target, "p - 1"))] += n


# ---- edwards_Fr only: sums of products with STORED extremes ------------------------------------------------------------------------------------
def check_lincomb(lib):
    """lincomb / lincomb_affine with 1, 7, 8, 9, 16 terms.  The kernel multiplies the stored vector word by the coefficient's table form
    (c 2^11 mod p, hfp3::table_form), eight products per fp7w_redc; both are set to the patterns here, so fp7w_mac's columns are full
    (all-ones limbs on both sides: 8 * 7 * (2^29 - 1)^2 per column) and p - 1 times p - 1 runs eight times into one reduction.  Then
    terms that sum to exactly 0, p - 1 and p (fp_redc's fp_cond_sub_p, the final fp_add)."""
    F = FP
    P = F.P
    pats = patterns(F)
    up = F.inv(1 << 11)
    extremes = [P - 1, pats["ones_5"], pats["ones_4"], pats["alt_0"], pats["alt_1"], pats["2^174-1"], P - 2, pats["ones_0"]]
    n = len(extremes)

    def run(vecs, coeffs_stored, constant_stored):
        bufs = [lib.malloc(24 * n) for _ in vecs] + [lib.malloc(24 * n)]
        try:
            for b, v in zip(bufs, vecs):
                lib.h2d(b, F.to_words(v))
            out = np.empty((n, 3), dtype=np.uint64)
            co = F.to_words(coeffs_stored)
            if constant_stored is None:
                lib.lincomb_dev(bufs[:-1], co, n, bufs[-1], prime_field=True)
            else:
                lib.lincomb_affine_dev(bufs[:-1], co, F.to_words([constant_stored])[0], n, bufs[-1], prime_field=True)
            lib.d2h(out, bufs[-1])
        finally:
            for b in bufs:
                lib.free(b)
        return F.to_ints(out)

    Rinv = F.inv(F.R)
    for terms in (1, 7, 8, 9, 16):
        for rot in range(len(extremes)):
            vecs = [[extremes[(j + i + rot) % n] for j in range(n)] for i in range(terms)]
            tables = [extremes[(i + rot) % n] for i in range(terms)]             # what fp7w_mac sees
            coeffs = [t * up % P for t in tables]                                # stored coefficient: table = stored * 2^11
            want = [sum(v[j] * c for v, c in zip(vecs, coeffs)) * Rinv % P for j in range(n)]
            _same(F, run(vecs, coeffs, None), want, "lincomb, %d terms" % terms)
            for const in (0, P - 1, pats["ones_5"]):
                _same(F, run(vecs, coeffs, const), [(w + const) % P for w in want], "lincomb_affine, %d terms" % terms)
        # the last term closes the sum at a chosen value: 0, p - 1, 1
        for target in (0, P - 1, 1):
            vecs = [[extremes[(j + i) % n] for j in range(n)] for i in range(terms)]
            coeffs = [extremes[i % n] * up % P for i in range(terms)]
            partial = [sum(v[j] * c for v, c in zip(vecs[:-1], coeffs[:-1])) * Rinv % P for j in range(n)]
            vecs[-1] = [(target - partial[j]) * F.inv(coeffs[-1] * Rinv % P) % P for j in range(n)]
            _same(F, run(vecs, coeffs, None), [target] * n, "lincomb closing at %d, %d terms" % (target, terms))
            _same(F, run(vecs, coeffs, (P - target) % P), [0] * n, "lincomb_affine closing at p, %d terms" % terms)
            COUNTS["edwards_Fr lincomb sum = %s" % {0: "0", 1: "1"}.get(target, "p - 1")] += n


def check_elementwise(lib):
    """k_fp3_mul / k_fp3_sub / k_fp3_inv / k_div_fp3 on every ordered pair of patterns (stored words in, libff's form out):
    mul = a b / R, sub at difference 0 and -1, inv and div with zero denominators giving zero."""
    F = FP
    P = F.P
    vals = list(patterns(F).values())
    a = [u for u in vals for _ in vals]
    b = [v for _ in vals for v in vals]
    n = len(a)
    Rinv = F.inv(F.R)
    d_a, d_b, d_o = lib.malloc(24 * n), lib.malloc(24 * n), lib.malloc(24 * n)
    try:
        lib.h2d(d_a, F.to_words(a))
        lib.h2d(d_b, F.to_words(b))
        out = np.empty((n, 3), dtype=np.uint64)
        lib.fp3_mul_dev(d_a, d_b, d_o, n)
        lib.d2h(out, d_o)
        _same(F, F.to_ints(out), [u * v * Rinv % P for u, v in zip(a, b)], "fp3_mul")
        lib.fp3_sub_dev(d_a, d_b, d_o, n)
        lib.d2h(out, d_o)
        _same(F, F.to_ints(out), [(u - v) % P for u, v in zip(a, b)], "fp3_sub")
        lib.field_inv_dev(d_b, d_o, n, prime_field=True)
        lib.d2h(out, d_o)
        # stored v = x R: the inverse's stored word is x^-1 R = R^2 / v
        _same(F, F.to_ints(out), [F.R * F.R * F.inv(v) % P if v else 0 for v in b], "fp3_inv")
        lib.field_div_dev(d_a, d_b, d_o, n, prime_field=True)
        lib.d2h(out, d_o)
        _same(F, F.to_ints(out), [u * F.R * F.inv(v) % P if v else 0 for u, v in zip(a, b)], "fp3_div")
    finally:
        for d in (d_a, d_b, d_o):
            lib.free(d)


def _pattern_columns(F, count, n):
    """`count` vectors of n stored patterns, rotated against each other so that every position sees a different combination"""
    vals = list(patterns(F).values())
    m = len(vals)
    return [[vals[(j * (k + 1) + 7 * k) % m] for j in range(n)] for k in range(count)]


def _domain(F, log_n, shift):
    return [shift * int(v) % F.P for v in _pows(F, F.gen(log_n), 1 << log_n)]


def _with_buffers(lib, F, arrays, n_out, call):
    bufs = [lib.malloc(max(24 * len(a), 8)) for a in arrays] + [lib.malloc(24 * n_out)]
    try:
        for b, a in zip(bufs, arrays):
            lib.h2d(b, F.to_words(a))
        call(bufs[:-1], bufs[-1])
        out = np.empty((n_out, 3), dtype=np.uint64)
        lib.d2h(out, bufs[-1])
    finally:
        for b in bufs:
            lib.free(b)
    return F.to_ints(out)


def check_virtual_oracles(lib, log_n=7, sub_log=4):
    """rowcheck, fz, sumcheck_g and lincheck in their multiplicative forms with stored patterns in every input vector.  Stored words are x R,
    so a product of two data values is a b / R on the stored integers; the vanishing polynomials and x are plain field values.
    rowcheck: (Az Bz - Cz) / Z_H(x) — fp7w_mac of two data words plus (p - Cz) times the stored 1, and Cz chosen so that the difference is
    exactly 0 (the sum in the accumulator is a multiple of p); fz: fw Z_I(x) + f1v; sumcheck_g: (f - mu / |H| - Z_H(x) h) / x, two fp_sub with
    differences 0 and -1 among the pattern pairs; lincheck: (sum_m r_m Mz_m) p1 - fz p2 with 1, 3 and 8 matrices (one fp7w_redc of eight
    products whose table operands are extreme patterns), and fz p2 chosen equal to the first term."""
    F = FP
    P, Rinv = F.P, F.inv(F.R)
    n, order = 1 << log_n, 1 << sub_log
    shift, sub_shift = F.generator, F.scalar("sub-domain shift")
    gen = F.elem(F.gen(log_n))
    xs = _domain(F, log_n, shift)
    z = [(pow(x, order, P) - pow(sub_shift, order, P)) % P for x in xs]
    az, bz, cz, hv = _pattern_columns(F, 4, n)
    # rowcheck
    for name, c in (("patterns", cz), ("Az Bz = Cz", [a * b * Rinv % P for a, b in zip(az, bz)])):
        got = F.to_ints(lib.rowcheck_multiplicative(F.to_words(az), F.to_words(bz), F.to_words(c), log_n, gen, F.elem(shift), sub_log, F.elem(sub_shift)))
        _same(F, got, [(a * b * Rinv - cc) * F.inv(zz) % P for a, b, cc, zz in zip(az, bz, c, z)], "rowcheck, %s" % name)
        if name != "patterns":
            assert got == [0] * n
            COUNTS["edwards_Fr rowcheck difference = 0"] += n
    # fz
    got = F.to_ints(lib.fz_multiplicative(F.to_words(az), F.to_words(bz), log_n, gen, F.elem(shift), sub_log, F.elem(sub_shift)))
    _same(F, got, [(a * zz + b) % P for a, b, zz in zip(az, bz, z)], "fz")
    f1v = [(-a * zz) % P for a, zz in zip(az, z)]                      # fw Z_I + f1v = p as integers
    _same(F, F.to_ints(lib.fz_multiplicative(F.to_words(az), F.to_words(f1v), log_n, gen, F.elem(shift), sub_log, F.elem(sub_shift))), [0] * n, "fz closing at p")
    COUNTS["edwards_Fr fz sum = p"] += sum(1 for a in az if a)
    # sumcheck_g
    for mu in (0, P - 1, patterns(F)["ones_5"]):                       # the stored word of the claimed sum
        c = mu * F.inv(order) % P
        got = F.to_ints(lib.sumcheck_g_multiplicative(F.to_words(az), F.to_words(hv), log_n, gen, F.elem(shift), sub_log, F.elem(sub_shift), F.to_words([mu])[0]))
        _same(F, got, [(a - c - zz * h) * F.inv(x) % P for a, h, zz, x in zip(az, hv, z, xs)], "sumcheck_g, mu %d" % mu)
    # lincheck
    up = F.inv(1 << 11)
    extremes = [P - 1, patterns(F)["ones_5"], patterns(F)["alt_0"], patterns(F)["ones_4"], patterns(F)["alt_1"], P - 2, patterns(F)["2^174-1"], patterns(F)["ones_0"]]
    for num in (1, 3, 8):
        mz = _pattern_columns(F, num + 3, n)
        fzv, p1, p2, mz = mz[0], mz[1], mz[2], mz[3:]
        r_stored = [extremes[m] * up % P for m in range(num)]              # table form (r 2^11) = the extreme pattern
        comb = [sum(r * v[j] for r, v in zip(r_stored, mz)) * Rinv % P for j in range(n)]
        for name, q2 in (("patterns", p2), ("terms equal", [comb[j] * p1[j] * F.inv(fzv[j]) % P if fzv[j] else 0 for j in range(n)])):
            got = F.to_ints(lib.lincheck(F.to_words(fzv), [F.to_words(v) for v in mz], F.to_words(r_stored), F.to_words(p1), F.to_words(q2), prime_field=True))
            _same(F, got, [(comb[j] * p1[j] - fzv[j] * q2[j]) * Rinv % P for j in range(n)], "lincheck, %d matrices, %s" % (num, name))
            if name != "patterns":
                COUNTS["edwards_Fr lincheck difference = 0"] += sum(1 for j in range(n) if fzv[j] and got[j] == 0)


def check_sparse_and_division(lib):
    """k_spmv_fp3: rows of 0, 1, 2, 9 and 40 entries whose coefficients AND vector entries are stored patterns (data x data products summed with
    fp_add, then one product with the scale), with and without a scale and accumulation, and rows closed at 0 and p - 1.  The division by
    X^N - shift^N (k_polydiv_pass_fp3, one pass per doubling of the offset): 1, 2 and 4 passes over pattern coefficients."""
    F = FP
    P, Rinv = F.P, F.inv(F.R)
    vals = list(patterns(F).values())
    m = len(vals)
    lens = [0, 1, 2, 9, 40, 1, 3, 8, 16, 5] * 3
    row_ptr, col, coeff = [0], [], []
    for r, ln in enumerate(lens):
        for t in range(ln):
            col.append((5 * r + 3 * t) % m)
            coeff.append(vals[(r + 7 * t) % m])
        row_ptr.append(len(col))
    vec = list(vals)
    rows = len(lens)
    plain = [sum(coeff[t] * vec[col[t]] for t in range(row_ptr[r], row_ptr[r + 1])) * Rinv % P for r in range(rows)]
    # close the rows that have at least two entries at 0 and p - 1 through their last coefficient
    for r in range(rows):
        if lens[r] >= 2 and vec[col[row_ptr[r + 1] - 1]]:
            t = row_ptr[r + 1] - 1
            target = (0, P - 1)[r % 2]
            rest = (plain[r] - coeff[t] * vec[col[t]] * Rinv) % P
            coeff[t] = (target - rest) * F.R * F.inv(vec[col[t]]) % P
            plain[r] = target
            COUNTS["edwards_Fr spmv row sum = %s" % ("0" if target == 0 else "p - 1")] += 1
    d_rp, d_col, d_co, d_vec, d_out = lib.malloc(8 * len(row_ptr)), lib.malloc(4 * len(col)), lib.malloc(24 * len(coeff)), lib.malloc(24 * m), lib.malloc(24 * rows)
    try:
        lib.h2d(d_rp, np.array(row_ptr, dtype=np.uint64))
        lib.h2d(d_col, np.array(col, dtype=np.uint32))
        lib.h2d(d_co, F.to_words(coeff))
        lib.h2d(d_vec, F.to_words(vec))
        out = np.empty((rows, 3), dtype=np.uint64)
        start = [vals[(3 * r) % m] for r in range(rows)]
        for scale_stored in (None, P - 1, patterns(F)["ones_5"]):
            k = 1 if scale_stored is None else scale_stored * Rinv % P
            for accumulate in (False, True):
                lib.h2d(d_out, F.to_words(start))
                lib.spmv_dev(d_rp, d_col, d_co, rows, d_vec, d_out, scale=None if scale_stored is None else F.to_words([scale_stored])[0],
                             accumulate=accumulate, prime_field=True)
                lib.d2h(out, d_out)
                _same(F, F.to_ints(out), [(k * v + (s0 if accumulate else 0)) % P for v, s0 in zip(plain, start)], "spmv, scale %s, accumulate %s" % (scale_stored, accumulate))
    finally:
        for d in (d_rp, d_col, d_co, d_vec, d_out):
            lib.free(d)
    for log_order, n_coeffs in ((3, 13), (3, 24), (2, 64), (0, 9)):
        N = 1 << log_order
        shift = F.scalar("division shift")
        c = pow(shift, N, P)
        poly = [vals[(11 * j + 3) % m] for j in range(n_coeffs)]
        work, q = list(poly), [0] * (n_coeffs - N)
        for i in range(n_coeffs - 1, N - 1, -1):                       # schoolbook division by X^N - c
            q[i - N] = work[i]
            work[i - N] = (work[i - N] + c * work[i]) % P
        got = _with_buffers(lib, F, [poly], n_coeffs - N, lambda b, o: lib.poly_div_vanishing_multiplicative_dev(b[0], n_coeffs, log_order, F.elem(shift), o))
        _same(F, got, q, "division of %d coefficients by X^%d - c" % (n_coeffs, N))


def check_rationals(lib, log_n=7, sub_log=3):
    """rational_combine with 1 to 4 rationals (numerators c_i N_i prod_{k != i} D_k summed in one fp7w_redc, the denominators' product) and
    rational_sumcheck_constraint, (D (x p + mu / |K|) - N) / Z_K(x), on stored patterns; N chosen so that the difference is exactly 0."""
    F = FP
    P, Rinv = F.P, F.inv(F.R)
    n = 1 << log_n
    up = F.inv(1 << 11)
    extremes = [P - 1, patterns(F)["ones_5"], patterns(F)["alt_0"], patterns(F)["ones_4"]]
    for num in (1, 2, 3, 4):
        cols = _pattern_columns(F, 2 * num, n)
        Ns, Ds = cols[:num], cols[num:]
        c_stored = [extremes[i] * up % P for i in range(num)]
        wantN, wantD = [], []
        for j in range(n):
            d = [D[j] * Rinv % P for D in Ds]                          # plain values of the denominators
            acc = 0
            for i in range(num):
                term = c_stored[i] * Rinv % P * Ns[i][j] % P
                for k in range(num):
                    if k != i:
                        term = term * d[k] % P
                acc += term
            wantN.append(acc % P)
            prod = Ds[0][j]
            for k in range(1, num):
                prod = prod * d[k] % P
            wantD.append(prod)
        bufs = [lib.malloc(24 * n) for _ in range(2 * num + 2)]
        try:
            for b, v in zip(bufs, Ns + Ds):
                lib.h2d(b, F.to_words(v))
            lib.rational_combine_dev(bufs[:num], bufs[num:2 * num], F.to_words(c_stored), n, bufs[-2], bufs[-1], prime_field=True)
            oN, oD = np.empty((n, 3), dtype=np.uint64), np.empty((n, 3), dtype=np.uint64)
            lib.d2h(oN, bufs[-2])
            lib.d2h(oD, bufs[-1])
        finally:
            for b in bufs:
                lib.free(b)
        _same(F, F.to_ints(oN), wantN, "rational_combine numerator, %d rationals" % num)
        _same(F, F.to_ints(oD), wantD, "rational_combine denominator, %d rationals" % num)
    shift, k_shift = F.generator, F.scalar("summation shift")
    order = 1 << sub_log
    xs = _domain(F, log_n, shift)
    z = [(pow(x, order, P) - pow(k_shift, order, P)) % P for x in xs]
    pv, Nv, Dv = _pattern_columns(F, 3, n)
    gen = F.elem(F.gen(log_n))
    for mu in (0, P - 1, patterns(F)["ones_5"]):
        c = mu * F.inv(order) % P
        s = [(x * a + c) % P for x, a in zip(xs, pv)]
        for name, Nn in (("patterns", Nv), ("D s = N", [d * t * Rinv % P for d, t in zip(Dv, s)])):
            got = _with_buffers(lib, F, [pv, Nn, Dv], n, lambda b, o: lib.rational_sumcheck_constraint_multiplicative_dev(
                b[0], b[1], b[2], log_n, gen, F.elem(shift), sub_log, F.elem(k_shift), F.to_words([mu])[0], o))
            _same(F, got, [(d * t * Rinv - nn) * F.inv(zz) % P for d, t, nn, zz in zip(Dv, s, Nn, z)], "rational_sumcheck_constraint, mu %d, %s" % (mu, name))
            if name != "patterns":
                assert got == [0] * n
                COUNTS["edwards_Fr sumcheck constraint difference = 0"] += n


# ---- alt_bn128 only ---------------------------------------------------------------------------------------------------------------------------
def check_to_montgomery(lib):
    """bn128_to_montgomery (FieldT(bigint)) on 256-bit inputs below, at and above r, up to 2^256 - 1: the patterns, each pattern plus r, 2r,
    ... while it fits, and the top of the 256-bit range"""
    F = BN
    xs = []
    for v in patterns(F).values():
        k = 0
        while v + k * F.P < (1 << 256):
            xs.append(v + k * F.P)
            k += 1
    xs += [(1 << 256) - 1, (1 << 256) - 2, 5 * F.P, 5 * F.P - 1, 5 * F.P + 1, (1 << 255), (1 << 255) - 1, (1 << 254), (1 << 254) - 1]
    got = F.to_ints(lib.bn128_to_montgomery(F.to_words(xs)))
    _same(F, got, [x * F.R % F.P for x in xs], "to_montgomery")
    COUNTS["bn128 to_montgomery inputs at or above r"] += sum(1 for x in xs if x >= F.P)


def check_poseidon(lib, name):
    """poseidon_permute and the Poseidon Merkle leaves / tree levels with states and leaves whose STORED words are the patterns (bn9_load_mont,
    the sbox's bn9_sqr / bn9_mul and bn9_dot<3> / <4> of the MDS layers, bn9_store_mont), against the CPU oracle of this repository
    (oracle/poseidon.hpp) — an implementation that shares no arithmetic with the kernels."""
    import oracle
    import poseidon_cases
    F = BN
    p, po = poseidon_cases.param_pair(name)
    t = p.state_size
    vals = list(patterns(F).values())
    top = [v for v in vals if v >= (1 << 253)]
    states = [[v] * t for v in vals[::3]] + [[vals[(i + 5 * k) % len(vals)] for k in range(t)] for i in range(0, len(vals), 3)]
    states += [[top[(i + k) % len(top)] for k in range(t)] for i in range(0, len(top), 3)]
    st = F.to_words([v for s in states for v in s]).reshape(len(states), t, 4)
    got = lib.poseidon_permute(p, st)
    for i in range(len(states)):
        assert np.array_equal(got[i], oracle.poseidon_permute(po, st[i])), (name, "state %d" % i)
    COUNTS["bn128 [2^253, r) -> poseidon_permute states"] += sum(1 for s in states if any(v >= (1 << 253) for v in s))
    leaves = 16
    for cs in (1, 2, 4):
        n = leaves * cs
        oracles = [F.to_words([vals[(3 * j + k) % len(vals)] for j in range(n)]) for k in range(2)] + [F.to_words(scattered(F, "poseidon", n))]
        assert np.array_equal(lib.merkle_tree_poseidon(p, oracles, cs, 1), oracle.poseidon_merkle(po, oracles, cs, False, None)), (name, cs)
        COUNTS["bn128 [2^253, r) -> poseidon merkle oracles"] += len(oracles)


# ---- the counts each check is there for ---------------------------------------------------------------------------------------------------------
def _counting(fn, minimums):
    def run(lib, *args):
        with counted(minimums(*args)):
            fn(lib, *args)
    run.__doc__, run.__name__ = fn.__doc__, fn.__name__
    return run


def _top(entries, minimum):
    return lambda F, *a: {"bn128 [2^253, r) -> " + e: minimum for e in (entries(*a) if callable(entries) else entries)} if F is BN else {}


def _targets(F):
    need = {"%s targeted fold: product %s, sum = p" % (F.name, t): 1 for t in ("0", "1", "p - 1", "ones")}
    need.update({"%s targeted fold: product %s, u = t" % (F.name, t): 1 for t in ("0", "1", "p - 1")})
    need.update({"%s fold pairs a = b" % F.name: 40, "%s fold pairs a = -b" % F.name: 10})
    need.update(_top(["fold eta 1", "fold eta 4"], 1)(F))
    return need


def _ldt_minimums(F, log_n):
    need = {"%s ldt sum of products = %s" % (F.name, t): 1 << log_n for t in ("0 (= p)", "1", "p - 1")}
    need.update(_top(["ldt"], 10)(F))
    return need


check_transforms = _counting(check_transforms, _top(["fft", "ifft", "known-degree ifft"], 2))
check_large_transforms = _counting(check_large_transforms, _top(["fft", "ifft"], 1))
check_folds = _counting(check_folds, _top(lambda log_n: ["fold eta %d" % e for e in (1, 2, 3, 4) if e <= log_n], 2))
check_fold_pair_sweep_and_targets = _counting(lambda lib, F: (check_fold_pair_sweep(lib, F), check_targeted_folds(lib, F)), _targets)
check_ldt = _counting(check_ldt, _ldt_minimums)
check_lincomb = _counting(check_lincomb, lambda: {"edwards_Fr lincomb sum = %s" % t: 40 for t in ("0", "1", "p - 1")})
check_virtual_oracles = _counting(check_virtual_oracles, lambda *a: {"edwards_Fr rowcheck difference = 0": 128, "edwards_Fr fz sum = p": 100,
                                                                     "edwards_Fr lincheck difference = 0": 100})
check_sparse_and_division = _counting(check_sparse_and_division, lambda: {"edwards_Fr spmv row sum = 0": 3, "edwards_Fr spmv row sum = p - 1": 3})
check_rationals = _counting(check_rationals, lambda *a: {"edwards_Fr sumcheck constraint difference = 0": 128})
check_to_montgomery = _counting(check_to_montgomery, lambda: {"bn128 to_montgomery inputs at or above r": 100})
check_poseidon = _counting(check_poseidon, lambda name: {"bn128 [2^253, r) -> poseidon_permute states": 20, "bn128 [2^253, r) -> poseidon merkle oracles": 9})


if __name__ == "__main__":          # everything on the CPU build, then the counts (the figures quoted in the commit message)
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from emu_lib import emu
    lib = emu()
    for F in (FP, BN):
        check_all_pairs(lib, F)
        check_targeted_transforms(lib, F)
        for log_n in range(1, 12):
            check_transforms(lib, F, log_n)
        for log_n in (12, 13, PAIR_SWEEP_LOG, 19):
            check_large_transforms(lib, F, log_n)
        for log_n in (1, 3, 4, 6, 8):
            check_folds(lib, F, log_n)
        check_fold_pair_sweep_and_targets(lib, F)
        for log_n in (5, 8):
            check_ldt(lib, F, log_n)
    check_lincomb(lib)
    check_elementwise(lib)
    check_virtual_oracles(lib)
    check_sparse_and_division(lib)
    check_rationals(lib)
    check_to_montgomery(lib)
    for name in ("test_params", "starkware_alpha5_t3", "high_alpha17_t3", "high_alpha17_t4"):
        check_poseidon(lib, name)
    for key in sorted(COUNTS):
        print("%6d  %s" % (COUNTS[key], key))
