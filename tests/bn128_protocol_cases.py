"""Integer model, input recipes and drivers for the protocol-layer entries over the prime fields (the seventeen iopx_*_bn128_dev
entries and their edwards_Fr twins), shared by the fixture generators (tests/golden/make_bn128_protocol_tiny.py,
make_bn128_protocol_digests_large.py) and the tests (test_bn128_protocol_emu.py, test_gpu_bn128_protocol.py).

The model is written once, over Python integers, and parametrised by the field (p, R, generator, two-adicity, words): run with
edwards_Fr's parameters it must reproduce the existing *_fp3_dev entries bit for bit, which is how it checks itself.

Elements are Montgomery words (x * R mod p, little-endian uint64).  The model decodes every data word to its residue (so raw words
at or above p are read as the entries must read them) and encodes canonical words; x_j = shift * gen^j with gen the generator of
the order-2^log_n subgroup, generator^((p - 1) / 2^log_n)."""
import ctypes

import numpy as np

import bn128_cases as B
from bn128_cases import chunk_digests, data_words, digest, load_json, seeded_scalar  # noqa: F401  (re-exported)

_vp, _sz, _u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)


class Field:
    def __init__(self, name, p, r_bits, generator, two_adicity, words, symbols):
        self.name, self.p, self.R, self.generator, self.two_adicity, self.words = name, p, 1 << r_bits, generator, two_adicity, words
        self.Rinv = pow(self.R, -1, p)
        self.symbols = symbols

    def gen(self, log_n):
        return pow(self.generator, (self.p - 1) >> log_n, self.p)

    def enc(self, v):
        return v % self.p * self.R % self.p

    def dec(self, w):
        return w * self.Rinv % self.p

    def to_words(self, ints):
        out = np.empty((len(ints), self.words), dtype=np.uint64)
        for i, v in enumerate(ints):
            out[i] = [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(self.words)]
        return out

    def to_ints(self, a):
        b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
        step = 8 * self.words
        return [int.from_bytes(b[step * i:step * i + step], "little") for i in range(len(b) // step)]

    def elem(self, v):
        """a plain value -> its Montgomery words"""
        return self.to_words([self.enc(v)])[0]

    def data(self, tag, count):
        """count canonical Montgomery words seeded by tag (the top word masked below the modulus)"""
        w = data_words(self.name + " " + tag if self.words == 3 else tag, count)
        if self.words == 3:
            w = np.ascontiguousarray(w[:, :3])
            w[:, 2] &= np.uint64((1 << 52) - 1)
        return w


_OPS = ["rowcheck", "fz", "sumcheck_g", "lincheck", "spmv", "poly_div_vanishing", "lincomb", "mul", "sub", "inv", "pow_table", "lincomb_affine", "div",
        "domain_offsets", "vanishing_evals", "rational_combine", "rational_sumcheck_constraint"]
_ELEMENTWISE = {"mul", "sub", "inv", "pow_table", "div"}


def _symbols(tag):
    return {op: ("iopx_%s_%s_dev" % (tag, op) if op in _ELEMENTWISE else "iopx_%s_%s_dev" % (op, tag)) for op in _OPS}


BN = Field("alt_bn128_Fr", B.P, 256, B.GENERATOR, B.TWO_ADICITY, 4, _symbols("bn128"))
ED = Field("edwards_Fr", 0x0010357f274a8e56c4e2e493b92e12cc1de5532780000001, 192, 19, 31, 3, _symbols("fp3"))


# ---- the integer model ---------------------------------------------------------------------------------------------------------
def _points(F, log_n, shift, idxs):
    """x_j for j in idxs (a range starting anywhere is walked incrementally)"""
    g = F.gen(log_n)
    if isinstance(idxs, range) and idxs.step == 1 and len(idxs):
        out, x = [], shift * pow(g, idxs.start, F.p) % F.p
        for _ in idxs:
            out.append(x)
            x = x * g % F.p
        return out
    return [shift * pow(g, j, F.p) % F.p for j in idxs]


def _col(F, a, idxs):
    """the residues of the data words of `a` at idxs"""
    if isinstance(idxs, range) and idxs.step == 1 and len(idxs) == len(a) and idxs.start == 0:
        return [F.dec(w) for w in F.to_ints(a)]
    return [F.dec(w) for w in F.to_ints(np.ascontiguousarray(a)[list(idxs)])]


def _batch_inv0(F, vals):
    """the inverses of vals (zero stays zero) with one modular inversion: what makes the 2^22 recipes affordable in Python"""
    p, pre, acc = F.p, [], 1
    for v in vals:
        pre.append(acc)
        if v:
            acc = acc * v % p
    inv, out = pow(acc, p - 2, p), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        if vals[i]:
            out[i] = inv * pre[i] % p
            inv = inv * vals[i] % p
    return out


def _vanishing_inverses(F, xs, order, c):
    """1 / (x^order - c) for x in xs; the values repeat with period |L| / order over a domain, so each is inverted once"""
    cache, out = {}, []
    for x in xs:
        z = (pow(x, order, F.p) - c) % F.p
        if z not in cache:
            cache[z] = pow(z, F.p - 2, F.p)
        out.append(cache[z])
    return out


def model(F, case, inp, idxs=None):
    """[output value lists] of `case` on inputs `inp` at positions idxs (default: all), as plain residues"""
    p, op = F.p, case["op"]
    n = out_count(case)
    idxs = range(n) if idxs is None else idxs
    col = lambda k: _col(F, inp[k], idxs)                                           # noqa: E731
    if op == "rowcheck":
        xs, H = _points(F, case["log_n"], case["shift"], idxs), 1 << case["sub_log"]
        c = pow(case["sub_shift"], H, p)
        return [[(a * b - cc) * zi % p for a, b, cc, zi in zip(col("a"), col("b"), col("c"), _vanishing_inverses(F, xs, H, c))]]
    if op == "fz":
        xs, I = _points(F, case["log_n"], case["shift"], idxs), 1 << case["sub_log"]
        c = pow(case["sub_shift"], I, p)
        return [[(fw * (pow(x, I, p) - c) + f1) % p for fw, f1, x in zip(col("a"), col("b"), xs)]]
    if op == "sumcheck_g":
        xs, H = _points(F, case["log_n"], case["shift"], idxs), 1 << case["sub_log"]
        c, mu_h = pow(case["sub_shift"], H, p), case["mu"] * pow(H, p - 2, p) % p
        return [[(f - mu_h - (pow(x, H, p) - c) * h) * xi % p for f, h, x, xi in zip(col("a"), col("b"), xs, _batch_inv0(F, xs))]]
    if op == "lincheck":
        mz = [col("m%d" % i) for i in range(case["num"])]
        return [[(sum(r * m[t] for r, m in zip(case["coeffs"], mz)) * p1 - fz * p2) % p
                 for t, (fz, p1, p2) in enumerate(zip(col("a"), col("b"), col("c")))]]
    if op == "spmv":
        vec, coeff, prev = _col(F, inp["vec"], range(len(inp["vec"]))), _col(F, inp["coeff"], range(len(inp["coeff"]))), col("out")
        rp, cols = inp["row_ptr"], inp["col"]
        scale = 1 if case["scale"] is None else case["scale"]
        return [[(scale * sum(coeff[t] * vec[int(cols[t])] for t in range(int(rp[r]), int(rp[r + 1]))) + (prev[k] if case["accumulate"] else 0)) % p
                 for k, r in enumerate(idxs)]]
    if op == "poly_div_vanishing":
        N, nc = 1 << case["sub_log"], case["n_coeffs"]
        c = pow(case["shift"], N, p)
        out = []
        for j in idxs:                      # Q_j = P_{j+N} + c P_{j+2N} + ...
            ks = list(range(j + N, nc, N))
            vals = _col(F, inp["a"], ks)
            acc = 0
            for v in reversed(vals):
                acc = (acc * c + v) % p
            out.append(acc)
        return [out]
    if op in ("lincomb", "lincomb_affine"):
        os_ = [col("m%d" % i) for i in range(case["num"])]
        c0 = case["constant"] if op == "lincomb_affine" else 0
        return [[(sum(c * o[t] for c, o in zip(case["coeffs"], os_)) + c0) % p for t in range(len(idxs))]]
    if op == "mul":
        return [[a * b % p for a, b in zip(col("a"), col("b"))]]
    if op == "sub":
        return [[(a - b) % p for a, b in zip(col("a"), col("b"))]]
    if op == "inv":
        return [_batch_inv0(F, col("a"))]
    if op == "div":
        den = col("b")
        num = col("a") if case["with_num"] else [1] * len(den)
        return [[a * b % p for a, b in zip(num, _batch_inv0(F, den))]]
    if op == "pow_table":
        if isinstance(idxs, range) and len(idxs) and idxs.step == 1:
            out, x = [], case["init"] * pow(case["base"], idxs.start, p) % p
            for _ in idxs:
                out.append(x)
                x = x * case["base"] % p
            return [out]
        return [[case["init"] * pow(case["base"], j, p) % p for j in idxs]]
    if op == "domain_offsets":
        return [[(case["point"] - x) % p for x in _points(F, case["log_n"], case["shift"], idxs)]]
    if op == "vanishing_evals":
        S = 1 << case["sub_log"]
        c = pow(case["sub_shift"], S, p)
        return [[(case["constant"] - (pow(x, S, p) - c)) % p for x in _points(F, case["log_n"], case["shift"], idxs)]]
    if op == "rational_combine":
        k = case["num"]
        Ns, Ds = [col("n%d" % i) for i in range(k)], [col("d%d" % i) for i in range(k)]
        outN, outD = [], []
        for t in range(len(idxs)):
            num, den = 0, 1
            for i in range(k):
                term = case["coeffs"][i] * Ns[i][t]
                for q in range(k):
                    if q != i:
                        term = term * Ds[q][t] % p
                num += term
                den = den * Ds[i][t] % p
            outN.append(num % p)
            outD.append(den)
        return [outN, outD]
    if op == "rational_sumcheck_constraint":
        xs, K = _points(F, case["log_n"], case["shift"], idxs), 1 << case["sub_log"]
        c, mu_k = pow(case["sub_shift"], K, p), case["mu"] * pow(K, p - 2, p) % p
        return [[(D * (x * pp + mu_k) - N) * zi % p for pp, N, D, x, zi in zip(col("a"), col("b"), col("c"), xs, _vanishing_inverses(F, xs, K, c))]]
    raise KeyError(op)


def model_words(F, case, inp, idxs=None):
    return [F.to_words([F.enc(v) for v in vals]) for vals in model(F, case, inp, idxs)]


# ---- cases and their inputs ----------------------------------------------------------------------------------------------------
def out_count(case):
    op = case["op"]
    if op in ("rowcheck", "fz", "sumcheck_g", "domain_offsets", "vanishing_evals", "rational_sumcheck_constraint"):
        return 1 << case["log_n"]
    if op == "spmv":
        return case["rows"]
    if op == "poly_div_vanishing":
        return max(0, case["n_coeffs"] - (1 << case["sub_log"]))
    return case["n"]


def _zero_positions(pattern, n):
    if pattern == "none" or n == 0:
        return []
    return {"first": [0], "last": [n - 1], "all": list(range(n)), "some": sorted({0, n // 3, n // 2, n - 1})}[pattern]


def spmv_row_lengths(case):
    rows, kind = case["rows"], case["shape"]
    if kind == "mixed":                     # empty rows, a single-entry row, a long row, short rows
        base = [0, 1, 310, 0, 2, 5, 3, 0, 4, 7]
        return [base[r % len(base)] if r < len(base) else 1 + (r * 7) % 4 for r in range(rows)]
    return [1 + (r * 5) % 3 for r in range(rows)]      # "short": the synthetic instance's one to three entries per row


def inputs(F, case, tag=None):
    """the device vectors of a case, as word arrays keyed by role"""
    tag = tag or case["name"]
    op, n = case["op"], out_count(case)
    inp = {}
    if op in ("rowcheck", "rational_sumcheck_constraint"):
        for k in "abc":
            inp[k] = F.data(tag + " " + k, n)
    elif op in ("fz", "sumcheck_g", "mul", "sub"):
        for k in "ab":
            inp[k] = F.data(tag + " " + k, n)
    elif op == "lincheck":
        for k in "abc":
            inp[k] = F.data(tag + " " + k, n)
        for i in range(case["num"]):
            inp["m%d" % i] = F.data(tag + " m%d" % i, n)
    elif op in ("lincomb", "lincomb_affine"):
        for i in range(case["num"]):
            inp["m%d" % i] = F.data(tag + " m%d" % i, n)
    elif op == "rational_combine":
        for i in range(case["num"]):
            inp["n%d" % i], inp["d%d" % i] = F.data(tag + " n%d" % i, n), F.data(tag + " d%d" % i, n)
    elif op == "poly_div_vanishing":
        inp["a"] = F.data(tag + " a", case["n_coeffs"])
    elif op in ("inv", "div"):
        inp["b" if op == "div" else "a"] = F.data(tag + " den", n)
        if op == "div" and case["with_num"]:
            inp["a"] = F.data(tag + " num", n)
        for z in _zero_positions(case["zeros"], n):
            inp["b" if op == "div" else "a"][z] = 0
    elif op == "spmv":
        lens = spmv_row_lengths(case)
        rp = np.zeros(case["rows"] + 1, dtype=np.uint64)
        rp[1:] = np.cumsum(lens)
        nnz = int(rp[-1])
        seed = int.from_bytes(tag.encode()[:8].ljust(8, b"\0"), "little")
        inp["row_ptr"], inp["col"] = rp, np.random.default_rng(seed).integers(0, case["cols"], size=max(nnz, 1), dtype=np.uint32)
        inp["coeff"], inp["vec"], inp["out"] = F.data(tag + " coeff", max(nnz, 1)), F.data(tag + " vec", case["cols"]), F.data(tag + " out", case["rows"])
    return inp


def _scalar(F, tag):
    return seeded_scalar(tag) % F.p


def _domain_case(F, op, log_n, sub_log, sub_shift_kind, mu_kind="seeded"):
    name = "%s_%d_%d_%s_%s" % (op, log_n, sub_log, sub_shift_kind, mu_kind)
    sub_shift = 1 if sub_shift_kind == "one" else _scalar(F, "sub shift " + op)
    return {"op": op, "name": name, "log_n": log_n, "shift": F.generator, "sub_log": sub_log, "sub_shift": sub_shift,
            "mu": 0 if mu_kind == "zero" else _scalar(F, "mu " + op), "constant": _scalar(F, "constant " + op)}


def tiny_cases(F):
    cases = []
    for log_n in range(4, 11):
        subs = sorted({0, 1, log_n - 2})
        for i, sub in enumerate(subs):
            kind = "one" if (log_n + i) % 2 == 0 else "seeded"
            cases.append(_domain_case(F, "rowcheck", log_n, sub, kind))
            cases.append(_domain_case(F, "fz", log_n, sub, kind))
            cases.append(_domain_case(F, "vanishing_evals", log_n, sub, kind))
            for mu in ("zero", "seeded"):
                cases.append(_domain_case(F, "sumcheck_g", log_n, sub, kind, mu))
                cases.append(_domain_case(F, "rational_sumcheck_constraint", log_n, sub, kind, mu))
        cases.append({"op": "domain_offsets", "name": "domain_offsets_%d" % log_n, "log_n": log_n, "shift": _scalar(F, "offsets shift"), "point": _scalar(F, "offsets point")})
    for num in (1, 3, 8):
        cases.append({"op": "lincheck", "name": "lincheck_%d" % num, "n": 300, "num": num, "coeffs": [_scalar(F, "lincheck r %d" % i) for i in range(num)]})
    for num in (1, 2, 4, 5, 9, 16):
        cs = [_scalar(F, "lincomb c %d" % i) for i in range(num)]
        cases.append({"op": "lincomb", "name": "lincomb_%d" % num, "n": 257, "num": num, "coeffs": cs})
        cases.append({"op": "lincomb_affine", "name": "lincomb_affine_%d" % num, "n": 257, "num": num, "coeffs": cs, "constant": _scalar(F, "affine constant")})
    for num in (1, 2, 3, 4):
        cases.append({"op": "rational_combine", "name": "rational_combine_%d" % num, "n": 259, "num": num, "coeffs": [_scalar(F, "rational c %d" % i) for i in range(num)]})
    for scale in (None, _scalar(F, "spmv scale")):
        for acc in (0, 1):
            cases.append({"op": "spmv", "name": "spmv_mixed_%s_%d" % ("noscale" if scale is None else "scale", acc), "rows": 300, "cols": 97, "shape": "mixed",
                          "scale": scale, "accumulate": acc})
    for nc in (5, 8, 9, 16, 31, 100):       # below, equal to and above |domain| = 8
        cases.append({"op": "poly_div_vanishing", "name": "poly_div_%d" % nc, "n_coeffs": nc, "sub_log": 3, "shift": _scalar(F, "poly div shift")})
    cases.append({"op": "poly_div_vanishing", "name": "poly_div_unit_2000", "n_coeffs": 2000, "sub_log": 0, "shift": 1})
    for n in (1, 3, 255, 1031):             # not multiples of the batch (4) or the workgroup (256)
        for zeros in ("none", "first", "last", "all", "some"):
            cases.append({"op": "inv", "name": "inv_%d_%s" % (n, zeros), "n": n, "zeros": zeros})
            for with_num in (0, 1):
                cases.append({"op": "div", "name": "div_%d_%s_%d" % (n, zeros, with_num), "n": n, "zeros": zeros, "with_num": with_num})
    cases.append({"op": "div", "name": "div_5000_some_1", "n": 5000, "zeros": "some", "with_num": 1})
    for n in (1, 777):
        cases.append({"op": "mul", "name": "mul_%d" % n, "n": n})
        cases.append({"op": "sub", "name": "sub_%d" % n, "n": n})
    for n in (0, 1, 4096, 4097):
        cases.append({"op": "pow_table", "name": "pow_table_%d" % n, "n": n, "base": _scalar(F, "pow base"), "init": _scalar(F, "pow init")})
    return cases


def large_cases(F, m):
    """one case per entry at 2^m elements (SpMV: 2^(m-5) rows of the synthetic instance's shape, at least 2^5)"""
    sub = max(m - 5, 0)
    rows = 1 << max(m - 5, 5)
    cs = lambda k, t: [_scalar(F, "large %s %d" % (t, i)) for i in range(k)]       # noqa: E731
    out = [dict(_domain_case(F, op, m, sub, "seeded"), name="%s_%d" % (op, m)) for op in ("rowcheck", "fz", "sumcheck_g", "vanishing_evals", "rational_sumcheck_constraint")]
    out += [{"op": "domain_offsets", "name": "domain_offsets_%d" % m, "log_n": m, "shift": F.generator, "point": _scalar(F, "large point")},
            {"op": "lincheck", "name": "lincheck_%d" % m, "n": 1 << m, "num": 3, "coeffs": cs(3, "r")},
            {"op": "lincomb", "name": "lincomb_%d" % m, "n": 1 << m, "num": 6, "coeffs": cs(6, "c")},
            {"op": "lincomb_affine", "name": "lincomb_affine_%d" % m, "n": 1 << m, "num": 3, "coeffs": cs(3, "a"), "constant": _scalar(F, "large constant")},
            {"op": "rational_combine", "name": "rational_combine_%d" % m, "n": 1 << m, "num": 3, "coeffs": cs(3, "q")},
            {"op": "spmv", "name": "spmv_%d" % m, "rows": rows, "cols": rows, "shape": "short", "scale": _scalar(F, "large scale"), "accumulate": 1},
            {"op": "poly_div_vanishing", "name": "poly_div_%d" % m, "n_coeffs": 1 << m, "sub_log": max(m - 3, 0), "shift": _scalar(F, "large div shift")},
            {"op": "mul", "name": "mul_%d" % m, "n": 1 << m}, {"op": "sub", "name": "sub_%d" % m, "n": 1 << m},
            {"op": "inv", "name": "inv_%d" % m, "n": 1 << m, "zeros": "some"},
            {"op": "div", "name": "div_%d" % m, "n": 1 << m, "zeros": "some", "with_num": 1},
            {"op": "pow_table", "name": "pow_table_%d" % m, "n": 1 << m, "base": _scalar(F, "large base"), "init": _scalar(F, "large init")}]
    return out


# ---- running a case through a Library (the CPU build or the HIP one) -----------------------------------------------------------
class _Dev:
    """device copies of host arrays, freed together"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = self.lib.malloc(max(a.nbytes, 8))
        self.ptrs.append(d)
        if a.nbytes:
            self.lib.h2d(d, a)
        return d

    def empty(self, nbytes):
        d = self.lib.malloc(max(nbytes, 8))
        self.ptrs.append(d)
        return d

    def down(self, d, count, words):
        out = np.empty((count, words), dtype=np.uint64)
        if count:
            self.lib.d2h(out, d)
        return out

    def close(self):
        for d in self.ptrs:
            self.lib.free(d)
        self.ptrs = []


def _w(F, v):
    return F.elem(v).ctypes.data_as(_u64p)


def _ws(F, vals):
    a = F.to_words([F.enc(v) for v in vals])
    return a, a.ctypes.data_as(_u64p)


def call(lib, F, case, d, d_outs, gen_words=None):
    """the C call of `case` on device pointers d[role] -> return code"""
    op = case["op"]
    fn = getattr(lib.c, F.symbols[op])
    P = lambda k: _vp(d[k])                                                         # noqa: E731
    if op in ("rowcheck", "fz", "sumcheck_g", "domain_offsets", "vanishing_evals", "rational_sumcheck_constraint"):
        g = (F.elem(F.gen(case["log_n"])) if gen_words is None else gen_words).ctypes.data_as(_u64p)
    if op == "rowcheck":
        return fn(P("a"), P("b"), P("c"), case["log_n"], g, _w(F, case["shift"]), case["sub_log"], _w(F, case["sub_shift"]), _vp(d_outs[0]))
    if op == "fz":
        return fn(P("a"), P("b"), case["log_n"], g, _w(F, case["shift"]), case["sub_log"], _w(F, case["sub_shift"]), _vp(d_outs[0]))
    if op == "sumcheck_g":
        return fn(P("a"), P("b"), case["log_n"], g, _w(F, case["shift"]), case["sub_log"], _w(F, case["sub_shift"]), _w(F, case["mu"]), _vp(d_outs[0]))
    if op == "rational_sumcheck_constraint":
        return fn(P("a"), P("b"), P("c"), case["log_n"], g, _w(F, case["shift"]), case["sub_log"], _w(F, case["sub_shift"]), _w(F, case["mu"]), _vp(d_outs[0]))
    if op == "domain_offsets":
        return fn(case["log_n"], g, _w(F, case["shift"]), _w(F, case["point"]), _vp(d_outs[0]))
    if op == "vanishing_evals":
        return fn(case["log_n"], g, _w(F, case["shift"]), case["sub_log"], _w(F, case["sub_shift"]), _w(F, case["constant"]), _vp(d_outs[0]))
    if op == "lincheck":
        ptrs = (_vp * case["num"])(*[d["m%d" % i] for i in range(case["num"])])
        keep, r = _ws(F, case["coeffs"])      # keep: the array r points into, alive across the call
        return fn(P("a"), ptrs, case["num"], r, P("b"), P("c"), case["n"], _vp(d_outs[0]))
    if op in ("lincomb", "lincomb_affine"):
        ptrs = (_vp * case["num"])(*[d["m%d" % i] for i in range(case["num"])])
        keep, c = _ws(F, case["coeffs"])      # keep: the array c points into, alive across the call
        if op == "lincomb":
            return fn(ptrs, case["num"], c, case["n"], _vp(d_outs[0]))
        return fn(ptrs, case["num"], c, _w(F, case["constant"]), case["n"], _vp(d_outs[0]))
    if op == "rational_combine":
        k = case["num"]
        pn, pd = (_vp * k)(*[d["n%d" % i] for i in range(k)]), (_vp * k)(*[d["d%d" % i] for i in range(k)])
        keep, c = _ws(F, case["coeffs"])      # keep: the array c points into, alive across the call
        return fn(pn, pd, k, c, case["n"], _vp(d_outs[0]), _vp(d_outs[1]))
    if op == "spmv":
        sc = None if case["scale"] is None else _w(F, case["scale"])
        return fn(P("row_ptr"), P("col"), P("coeff"), case["rows"], P("vec"), sc, case["accumulate"], _vp(d_outs[0]))
    if op == "poly_div_vanishing":
        return fn(P("a"), case["n_coeffs"], case["sub_log"], _w(F, case["shift"]), _vp(d_outs[0]))
    if op in ("mul", "sub"):
        return fn(P("a"), P("b"), _vp(d_outs[0]), case["n"])
    if op == "inv":
        return fn(P("a"), _vp(d_outs[0]), case["n"])
    if op == "div":
        return fn(P("a") if case["with_num"] else None, P("b"), _vp(d_outs[0]), case["n"])
    if op == "pow_table":
        return fn(_vp(d_outs[0]), case["n"], _w(F, case["base"]), _w(F, case["init"]))
    raise KeyError(op)


def run_case(lib, F, case, inp):
    """[output word arrays] of `case` through lib"""
    dev = _Dev(lib)
    try:
        d = {k: dev.up(v) for k, v in inp.items() if k != "out"}
        n = out_count(case)
        nout = 2 if case["op"] == "rational_combine" else 1
        d_outs = [dev.up(inp["out"]) if case["op"] == "spmv" else dev.empty(n * 8 * F.words) for _ in range(nout)]
        lib._check(call(lib, F, case, d, d_outs))
        return [dev.down(p, n, F.words) for p in d_outs]
    finally:
        dev.close()


def case_digest(outs):
    return digest(np.concatenate([np.ascontiguousarray(o).reshape(-1) for o in outs])) if outs else digest(np.zeros(0, dtype=np.uint64))


def run_tiny(lib, F=BN):
    """{name: digest of the outputs} for every tiny case, the layout of bn128_protocol_tiny.json"""
    return {c["name"]: case_digest(run_case(lib, F, c, inputs(F, c))) for c in tiny_cases(F)}


def model_tiny(F=BN):
    return {c["name"]: case_digest(model_words(F, c, inputs(F, c))) for c in tiny_cases(F)}


def run_large(lib, m, F=BN):
    """yields (name, concatenated output words) for the 2^m recipes"""
    for c in large_cases(F, m):
        outs = run_case(lib, F, c, inputs(F, c))
        yield c["name"], np.concatenate(outs)


def model_large(m, F=BN):
    for c in large_cases(F, m):
        yield c["name"], np.concatenate(model_words(F, c, inputs(F, c)))


# ---- raw data words: r - 1, r, r + 1, 2^256 - 1, 0 ---------------------------------------------------------------------------
RAW_WORDS = [B.P - 1, B.P, B.P + 1, (1 << 256) - 1, 0]


def raw_cases():
    """small cases of every entry with a data operand; the driver plants RAW_WORDS in each operand in turn"""
    F = BN
    cs = lambda k, t: [_scalar(F, "raw %s %d" % (t, i)) for i in range(k)]          # noqa: E731
    return [dict(_domain_case(F, "rowcheck", 5, 2, "seeded"), name="raw_rowcheck"), dict(_domain_case(F, "fz", 5, 2, "seeded"), name="raw_fz"),
            dict(_domain_case(F, "sumcheck_g", 5, 2, "seeded"), name="raw_sumcheck_g"),
            dict(_domain_case(F, "rational_sumcheck_constraint", 5, 2, "seeded"), name="raw_constraint"),
            {"op": "lincheck", "name": "raw_lincheck", "n": 32, "num": 5, "coeffs": cs(5, "r")},
            {"op": "lincomb", "name": "raw_lincomb", "n": 32, "num": 3, "coeffs": cs(3, "c")},
            {"op": "lincomb", "name": "raw_lincomb6", "n": 32, "num": 6, "coeffs": cs(6, "c")},
            {"op": "lincomb_affine", "name": "raw_lincomb_affine", "n": 32, "num": 2, "coeffs": cs(2, "a"), "constant": _scalar(F, "raw constant")},
            {"op": "rational_combine", "name": "raw_rational1", "n": 32, "num": 1, "coeffs": cs(1, "q")},
            {"op": "rational_combine", "name": "raw_rational4", "n": 32, "num": 4, "coeffs": cs(4, "q")},
            {"op": "spmv", "name": "raw_spmv", "rows": 32, "cols": 32, "shape": "mixed", "scale": None, "accumulate": 1},
            # the quotient reads coefficients N = 8 and up only: two passes with the words where every term reaches (8..) and where none
            # does (33..: j + N >= M), and the quotients short enough that no pass runs (M <= N)
            {"op": "poly_div_vanishing", "name": "raw_poly_div", "n_coeffs": 40, "sub_log": 3, "shift": _scalar(F, "raw div shift"), "raw_at": 8},
            {"op": "poly_div_vanishing", "name": "raw_poly_div_tail", "n_coeffs": 40, "sub_log": 3, "shift": _scalar(F, "raw div shift"), "raw_at": 33},
            {"op": "poly_div_vanishing", "name": "raw_poly_div_no_pass", "n_coeffs": 16, "sub_log": 3, "shift": _scalar(F, "raw div shift"), "raw_at": 8},
            {"op": "poly_div_vanishing", "name": "raw_poly_div_short", "n_coeffs": 13, "sub_log": 3, "shift": _scalar(F, "raw div shift"), "raw_at": 8},
            {"op": "mul", "name": "raw_mul", "n": 32}, {"op": "sub", "name": "raw_sub", "n": 32}, {"op": "inv", "name": "raw_inv", "n": 32, "zeros": "none"},
            {"op": "div", "name": "raw_div", "n": 32, "zeros": "none", "with_num": 1}]


def plant_raw(inp, role, at=0):
    """`inp` with RAW_WORDS written over positions at, at + 1, ... of operand `role` (spread over a vector's batch positions)"""
    out = dict(inp)
    a = np.array(inp[role], copy=True)
    assert at + len(RAW_WORDS) <= len(a), "the operand is too short for the raw words"
    a[at:at + len(RAW_WORDS)] = BN.to_words(RAW_WORDS)
    out[role] = a
    return out


def data_roles(inp):
    return [k for k in inp if k not in ("row_ptr", "col")]


def check_raw_words(lib):
    """r - 1, r, r + 1, 2^256 - 1 and 0 in every data operand: canonical results, congruent to the model on the reduced inputs"""
    bad = []
    for c in raw_cases():
        base = inputs(BN, c)
        plain = model_words(BN, c, base)
        for role in data_roles(base):
            inp = plant_raw(base, role, c.get("raw_at", 0))
            got, want = run_case(lib, BN, c, inp), model_words(BN, c, inp)
            # the planted words must be read by the entry: otherwise the case shows nothing about them
            assert any(not np.array_equal(w, q) for w, q in zip(want, plain)), "raw words in %s of %s do not reach the output" % (role, c["name"])
            for g, w in zip(got, want):
                if not np.array_equal(g, w) or any(v >= BN.p for v in BN.to_ints(g)):
                    bad.append((c["name"], role))
    assert not bad, bad
