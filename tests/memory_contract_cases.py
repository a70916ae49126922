"""The memory contract of the device entries, shared by the CPU-emulation suite (tests/test_memory_contract_emu.py) and the GPU suite
(tests/test_gpu_memory_contract.py): what an entry may touch besides the bytes it is asked to produce.

Every row of the table runs under the library's memory-check mode (option IOPX_MEM_CHECK, include/libiop_amd.h): each block the library
allocates is  front guard | payload of exactly the requested bytes | back guard, the payload poisoned, the guards compared when the block is
released.  Around the call, every input sits in a 4096-byte frame of random non-zero bytes and every output in a frame pre-filled with random
bytes (movement_cases.Guarded).  After the call the outputs equal the expected bytes, the frames of every buffer are intact, every input
reads back byte for byte, and the library counted no damaged guard.  Each row runs with the poison bytes 0xA5 and 0x5A and must give the
same bytes both times (an entry that reads a temporary it never wrote follows the poison), and at the payload offsets 0 and 8 modulo 16
(the header promises element alignment, eight bytes, for every entry).

The expected bytes come from `oracle` (by the same calls as gf64_cases, ldt_cases, fold_cases, merkle_cases, poseidon_cases, halves_cases and
dist_blocks_check make) or from the integer model of bn128_protocol_cases.  The gf192 forms that no case module pins by value (fractal_cases
checks them through the library's own products: vanishing polynomials and the division by one, the rational sumcheck's constraint; SpMV, the
linear and rational combinations) are composed from `oracle.gf_mul` / `gf_inv` here.  The prime fields' transforms, folds and LDT combination
use one integer model written over bn128_protocol_cases.Field, which test_memory_contract_emu.py holds against the oracle with edwards_Fr's
parameters.  Never from a second call of the library.

What a guarded, poisoned run cannot show: a read past an input that does not change the result.

`*_dev` methods of Library without a row, and why:
  additive_FFT_dist_dev                      needs a communicator; its kernels are the taylor / pow_table / combine rows
Exported `iopx_*_dev` symbols without a row (every other one is called by a row, directly or through the Library method it names):
  iopx_add_fft_gf192_dist_dev, iopx_add_ifft_gf192_dist_dev                          the sharded transforms: need a communicator (as above)
  iopx_comm_all_gather_dev, iopx_comm_all_reduce_u64_dev, iopx_comm_broadcast_dev,
  iopx_comm_all_to_all_dev, iopx_comm_sendrecv_dev                                   collectives: need a communicator; no kernels of their own beside copies
  iopx_gather_dev, iopx_scatter_dev, iopx_gather_stride_dev, iopx_count_mismatch_dev,
  iopx_interleave_dev, iopx_gather_rows_dev, iopx_memset_dev                         already inside guard frames in layout_cases / movement_cases
"""
import contextlib
import functools

import numpy as np

import bn128_cases as B
import bn128_protocol_cases as PC
import fold_cases
import gf64_cases as G64
import ldt_cases
import merkle_cases
import movement_cases as mv
import oracle
import poseidon_cases as PO
from helpers import rand_elems

import ctypes

_vp, _sz, _u64p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)

FRAME = 4096                    # a wrong stride lands further away than movement_cases.PAD
POISONS = (0xA5, 0x5A)
OFFSETS = (0, 8)                # payload offsets modulo 16
COUNTS = (1, 255, 256, 257)     # element-wise and per-position kernels: below, at and above one workgroup
W = 3


# ---- B1: the mode around a block of test code --------------------------------------------------------------------------------------
@contextlib.contextmanager
def memory_checks(lib, poison=0xA5):
    """The memory-check mode with the given poison byte.  On the way out the options are cleared and the plans and the pool dropped (their
    blocks are checked as they go), even after a failure; a body that ended normally then fails on a damaged guard, with the library's text
    for the first one, and on a run that never reached the allocator."""
    lib.init(0)
    lib.clear_plans()                                   # every block of the body is allocated under the mode
    lib.set_option("IOPX_MEM_CHECK", 1)
    lib.set_option("IOPX_MEM_CHECK_POISON", poison)
    lib.mem_check_stats(reset=True)
    ok = False
    try:
        yield lib
        ok = True
    finally:
        lib.clear_option("IOPX_MEM_CHECK")
        lib.clear_option("IOPX_MEM_CHECK_POISON")
        lib.clear_plans()
        checked, violations, first = lib.mem_check_stats(reset=True)
        if ok:
            assert violations == 0, "%d damaged guards; the first: %s" % (violations, first)
            assert checked > 0, "no guarded block was released: the run never reached the allocator"


# ---- B2: the harness ---------------------------------------------------------------------------------------------------------------
class Case:
    """What a row's builder returns.  inputs: host arrays, uploaded into frames and read back after the call.  outputs: one expected array per
    device output (None: only the frames are checked).  init: {output index: array} for an output whose old contents the entry reads (in
    place, accumulate); every other output starts as random bytes.  call(lib, d_in, d_out) runs the entry; what it returns is compared with
    `returns` (host results) when that is not None."""

    def __init__(self, inputs, outputs, call, init=None, returns=None, out_bytes=None):
        self.inputs = [np.ascontiguousarray(a) for a in inputs]
        self.outputs = [None if o is None else np.ascontiguousarray(o) for o in outputs]
        self.call, self.init, self.returns = call, init or {}, returns
        self.out_bytes = out_bytes or [o.nbytes for o in self.outputs]


class Row:
    def __init__(self, entry, name, build, offsets=OFFSETS):
        self.entry, self.name, self.offsets = entry, name, offsets
        self.build = functools.lru_cache(maxsize=None)(build)       # the reference is computed once and shared by every run of the row


def _frame(lib, nbytes, seed, off):
    g = mv.Guarded(lib, nbytes + 16, seed, pad=FRAME)
    g.image[g.image == 0] = 0x3C                         # non-zero: an entry that relies on zero padding around its input finds none
    g.off = off
    return g


def _read(g, what):
    got = np.empty(g.total, dtype=np.uint8)
    g.lib.d2h(got, g.d)
    bad = np.flatnonzero(got != g.image)
    assert bad.size == 0, "%s: %d bytes differ, the first at byte %d of the payload" % (what, bad.size, bad[0] - FRAME - g.off)
    return got


def _run_once(lib, row, case, off):
    frames_in, frames_out = [], []
    try:
        for k, a in enumerate(case.inputs):
            g = _frame(lib, a.nbytes, 1000 + k, off)
            frames_in.append(g)
            g.expect(off, a.reshape(-1).view(np.uint8))
            g.reset()
        for k, nbytes in enumerate(case.out_bytes):
            g = _frame(lib, nbytes, 2000 + k, off)
            frames_out.append(g)
            if k in case.init:
                g.expect(off, np.ascontiguousarray(case.init[k]).reshape(-1).view(np.uint8))
            g.reset()
        ret = case.call(lib, [g.dst(off) for g in frames_in], [g.dst(off) for g in frames_out])
        lib.synchronize()
        seen = []
        for k, (g, want) in enumerate(zip(frames_out, case.outputs)):
            what = "%s, offset %d: output %d" % (row.name, off, k)
            if want is None:                                # the payload is the entry's to write: frames only
                got = np.empty(g.total, dtype=np.uint8)
                lib.d2h(got, g.d)
                g.expect(off, got[FRAME + off:FRAME + off + case.out_bytes[k]])
            else:
                g.expect(off, want.reshape(-1).view(np.uint8))
            seen.append(_read(g, what)[FRAME + off:FRAME + off + case.out_bytes[k]].tobytes())
        for k, g in enumerate(frames_in):
            _read(g, "%s, offset %d: input %d after the call" % (row.name, off, k))
        if case.returns is not None:
            ret = np.ascontiguousarray(ret)
            assert ret.shape == case.returns.shape and np.array_equal(ret, case.returns), "%s, offset %d: returned values" % (row.name, off)
            seen.append(ret.tobytes())
        return seen
    finally:
        for g in frames_in + frames_out:
            g.free()


def run_row(lib, row):
    case = row.build()
    seen = {}
    for poison in POISONS:
        with memory_checks(lib, poison):
            for off in row.offsets:
                seen.setdefault(off, []).append(_run_once(lib, row, case, off))
    for off, (a, b) in seen.items():
        assert a == b, "%s, offset %d: the bytes follow the poison" % (row.name, off)


def run_group(lib, group):
    for row in GROUPS[group]:
        run_row(lib, row)


# ---- reference pieces ---------------------------------------------------------------------------------------------------------------
def _gf_domain(m, kind="aurora", seed=0):
    return fold_cases.additive_domain(m, kind, 400 + m + seed)


def _rep(v, n):
    return np.repeat(np.asarray(v, dtype=np.uint64).reshape(1, -1), n, axis=0)


def _xor_sum(terms, like):
    acc = np.zeros_like(like)
    for t in terms:
        acc = acc ^ t
    return acc


def _taylor(S):
    """the Taylor-expansion network of dist_blocks_check.check_taylor (fft.tcc:73-83 with j = 0)"""
    ref, n = S.copy(), S.shape[0]
    stride = n // 4
    while stride >= 1:
        for ofs in range(0, n, stride * 4):
            ref[ofs + 2 * stride:ofs + 3 * stride] ^= ref[ofs + 3 * stride:ofs + 4 * stride]
            ref[ofs + stride:ofs + 2 * stride] ^= ref[ofs + 2 * stride:ofs + 3 * stride]
        stride //= 2
    return ref


def _twists(count, index_base, basis, shift_term):
    tw = _rep(shift_term, count)
    for i in range(count):
        for k in range(basis.shape[0]):
            if ((index_base + i) >> k) & 1:
                tw[i] ^= basis[k]
    return tw


def _gf_vanishing(points, sub_basis, sub_shift):
    """Z_S(x) = prod over s in S of (x + s) for every x in points; S = span(sub_basis) + sub_shift"""
    acc = np.zeros_like(points)
    acc[:, 0] = 1
    for s in oracle.all_subset_sums(sub_basis, sub_shift) if sub_basis.shape[0] else np.asarray(sub_shift, dtype=np.uint64).reshape(1, W):
        acc = oracle.gf_mul(acc, points ^ s.reshape(1, W))
    return acc


def _gf1(a, b):
    return oracle.gf_mul(np.asarray(a, dtype=np.uint64).reshape(1, W), np.asarray(b, dtype=np.uint64).reshape(1, W))[0]


def _gf_vanishing_coefficients(sub_basis, sub_shift):
    """{exponent: coefficient} of Z_S, S = span(sub_basis) + sub_shift: the linearized polynomial L of the span, built one basis vector at a
    time by L'(x) = L(x)^2 + L(b) L(x) (linearized_polynomial.tcc), plus the constant L(shift)"""
    lin = [np.array([1, 0, 0], dtype=np.uint64)]            # L(x) = sum_i lin[i] x^(2^i)

    def at(x):
        acc, xp = np.zeros(W, dtype=np.uint64), np.asarray(x, dtype=np.uint64)
        for c in lin:
            acc, xp = acc ^ _gf1(c, xp), _gf1(xp, xp)
        return acc
    for b in sub_basis:
        lb = at(b)
        sq = [np.zeros(W, dtype=np.uint64)] + [_gf1(c, c) for c in lin]
        lin = [sq[i] ^ (_gf1(lb, lin[i]) if i < len(lin) else 0) for i in range(len(sq))]
    out = {1 << i: c for i, c in enumerate(lin)}
    out[0] = at(sub_shift)
    return out


def _gf_poly_div_vanishing(poly, sub_basis, sub_shift):
    """the quotient of poly (coefficients, lowest first) by Z_S: schoolbook long division, Z_S monic of degree |S|"""
    z, N = _gf_vanishing_coefficients(sub_basis, sub_shift), 1 << len(sub_basis)
    cur, n = poly.copy(), poly.shape[0]
    q = np.zeros((max(n - N, 0), W), dtype=np.uint64)
    for j in range(n - 1, N - 1, -1):
        q[j - N] = cur[j]
        for e, c in z.items():
            if e != N:
                cur[j - N + e] ^= _gf1(q[j - N], c)
    return q


# ---- the integer model of the prime fields' transforms (PC.Field: edwards_Fr and alt_bn128 Fr) ------------------------------------------
def int_fft(F, values, log_n, shift):
    """[P(shift g^j)] for P's coefficient residues `values` (at most 2^log_n of them), g = F.gen(log_n); an iterative radix-2 transform"""
    n, p = 1 << log_n, F.p
    a = [(v * pow(shift, i, p)) % p for i, v in enumerate(values)] + [0] * (n - len(values))
    return _int_ntt(a, F.gen(log_n), p)


def _int_ntt(a, g, p):
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = _int_ntt(a[0::2], g * g % p, p), _int_ntt(a[1::2], g * g % p, p)
    out, w = [0] * n, 1
    for k in range(n // 2):
        t = w * odd[k] % p
        out[k], out[k + n // 2] = (even[k] + t) % p, (even[k] - t) % p
        w = w * g % p
    return out


def int_ifft(F, evals, log_n, shift):
    n, p = 1 << log_n, F.p
    c = _int_ntt(list(evals), pow(F.gen(log_n), p - 2, p), p)
    ninv, sinv = pow(n, p - 2, p), pow(shift, p - 2, p)
    return [v * ninv % p * pow(sinv, i, p) % p for i, v in enumerate(c)]


def int_fold(F, f, log_n, shift, coset_size, x):
    """multiplicative_evaluate_next_f_i_over_entire_domain (fri_aux.tcc:105-249): the interpolant of f on each coset of order coset_size, at x.
    Position j of the result belongs to the coset {shift g^(j + k n / coset_size)}; x off the domain."""
    n, p, g = 1 << log_n, F.p, F.gen(log_n)
    m = n // coset_size
    out = []
    for j in range(m):
        xs = [shift * pow(g, j + k * m, p) % p for k in range(coset_size)]
        ys = [f[j + k * m] for k in range(coset_size)]
        acc = 0
        for i, (xi, yi) in enumerate(zip(xs, ys)):
            num, den = 1, 1
            for q, xq in enumerate(xs):
                if q != i:
                    num, den = num * (x - xq) % p, den * (xi - xq) % p
            acc = (acc + yi * num % p * pow(den, p - 2, p)) % p
        out.append(acc)
    return out


def int_ldt(F, evals, degrees, coeffs, log_n, shift):
    """combined_LDT_virtual_oracle::evaluated_contents (ldt_reducer_aux.tcc:39-131) over residues: sum_k (c_k + c'_k x^(max - deg_k)) f_k(x)
    with c = [1] + coeffs (:26-37), the second coefficient only for the oracles below the maximal degree, taken in their order from c[k..]"""
    n, p, mx, k = 1 << log_n, F.p, max(degrees), len(degrees)
    coeffs = [1] + list(coeffs)
    xs = PC._points(F, log_n, shift, range(n))
    out, sub = [0] * n, 0
    for i, d in enumerate(degrees):
        if d < mx:
            bump = coeffs[k + sub]
            sub += 1
            out = [(o + (coeffs[i] + bump * pow(x, mx - d, p)) * f) % p for o, x, f in zip(out, xs, evals[i])]
        else:
            out = [(o + coeffs[i] * f) % p for o, f in zip(out, evals[i])]
    return out


def _res(F, words):
    return [F.dec(w) for w in F.to_ints(words)]


def _enc_words(F, residues):
    return F.to_words([F.enc(v) for v in residues])


_PRIME = {"fp3": PC.ED, "bn128": PC.BN}
_FP3_METHODS = {"rowcheck": "rowcheck_multiplicative_dev", "fz": "fz_multiplicative_dev", "sumcheck_g": "sumcheck_g_multiplicative_dev",
                "poly_div_vanishing": "poly_div_vanishing_multiplicative_dev", "mul": "fp3_mul_dev", "sub": "fp3_sub_dev", "pow_table": "fp3_pow_table_dev",
                "domain_offsets": "domain_offsets_multiplicative_dev", "vanishing_evals": "vanishing_evals_multiplicative_dev",
                "rational_sumcheck_constraint": "rational_sumcheck_constraint_multiplicative_dev", "inv": "field_inv_dev (prime_field)", "div": "field_div_dev (prime_field)"}
# the Library method behind each of bn128_protocol_cases' C symbols (the rows call the symbol, as that module does)
_PRIME_METHODS = {"fp3": lambda op: _FP3_METHODS.get(op, "%s_dev (prime_field)" % op), "bn128": lambda op: "bn128_%s_dev" % op}


def _prime_call(lib, tag, stem, *args):
    lib._check(getattr(lib.c, "iopx_%s_%s_dev" % (stem, tag))(*args))


# ---- rows: transforms ---------------------------------------------------------------------------------------------------------------
def _u(a):
    return np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(_u64p)


def _gf192_fft_rows(d):
    rows = []
    for kind in ("aurora", "general"):
        basis, shift = _gf_domain(d, kind)
        for count in sorted({1 << d, (1 << d) // 2 + 1}):
            def build(basis=basis, shift=shift, count=count):
                coeffs = rand_elems(50 + d + count, count, W)
                return Case([coeffs], [oracle.additive_fft(coeffs, basis, shift)],
                            lambda lib, i, o: lib.additive_FFT_dev(i[0], count, basis, shift, o[0]))
            rows.append(Row("additive_FFT_dev", "gf192 FFT d=%d %s count=%d" % (d, kind, count), build))

        def build_inv(basis=basis, shift=shift):
            evals = rand_elems(60 + d, 1 << d, W)
            return Case([evals], [oracle.additive_ifft(evals, basis, shift)], lambda lib, i, o: lib.additive_IFFT_dev(i[0], basis, shift, o[0]))
        rows.append(Row("additive_IFFT_dev", "gf192 IFFT d=%d %s" % (d, kind), build_inv))
    return rows


def _gf192_lde_rows(m=10, d=6, begin=3, count=5, kind="aurora", batches=(1, 3), forms=True):
    """Coset ranges with coset_begin != 0 and a count that is no power of two, and the batch and re-extension forms, of 2^d coefficients over
    2^m points.  d = 6: one edge pass per coset; d = 10: one whole tile per coset (k_bfly_edge_multi); d >= 11: upper passes into the staging
    buffer of a coset group, and for batches of 2 - 4 the batched last pass (k_bfly_edge_fwd_batch) with its combined shift terms."""
    rows = []
    basis, shift = _gf_domain(m, kind)
    tag = "m=%d d=%d %s cosets %d..%d" % (m, d, kind, begin, begin + count - 1)

    def build():
        coeffs = rand_elems(70, (1 << d) - 3, W)
        full = oracle.additive_fft(coeffs, basis, shift)
        return Case([coeffs], [full[begin << d:(begin + count) << d]],
                    lambda lib, i, o: lib.additive_LDE_dev(i[0], coeffs.shape[0], basis, shift, begin, count, o[0]))
    rows.append(Row("additive_LDE_dev", "gf192 LDE " + tag, build))
    for batch in batches:
        def build_lde(batch=batch):
            cs = [rand_elems(71 + k, 1 << d, W) for k in range(batch)]
            outs = [oracle.additive_fft(c, basis, shift)[begin << d:(begin + count) << d] for c in cs]
            return Case(cs, outs, lambda lib, i, o: lib.additive_LDE_batch_dev(i, 1 << d, basis, shift, begin, count, o))
        rows.append(Row("additive_LDE_batch_dev", "gf192 LDE batch of %d, %s" % (batch, tag), build_lde))

        def build_ifft(batch=batch):
            hb, hs = basis[:d], rand_elems(75, 1, W)[0]
            ev = [rand_elems(76 + k, 1 << d, W) for k in range(batch)]
            return Case([np.concatenate(ev)], [np.concatenate([oracle.additive_ifft(e, hb, hs) for e in ev])],
                        lambda lib, i, o: lib.additive_IFFT_batch_dev(i[0], batch, hb, hs, o[0]))
        rows.append(Row("additive_IFFT_batch_dev", "gf192 IFFT batch of %d, %s" % (batch, tag), build_ifft))

        def build_re(batch=batch):
            es = rand_elems(80, 1, W)[0]
            ev = [rand_elems(81 + k, 1 << d, W) for k in range(batch)]
            outs = [oracle.additive_fft(oracle.additive_ifft(e, basis[:d], es), basis, shift)[begin << d:(begin + count) << d] for e in ev]
            return Case([np.concatenate(ev)], outs,
                        lambda lib, i, o: lib.additive_reextend_batch_dev(i[0], batch, basis, d, es, shift, begin, count, o))
        rows.append(Row("additive_reextend_batch_dev", "gf192 re-extension batch of %d, %s" % (batch, tag), build_re))

    if not forms:
        return rows

    def build_re2():
        ea, eb = rand_elems(85, 1, W)[0], rand_elems(86, 1, W)[0]
        va, vb = [rand_elems(87 + k, 1 << d, W) for k in range(2)], [rand_elems(90, 1 << d, W)]
        cw = lambda e, s: oracle.additive_fft(oracle.additive_ifft(e, basis[:d], s), basis, shift)[begin << d:(begin + count) << d]   # noqa: E731
        return Case([np.concatenate(va), np.concatenate(vb)], [cw(e, ea) for e in va] + [cw(e, eb) for e in vb],
                    lambda lib, i, o: lib.additive_reextend2_batch_dev(i[0], 2, ea, i[1], 1, eb, basis, d, shift, begin, count, o))
    rows.append(Row("additive_reextend2_batch_dev", "gf192 re-extension of two groups, " + tag, build_re2))

    def build_re_lde():
        es = rand_elems(91, 1, W)[0]
        ev, cs = [rand_elems(92 + k, 1 << d, W) for k in range(2)], [rand_elems(95, (1 << d) - 5, W)]
        sl = slice(begin << d, (begin + count) << d)
        outs = [oracle.additive_fft(oracle.additive_ifft(e, basis[:d], es), basis, shift)[sl] for e in ev] + [oracle.additive_fft(c, basis, shift)[sl] for c in cs]
        return Case([np.concatenate(ev)] + cs, outs,
                    lambda lib, i, o: lib.additive_reextend_lde_batch_dev(i[0], 2, i[1:], cs[0].shape[0], basis, d, es, shift, begin, count, o))
    rows.append(Row("additive_reextend_lde_batch_dev", "gf192 re-extension with a codeword, " + tag, build_re_lde))
    return rows


def _gf192_block_rows():
    rows = []
    for log_n in (2, 8, 9):
        def build(log_n=log_n):
            n = 1 << log_n
            S, tw = rand_elems(100 + log_n, n, W), rand_elems(101 + log_n, n, W)
            return Case([tw], [_taylor(oracle.gf_mul(S, tw))], lambda lib, i, o: lib.taylor_dev(o[0], log_n, i[0]), init={0: S})
        rows.append(Row("taylor_dev", "gf192 taylor 2^%d with twist" % log_n, build))

        def build_inv(log_n=log_n):
            S = rand_elems(102 + log_n, 1 << log_n, W)
            return Case([], [S], lambda lib, i, o: lib.taylor_inv_dev(o[0], log_n, 0), init={0: _taylor(S)})
        rows.append(Row("taylor_inv_dev", "gf192 taylor_inv 2^%d" % log_n, build_inv))
    for count in COUNTS:
        nb, index_base = 13, 4096
        for upper in (0, 1):
            def build_c(count=count, upper=upper):
                a, b = rand_elems(5, count, W), rand_elems(6, count, W)
                Bs, sh = rand_elems(7, nb, W), rand_elems(8, 1, W)[0]
                lower = a ^ oracle.gf_mul(b, _twists(count, index_base, Bs, sh))
                return Case([a, b], [lower ^ b if upper else lower], lambda lib, i, o: lib.combine_dev(i[0], i[1], o[0], count, index_base, Bs, sh, upper))
            rows.append(Row("combine_dev", "gf192 combine count=%d upper=%d" % (count, upper), build_c))

            def build_ci(count=count, upper=upper):
                a, b = rand_elems(9, count, W), rand_elems(10, count, W)
                Bs, sh = rand_elems(7, nb, W), rand_elems(8, 1, W)[0]
                lo = a ^ oracle.gf_mul(b, _twists(count, index_base, Bs, sh))
                return Case([lo, lo ^ b], [b if upper else a], lambda lib, i, o: lib.combine_inv_dev(i[0], i[1], o[0], count, index_base, Bs, sh, upper))
            rows.append(Row("combine_inv_dev", "gf192 combine_inv count=%d upper=%d" % (count, upper), build_ci))

        def build_p(count=count):
            base, init = rand_elems(1, 1, W), rand_elems(2, 1, W)
            out, cur = np.empty((count, W), dtype=np.uint64), init
            for l in range(count):
                out[l] = cur[0]
                cur = oracle.gf_mul(cur, base)
            return Case([], [out], lambda lib, i, o: lib.pow_table_dev(o[0], count, base[0], init[0]))
        rows.append(Row("pow_table_dev", "gf192 pow_table count=%d" % count, build_p))
    return rows


def _gf64_rows(d):
    rows = []
    basis, shift = G64.std_basis(d), G64.elem((1 << 63) | 0x55)
    for count in sorted({1 << d, (1 << d) // 2 + 1}):
        def build(count=count):
            coeffs = G64.seeded("mc fft %d %d" % (d, count), count)
            return Case([coeffs], [oracle.additive_fft(coeffs, basis, shift)], lambda lib, i, o: lib.additive_FFT_gf64_dev(i[0], count, basis, shift, o[0]))
        rows.append(Row("additive_FFT_gf64_dev", "gf64 FFT d=%d count=%d" % (d, count), build))

    def build_inv():
        evals = G64.seeded("mc ifft %d" % d, 1 << d)
        return Case([evals], [oracle.additive_ifft(evals, basis, shift)], lambda lib, i, o: lib.additive_IFFT_gf64_dev(i[0], basis, shift, o[0]))
    rows.append(Row("additive_IFFT_gf64_dev", "gf64 IFFT d=%d" % d, build_inv))

    def build_inplace():
        evals = G64.seeded("mc ifft in place %d" % d, 1 << d)
        return Case([], [oracle.additive_ifft(evals, basis, shift)], lambda lib, i, o: lib.additive_IFFT_gf64_dev(o[0], basis, shift, o[0]), init={0: evals})
    rows.append(Row("additive_IFFT_gf64_dev", "gf64 IFFT d=%d in place" % d, build_inplace))
    return rows


def _c_symbol_rows():
    """device entries that Library reaches only inside host-array methods, through their C symbols"""
    rows = []
    for count in COUNTS:
        def build_uni(count=count):
            a, c = rand_elems(840, count, W), rand_elems(841, 1, W)
            return Case([a, c], [oracle.gf_mul(a, _rep(c[0], count))],
                        lambda lib, i, o: lib._check(lib.c.iopx_gf192_mul_uniform_dev(_vp(i[0]), _vp(i[1]), _vp(o[0]), _sz(count))))
        rows.append(Row("iopx_gf192_mul_uniform_dev", "gf192 mul_uniform count=%d" % count, build_uni))
    for m in (2, 8, 9):
        def build_dv(m=m):
            basis, shift = oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)      # the domain does not meet S
            sub, zero = 2, np.zeros(W, dtype=np.uint64)
            v = rand_elems(842, 1 << m, W)
            xs = oracle.all_subset_sums(basis, shift)
            want = oracle.gf_mul(v, oracle.gf_inv(_gf_vanishing(xs, basis[:sub], zero)))
            lib_args = lambda lib, i, o: lib._check(lib.c.iopx_div_by_vanishing_gf192_dev(_vp(i[0]), _u(basis), _sz(m), _u(shift), _sz(sub), _u(zero), _vp(o[0])))   # noqa: E731
            return Case([v], [want], lib_args)
        rows.append(Row("iopx_div_by_vanishing_gf192_dev", "gf192 div_by_vanishing m=%d" % m, build_dv))
    for tag in ("fp3", "bn128"):
        F = _PRIME[tag]
        for log_n, degree in ((3, 1), (8, 17), (8, 64), (9, 257)):
            def build_kd(F=F, tag=tag, log_n=log_n, degree=degree):
                k = max(degree - 1, 0).bit_length()
                shift = PC._scalar(F, "mc known degree shift")
                evals = F.data("mc known degree %d" % log_n, 1 << log_n)
                want = _enc_words(F, int_ifft(F, _res(F, evals[::1 << (log_n - k)]), k, shift))
                gen_w, shift_w = F.elem(F.gen(log_n)), F.elem(shift)
                return Case([evals], [want], lambda lib, i, o: _prime_call(lib, tag, "mul_ifft_known_degree", _vp(i[0]), _sz(degree), _sz(log_n), _u(gen_w), _u(shift_w), _vp(o[0])))
            rows.append(Row("iopx_mul_ifft_known_degree_%s_dev" % tag, "%s IFFT of known degree %d over 2^%d" % (tag, degree, log_n), build_kd))
    return rows


def _gf64_other_rows():
    rows = []
    m, d = 12, 7
    basis, shift = G64.std_basis(m), G64.elem((1 << 63) | 0x55)

    def build_lde():
        coeffs = G64.seeded("mc lde", (1 << d) - 3)
        return Case([coeffs], [oracle.additive_fft(coeffs, basis, shift)[5 << d:8 << d]],
                    lambda lib, i, o: lib.additive_LDE_gf64_dev(i[0], coeffs.shape[0], basis, shift, 5, 3, o[0]))
    rows.append(Row("additive_LDE_gf64_dev", "gf64 LDE m=12 d=7 cosets 5..7", build_lde))
    # the smallest coefficient dimension whose plan has an upper pass (4096-element tiles): 13, with 3 cosets through run_phase2_fwd_x's staging
    b15, s15 = G64.std_basis(15), G64.elem((1 << 63) | 3)

    def build_staged():
        coeffs = G64.seeded("mc staged", (1 << 12) + 1)
        return Case([coeffs], [oracle.additive_fft(coeffs, b15, s15)[1 << 13:4 << 13]],
                    lambda lib, i, o: lib.additive_LDE_gf64_dev(i[0], coeffs.shape[0], b15, s15, 1, 3, o[0]))
    rows.append(Row("additive_LDE_gf64_dev", "gf64 LDE m=15 d=13 cosets 1..3 (staged)", build_staged))
    fb, fs = G64.std_basis(10), G64.elem((1 << 63) | 0x77)
    for eta in (1, 3, 5):
        def build_fold(eta=eta):
            f, x = G64.seeded("mc fold %d" % eta, 1 << 10), G64.elem(int(G64.seeded("mc fold x", 1)[0, 0]))
            return Case([f], [oracle.fri_fold_additive(f, fb, fs, 1 << eta, x)],
                        lambda lib, i, o: lib.evaluate_next_f_i_over_entire_domain_gf64_dev(i[0], fb, fs, 1 << eta, x, o[0]))
        rows.append(Row("evaluate_next_f_i_over_entire_domain_gf64_dev", "gf64 fold 2^10 by 2^%d" % eta, build_fold))
    for name, degrees in (("one", [256]), ("mixed", [256, 255, 128, 129, 256])):
        def build_ldt(degrees=degrees, name=name):
            lb, ls = G64.std_basis(8), G64.elem((1 << 63) | 0xF0F)
            evals = [G64.seeded("mc ldt %s %d" % (name, k), 256) for k in range(len(degrees))]
            coef = G64.seeded("mc ldt coef " + name, 2 * len(degrees))
            return Case(evals, [oracle.ldt_combine_additive(evals, degrees, coef, lb, ls)], lambda lib, i, o: lib.ldt_combine_gf64_dev(i, degrees, coef, lb, ls, o[0]))
        rows.append(Row("ldt_combine_gf64_dev", "gf64 ldt_combine %s" % name, build_ldt))
    for count in COUNTS:
        def build_mul(count=count):
            a, b = G64.seeded("mc mul a", count), G64.seeded("mc mul b", count)
            return Case([a, b], [oracle.gf_mul(a, b)], lambda lib, i, o: lib.gf64_mul_dev(i[0], i[1], o[0], count))
        rows.append(Row("gf64_mul_dev", "gf64 mul count=%d" % count, build_mul))

        def build_inv(count=count):
            a = G64.seeded("mc inv", count) | np.uint64(1)
            return Case([a], [oracle.gf_inv(a)], lambda lib, i, o: lib.gf64_inv_dev(i[0], o[0], count))
        rows.append(Row("gf64_inv_dev", "gf64 inv count=%d" % count, build_inv))
    return rows


def _prime_fft_rows(tag, log_n):
    F = _PRIME[tag]
    rows = []
    shift = F.generator
    n = 1 << log_n
    gen_w, shift_w = F.elem(F.gen(log_n)), F.elem(shift)
    for count in sorted({n, n // 2 + 1}):
        def build(count=count):
            coeffs = F.data("mc fft %d" % log_n, n)[:count]
            want = _enc_words(F, int_fft(F, _res(F, coeffs), log_n, shift))
            return Case([coeffs], [want], lambda lib, i, o: _prime_call(lib, tag, "mul_fft", _vp(i[0]), _sz(count), _sz(log_n), _u(gen_w), _u(shift_w), _vp(o[0])))
        rows.append(Row("iopx_mul_fft_%s_dev" % tag, "%s FFT log_n=%d count=%d" % (tag, log_n, count), build))

    def build_inv():
        evals = F.data("mc ifft %d" % log_n, n)
        want = _enc_words(F, int_ifft(F, _res(F, evals), log_n, shift))
        return Case([evals], [want], lambda lib, i, o: _prime_call(lib, tag, "mul_ifft", _vp(i[0]), _sz(log_n), _u(gen_w), _u(shift_w), _vp(o[0])))
    rows.append(Row("iopx_mul_ifft_%s_dev" % tag, "%s IFFT log_n=%d" % (tag, log_n), build_inv))
    if log_n in (4, 12):                                # the windowed transform at a one-pass and a two-pass size

        def build_win():
            coeffs = F.data("mc fft windows %d" % log_n, n)[:n // 4 + 1]
            out = _enc_words(F, int_fft(F, _res(F, coeffs), log_n, shift))
            wins = [(1, 2), (0, log_n - 2)]
            method = "multiplicative_FFT_windows_dev" if tag == "fp3" else "multiplicative_FFT_windows_bn128_dev"
            return Case([coeffs], [out] + [out[f::1 << ls] for f, ls in wins],
                        lambda lib, i, o: getattr(lib, method)(i[0], coeffs.shape[0], log_n, shift_w, o[0], [(f, ls, d) for (f, ls), d in zip(wins, o[1:])], gen=gen_w))
        rows.append(Row("multiplicative_FFT_windows_dev" if tag == "fp3" else "multiplicative_FFT_windows_bn128_dev", "%s windowed FFT log_n=%d" % (tag, log_n), build_win))
    return rows


def _prime_big_fft_row(tag):
    """The three-pass size 2^19: Horner evaluations at 64 sampled positions; the frames, the inputs and the two-poison equality cover the whole buffer.
    1000 coefficients (the rest of the 2^19 are the transform's zero padding), so that the Horner references stay cheap."""
    F, log_n, count = _PRIME[tag], 19, 1000
    shift = F.generator
    gen_w, shift_w = F.elem(F.gen(log_n)), F.elem(shift)
    coeffs = F.data("mc fft 19", count)
    pos = sorted(set([0, 1, (1 << 19) - 1, 1 << 18] + [int(v) for v in np.random.default_rng(19).integers(0, 1 << 19, size=60)]))
    cres = _res(F, coeffs)
    want = {}
    for j in pos:
        x, acc = shift * pow(F.gen(log_n), j, F.p) % F.p, 0
        for c in reversed(cres):
            acc = (acc * x + c) % F.p
        want[j] = F.to_words([F.enc(acc)])[0]
    return coeffs, count, log_n, gen_w, shift_w, want


def check_three_pass_fft(lib, tag):
    F = _PRIME[tag]
    coeffs, count, log_n, gen_w, shift_w, want = _prime_big_fft_row(tag)
    nbytes = (8 * F.words) << log_n
    digests = []
    for poison in POISONS:
        with memory_checks(lib, poison):
            gi, go = _frame(lib, coeffs.nbytes, 1, 0), _frame(lib, nbytes, 2 + poison, 0)      # another prefill per poison: an element nobody writes differs between the runs
            try:
                gi.expect(0, coeffs.reshape(-1).view(np.uint8))
                gi.reset()
                go.reset()
                _prime_call(lib, tag, "mul_fft", _vp(gi.dst(0)), _sz(count), _sz(log_n), _u(gen_w), _u(shift_w), _vp(go.dst(0)))
                lib.synchronize()
                got = np.empty(go.total, dtype=np.uint8)
                lib.d2h(got, go.d)
                out = got[FRAME:FRAME + nbytes].view(np.uint64).reshape(-1, F.words)
                for j, w in want.items():
                    assert np.array_equal(out[j], w), (tag, j)
                go.expect(0, got[FRAME:FRAME + nbytes])
                assert np.array_equal(got, go.image), "%s 2^19: the output's frame" % tag
                _read(gi, "%s 2^19: input after the call" % tag)
                digests.append(B.digest(out))
            finally:
                gi.free()
                go.free()
    assert digests[0] == digests[1], "%s 2^19: the bytes follow the poison" % tag


def _prime_fold_ldt_rows(tag):
    F = _PRIME[tag]
    rows = []
    log_n, shift = 8, F.generator
    gen_w, shift_w = F.elem(F.gen(log_n)), F.elem(shift)
    for eta in (1, 2, 3, 4):                            # fused up to eta = 3, the unfused chain above
        def build(eta=eta):
            f, x = F.data("mc fold %d" % eta, 1 << log_n), PC._scalar(F, "mc fold x")
            want = _enc_words(F, int_fold(F, _res(F, f), log_n, shift, 1 << eta, x))
            return Case([f], [want], lambda lib, i, o: _prime_call(lib, tag, "fri_fold_mul", _vp(i[0]), _sz(log_n), _u(gen_w), _u(shift_w), _sz(1 << eta),
                                                                  _u(F.elem(x)), _vp(o[0])))
        rows.append(Row("iopx_fri_fold_mul_%s_dev" % tag, "%s fold 2^8 by 2^%d" % (tag, eta), build))
    for name, degrees in (("one", [256]), ("mixed", [256, 255, 100, 37, 256])):
        def build_ldt(degrees=degrees, name=name):
            evals = [F.data("mc ldt %s %d" % (name, k), 1 << log_n) for k in range(len(degrees))]
            cs = [PC._scalar(F, "mc ldt c %d" % k) for k in range(2 * len(degrees))]
            want = _enc_words(F, int_ldt(F, [_res(F, e) for e in evals], degrees, cs, log_n, shift))
            cw = F.to_words([F.enc(c) for c in cs])
            if tag == "fp3":
                return Case(evals, [want], lambda lib, i, o: lib.ldt_combine_multiplicative_dev(i, degrees, cw, log_n, gen_w, shift_w, o[0]))
            return Case(evals, [want], lambda lib, i, o: lib.ldt_combine_bn128_dev(i, degrees, cw, log_n, shift_w, o[0], gen=gen_w))
        rows.append(Row("ldt_combine_multiplicative_dev" if tag == "fp3" else "ldt_combine_bn128_dev", "%s ldt_combine %s" % (tag, name), build_ldt))
    return rows


# ---- rows: folds and LDT over gf192 ----------------------------------------------------------------------------------------------------
def _gf192_fold_ldt_rows():
    rows = []
    for m, cs, kind in ((8, 2, "aurora"), (8, 4, "general"), (8, 8, "aurora"), (8, 16, "general"), (8, 256, "aurora")):     # fused up to 8, unfused above
        def build(m=m, cs=cs, kind=kind):
            basis, shift = _gf_domain(m, kind)
            f, x = rand_elems(500 + m + cs, 1 << m, W), rand_elems(600 + m, 1, W)[0]
            return Case([f], [oracle.fri_fold_additive(f, basis, shift, cs, x)], lambda lib, i, o: lib.fri_fold_dev(i[0], basis, shift, cs, x, o[0]))
        rows.append(Row("fri_fold_dev", "gf192 fold 2^%d by %d (%s)" % (m, cs, kind), build))
    for m, degrees, seed, kind in ldt_cases.ADDITIVE[:3] + [ldt_cases.ADDITIVE[6], ldt_cases.ADDITIVE[7], ldt_cases.GAP1[0]]:
        def build_ldt(m=m, degrees=degrees, seed=seed, kind=kind):
            n = 1 << m
            basis, shift = (oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)) if kind == "standard" else \
                           (rand_elems(seed + 1, m, W), rand_elems(seed + 2, 1, W)[0])
            evals = [rand_elems(seed + 10 + k, n, W) for k in range(len(degrees))]
            coeffs = rand_elems(seed + 3, 2 * len(degrees), W)
            return Case(evals, [oracle.ldt_combine_additive(evals, degrees, coeffs, basis, shift)], lambda lib, i, o: lib.ldt_combine_dev(i, degrees, coeffs, basis, shift, o[0]))
        rows.append(Row("ldt_combine_dev", "gf192 ldt_combine m=%d %d oracles (%s)" % (m, len(degrees), kind), build_ldt))
    return rows


# ---- rows: the protocol layer ----------------------------------------------------------------------------------------------------------
def _gf192_protocol_rows():
    rows = []
    for m in (0, 8, 9):
        n = 1 << m
        basis, shift = oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)
        zero = np.zeros(W, dtype=np.uint64)
        h = max(m - 2, 0)
        hb = oracle.standard_basis(h, W) if h else np.zeros((0, W), dtype=np.uint64)

        def build_row(n=n, basis=basis, shift=shift, h=h):
            az, bz, cz = (rand_elems(700 + k, n, W) for k in range(3))
            return Case([az, bz, cz], [oracle.rowcheck_additive(az, bz, cz, basis, shift, h, zero)],
                        lambda lib, i, o: lib.rowcheck_dev(i[0], i[1], i[2], basis, shift, h, zero, o[0]))
        rows.append(Row("rowcheck_dev", "gf192 rowcheck m=%d" % m, build_row))

        def build_fz(n=n, basis=basis, shift=shift, hb=hb):
            fw, f1v = rand_elems(705, n, W), rand_elems(706, n, W)
            return Case([fw, f1v], [oracle.fz_additive(fw, f1v, basis, shift, hb, zero)], lambda lib, i, o: lib.fz_dev(i[0], i[1], basis, shift, hb, zero, o[0]))
        rows.append(Row("fz_dev", "gf192 fz m=%d" % m, build_fz))
        for mu_kind in ("zero", "random"):
            def build_g(n=n, basis=basis, shift=shift, hb=hb, mu_kind=mu_kind):
                f, hh = rand_elems(707, n, W), rand_elems(708, n, W)
                mu = zero if mu_kind == "zero" else rand_elems(709, 1, W)[0]
                return Case([f, hh], [oracle.sumcheck_g_additive(f, hh, basis, shift, hb, zero, mu)],
                            lambda lib, i, o: lib.sumcheck_g_dev(i[0], i[1], basis, shift, hb, zero, mu, o[0]))
            rows.append(Row("sumcheck_g_dev", "gf192 sumcheck_g m=%d mu %s" % (m, mu_kind), build_g))

        def build_off(n=n, basis=basis, shift=shift):
            point = rand_elems(710, 1, W)[0]
            xs = oracle.all_subset_sums(basis, shift) if basis.shape[0] else shift.reshape(1, W)
            return Case([], [xs ^ point.reshape(1, W)], lambda lib, i, o: lib.domain_offsets_dev(basis, shift, point, o[0]))
        rows.append(Row("domain_offsets_dev", "gf192 domain_offsets m=%d" % m, build_off))

        def build_van(n=n, basis=basis, shift=shift):
            c0 = rand_elems(711, 1, W)[0]
            vb, vs = rand_elems(712, min(2, basis.shape[0]), W), rand_elems(713, 1, W)[0]
            xs = oracle.all_subset_sums(basis, shift) if basis.shape[0] else shift.reshape(1, W)
            return Case([], [_gf_vanishing(xs, vb, vs) ^ c0.reshape(1, W)], lambda lib, i, o: lib.vanishing_evals_dev(basis, shift, vb, vs, c0, o[0]))
        rows.append(Row("vanishing_evals_dev", "gf192 vanishing_evals m=%d" % m, build_van))
        def build_rsc(n=n, basis=basis, shift=shift, m=m):
            # (D (p + eps^-1 mu x^(|K| - 1)) - N) / Z_K over the codeword domain, eps the linear coefficient of Z_K (rational_sumcheck.tcc:58-112)
            kd = min(2, m)
            ks, mu = rand_elems(714, 1, W)[0], rand_elems(715, 1, W)[0]
            pp, N, D = (rand_elems(716 + k, n, W) for k in range(3))
            xs = oracle.all_subset_sums(basis, shift) if m else shift.reshape(1, W)
            xinv = oracle.gf_inv(xs)
            xk = xs.copy()
            for _ in range(kd):
                xk = oracle.gf_mul(xk, xk)                  # x^|K|
            eps_inv = oracle.gf_inv(_gf_vanishing_coefficients(basis[:kd], ks)[1].reshape(1, W))[0]
            bump = oracle.gf_mul(oracle.gf_mul(xk, xinv), _rep(_gf1(eps_inv, mu), n))
            want = oracle.gf_mul(oracle.gf_mul(D, pp ^ bump) ^ N, oracle.gf_inv(_gf_vanishing(xs, basis[:kd], ks)))
            return Case([pp, N, D, xinv], [want], lambda lib, i, o: lib.rational_sumcheck_constraint_dev(i[0], i[1], i[2], i[3], basis, shift, kd, ks, mu, o[0]))
        rows.append(Row("rational_sumcheck_constraint_dev", "gf192 rational_sumcheck_constraint m=%d" % m, build_rsc))
    for n in COUNTS:
        def build_lin(n=n):
            fz, p1, p2 = (rand_elems(720 + k, n, W) for k in range(3))
            mz, r = [rand_elems(730 + k, n, W) for k in range(3)], rand_elems(723, 3, W)
            return Case([fz, p1, p2] + mz, [oracle.lincheck_combine(fz, mz, r, p1, p2, False)], lambda lib, i, o: lib.lincheck_dev(i[0], i[3:], r, i[1], i[2], n, o[0]))
        rows.append(Row("lincheck_dev", "gf192 lincheck n=%d" % n, build_lin))

        def build_lc(n=n, affine=False):
            os_, cs, c0 = [rand_elems(740 + k, n, W) for k in range(5)], rand_elems(745, 5, W), rand_elems(746, 1, W)[0]
            want = _xor_sum([oracle.gf_mul(o, _rep(c, n)) for o, c in zip(os_, cs)], os_[0])
            if affine:
                return Case(os_, [want ^ c0.reshape(1, W)], lambda lib, i, o: lib.lincomb_affine_dev(i, cs, c0, n, o[0]))
            return Case(os_, [want], lambda lib, i, o: lib.lincomb_dev(i, cs, n, o[0]))
        rows.append(Row("lincomb_dev", "gf192 lincomb n=%d" % n, build_lc))
        rows.append(Row("lincomb_affine_dev", "gf192 lincomb_affine n=%d" % n, functools.partial(build_lc, affine=True)))

        def build_div(n=n, with_num=True):
            num, den = rand_elems(750, n, W), rand_elems(751, n, W)
            den[n // 2] = 0                                 # a zero denominator gives zero
            inv = oracle.gf_inv(np.where(den.any(axis=1, keepdims=True), den, np.uint64(1)))
            want = oracle.gf_mul(num, inv) if with_num else inv
            want[n // 2] = 0
            if with_num:
                return Case([num, den], [want], lambda lib, i, o: lib.field_div_dev(i[0], i[1], o[0], n))
            return Case([den], [want], lambda lib, i, o: lib.field_div_dev(None, i[0], o[0], n))
        rows.append(Row("field_div_dev", "gf192 div n=%d" % n, build_div))
        rows.append(Row("field_div_dev", "gf192 div n=%d without numerators" % n, functools.partial(build_div, with_num=False)))

        def build_rat(n=n):
            k = 3
            Ns, Ds, cs = [rand_elems(760 + q, n, W) for q in range(k)], [rand_elems(770 + q, n, W) for q in range(k)], rand_elems(780, k, W)
            num, den = np.zeros((n, W), dtype=np.uint64), None
            for q in range(k):
                term = oracle.gf_mul(Ns[q], _rep(cs[q], n))
                for r in range(k):
                    if r != q:
                        term = oracle.gf_mul(term, Ds[r])
                num ^= term
                den = Ds[q] if den is None else oracle.gf_mul(den, Ds[q])
            return Case(Ns + Ds, [num, den], lambda lib, i, o: lib.rational_combine_dev(i[:k], i[k:], cs, n, o[0], o[1]))
        rows.append(Row("rational_combine_dev", "gf192 rational_combine n=%d" % n, build_rat))

        def build_add(n=n):
            a, b = rand_elems(790, n, W), rand_elems(791, n, W)
            return Case([a, b], [a ^ b], lambda lib, i, o: lib.field_add_dev(i[0], i[1], o[0], n))
        rows.append(Row("field_add_dev", "gf192 add n=%d" % n, build_add))

        def build_mul(n=n):
            a, b = rand_elems(792, n, W), rand_elems(793, n, W)
            return Case([a, b], [oracle.gf_mul(a, b)], lambda lib, i, o: lib.gf192_mul_dev(i[0], i[1], o[0], n))
        rows.append(Row("gf192_mul_dev", "gf192 mul n=%d" % n, build_mul))

        def build_inv(n=n):
            a = rand_elems(794, n, W) | np.uint64(1)
            return Case([a], [oracle.gf_inv(a)], lambda lib, i, o: lib.field_inv_dev(i[0], o[0], n))
        rows.append(Row("field_inv_dev", "gf192 inv n=%d" % n, build_inv))
    for nc in (9, 257, 264):
        def build_pdiv(nc=nc):
            poly, sb, ss = rand_elems(810, nc, W), rand_elems(811, 3, W), rand_elems(812, 1, W)[0]
            return Case([poly], [_gf_poly_div_vanishing(poly, sb, ss)], lambda lib, i, o: lib.poly_div_vanishing_dev(i[0], nc, sb, ss, o[0]))
        rows.append(Row("poly_div_vanishing_dev", "gf192 poly_div_vanishing n_coeffs=%d" % nc, build_pdiv))
    for scale, acc in ((False, False), (True, False), (True, True)):
        def build_spmv(scale=scale, acc=acc):
            rows_, cols = 257, 97
            lens = PC.spmv_row_lengths({"rows": rows_, "shape": "mixed"})
            rp = np.zeros(rows_ + 1, dtype=np.uint64)
            rp[1:] = np.cumsum(lens)
            nnz = int(rp[-1])
            col = np.random.default_rng(3).integers(0, cols, size=nnz, dtype=np.uint32)
            coeff, vec, prev, sc = rand_elems(800, nnz, W), rand_elems(801, cols, W), rand_elems(802, rows_, W), rand_elems(803, 1, W)[0]
            prod = oracle.gf_mul(coeff, vec[col])
            want = np.zeros((rows_, W), dtype=np.uint64)
            for r in range(rows_):
                for t in range(int(rp[r]), int(rp[r + 1])):
                    want[r] ^= prod[t]
            if scale:
                want = oracle.gf_mul(want, _rep(sc, rows_))
            if acc:
                want ^= prev
            return Case([rp, col, coeff, vec], [want], lambda lib, i, o: lib.spmv_dev(i[0], i[1], i[2], rows_, i[3], o[0], scale=sc if scale else None, accumulate=acc),
                        init={0: prev} if acc else None)
        rows.append(Row("spmv_dev", "gf192 spmv scale=%d accumulate=%d" % (scale, acc), build_spmv))

    def build_halves():
        n = 64 * 5
        a, c2 = rand_elems(0x4a1, n, W), rand_elems(0x4a2, 2, W)
        lane_mask = 0x21
        idx = np.arange(n, dtype=np.uint64)
        taken, low = (idx & np.uint64(lane_mask)) != 0, (idx % 64) < 32
        want = a.copy()
        for sel, c in ((taken & low, c2[0:1]), (taken & ~low, c2[1:2])):
            want[sel] = oracle.gf_mul(a[sel], np.repeat(c, int(sel.sum()), axis=0))
        return Case([a, c2], [want, None], lambda lib, i, o: lib.gf192_mul_halves_dev(i[0], i[1], o[0], o[1], n, lane_mask), out_bytes=[want.nbytes, 4 * (n // 64)])
    rows.append(Row("gf192_mul_halves_dev", "gf192 mul_halves (the lane counts: frames only)", build_halves))
    return rows


def _prime_protocol_rows(tag):
    """bn128_protocol_cases' seventeen entries per prime field, at this module's shapes, against that module's integer model"""
    F = _PRIME[tag]
    cases = []
    for log_n in (0, 8, 9):
        sub = max(log_n - 2, 0)
        for op in ("rowcheck", "fz", "vanishing_evals"):
            cases.append(PC._domain_case(F, op, log_n, sub, "seeded"))
        for mu in ("zero", "seeded"):
            cases.append(PC._domain_case(F, "sumcheck_g", log_n, sub, "seeded", mu))
            cases.append(PC._domain_case(F, "rational_sumcheck_constraint", log_n, sub, "seeded", mu))
        cases.append({"op": "domain_offsets", "name": "domain_offsets_%d" % log_n, "log_n": log_n, "shift": PC._scalar(F, "offsets shift"), "point": PC._scalar(F, "offsets point")})
    sc = lambda k, t: [PC._scalar(F, "mc %s %d" % (t, i)) for i in range(k)]              # noqa: E731
    for n in COUNTS:
        cases += [{"op": "lincheck", "name": "lincheck_%d" % n, "n": n, "num": 3, "coeffs": sc(3, "r")},
                  {"op": "lincomb", "name": "lincomb_%d" % n, "n": n, "num": 5, "coeffs": sc(5, "c")},
                  {"op": "lincomb_affine", "name": "lincomb_affine_%d" % n, "n": n, "num": 5, "coeffs": sc(5, "c"), "constant": PC._scalar(F, "affine constant")},
                  {"op": "rational_combine", "name": "rational_combine_%d" % n, "n": n, "num": 3, "coeffs": sc(3, "q")},
                  {"op": "inv", "name": "inv_%d" % n, "n": n, "zeros": "some"},
                  {"op": "div", "name": "div_%d_1" % n, "n": n, "zeros": "some", "with_num": 1}, {"op": "div", "name": "div_%d_0" % n, "n": n, "zeros": "some", "with_num": 0},
                  {"op": "mul", "name": "mul_%d" % n, "n": n}, {"op": "sub", "name": "sub_%d" % n, "n": n},
                  {"op": "pow_table", "name": "pow_table_%d" % n, "n": n, "base": PC._scalar(F, "pow base"), "init": PC._scalar(F, "pow init")}]
    for scale in (None, PC._scalar(F, "spmv scale")):
        for acc in ((0,) if scale is None else (0, 1)):
            cases.append({"op": "spmv", "name": "spmv_%s_%d" % ("noscale" if scale is None else "scale", acc), "rows": 257, "cols": 97, "shape": "mixed", "scale": scale, "accumulate": acc})
    for nc in (9, 257, 264):
        cases.append({"op": "poly_div_vanishing", "name": "poly_div_%d" % nc, "n_coeffs": nc, "sub_log": 3, "shift": PC._scalar(F, "poly div shift")})
    rows = []
    for c in cases:
        def build(c=c):
            inp = PC.inputs(F, c)
            roles = [k for k in inp if k != "out"]
            want = PC.model_words(F, c, inp)
            spmv = c["op"] == "spmv"

            def call(lib, i, o):
                lib._check(PC.call(lib, F, c, dict(zip(roles, i)), o))
            return Case([inp[k] for k in roles], want, call, init={0: inp["out"]} if spmv else None)
        rows.append(Row(_PRIME_METHODS[tag](c["op"]), "%s %s" % (tag, c["name"]), build))
    return rows


# ---- rows: commitment --------------------------------------------------------------------------------------------------------------------
LEAVES = (2, 64, 128, 512)
COSETS = (1, 2, 3, 16)


def _salts(L, nbytes=32):
    return np.random.default_rng(9).integers(0, 256, size=(L, nbytes), dtype=np.uint8)


def _blake_tree_rows():
    rows = []
    # 1024 leaves: the smallest tree with a level above 256 nodes, which k_merkle_level takes instead of the one-workgroup top
    shapes = [(L, cs) for L in LEAVES + (1024,) for cs in (COSETS if L == 64 else (2,))]
    for L, cs in shapes:
        for elem_words, additive, zk in ((3, True, False), (3, False, True), (1, True, False), (4, False, False)) if cs == 2 else ((3, True, False), (3, False, True)):
            n, r = L * cs, 2
            name = "%d leaves, cosets of %d, %d-byte elements, %s%s" % (L, cs, 8 * elem_words, "additive" if additive else "multiplicative", ", salted" if zk else "")

            def build(n=n, r=r, L=L, cs=cs, elem_words=elem_words, additive=additive, zk=zk, split=False):
                oracles = [rand_elems(800 + k, n, elem_words) for k in range(r)]
                salts = _salts(L) if zk else None
                want = oracle.merkle_build(oracles, cs, additive, salts)
                dt = 0 if additive else 1

                def call(lib, i, o):
                    ds = i[r] if zk else 0
                    if split:
                        lib.merkle_leaves_dev(i[:r], 8 * elem_words, n, cs, o[0], dt, ds, 32 if zk else 0)
                        lib.merkle_inner_dev(o[0], L)
                    else:
                        lib.merkle_tree_dev(i[:r], 8 * elem_words, n, cs, o[0], dt, ds, 32 if zk else 0)
                return Case(oracles + ([salts] if zk else []), [want], call)
            rows.append(Row("merkle_tree_dev", "BLAKE2b tree: " + name, build))
            rows.append(Row("merkle_leaves_dev + merkle_inner_dev", "BLAKE2b leaves + inner: " + name, functools.partial(build, split=True)))
    for r, cs, L in merkle_cases.ALIGN:                  # the shapes of the fixed 24-byte leaf kernels, with 1, 2 and 4 oracles (offset 8: the general kernel)
        rows.append(Row("merkle_tree_dev", "BLAKE2b tree: %d oracles, %d leaves, cosets of %d, 24-byte elements, additive" % (r, L, cs),
                        functools.partial(build, n=L * cs, r=r, L=L, cs=cs, elem_words=3, additive=True, zk=False)))
    return rows


def _sub32_rows():
    """the 32-byte leaf path (one alt_bn128 element per leaf, IOPX_LEAVES_SUB32) on and off"""
    rows = []
    for on in (1, 0):
        for cs, r in ((2, 1), (4, 2), (8, 3)):
            def build(on=on, cs=cs, r=r):
                L = 128
                cols = [rand_elems(810 + k, L * cs, 4) for k in range(r)]
                want = oracle.merkle_build(cols, cs, False)

                def call(lib, i, o):
                    # k_merkle_leaves_sub32 takes 16-byte aligned oracles and nodes only: at payload offset 8 the general kernel must run;
                    # which kernel ran is read from the profile, so a wrong switch fails here and not only a wrong digest
                    aligned = all(q % 16 == 0 for q in list(i) + [o[0]])
                    lib.set_option("IOPX_LEAVES_SUB32", on)
                    try:
                        lib.profile_begin()
                        lib.merkle_leaves_dev(i, 32, L * cs, cs, o[0], 1)
                        ran = sorted(k for k in lib.profile_report() if k.startswith("k_merkle_leaves"))
                        lib.merkle_inner_dev(o[0], L)
                    finally:
                        lib.clear_option("IOPX_LEAVES_SUB32")
                    assert ran == (["k_merkle_leaves_sub32"] if on and aligned else ["k_merkle_leaves"]), (ran, on, aligned)
                return Case(cols, [want], call)
            rows.append(Row("merkle_leaves_dev + merkle_inner_dev", "BLAKE2b 32-byte leaves, %d oracles, cosets of %d, IOPX_LEAVES_SUB32=%d (offset 8: the general kernel)" % (r, cs, on), build))
    return rows


def _poseidon_rows():
    rows = []
    for name in ("high_alpha17_t3", "high_alpha17_t4"):
        for L in LEAVES:
            for zk in (False, True):
                cs = 2 if L != 64 else 3

                def build(name=name, L=L, zk=zk, cs=cs):
                    p, po = PO.param_pair(name)
                    oracles = [PO.rand_bn(100 + k, L * cs) for k in range(2)]
                    salts = _salts(L) if zk else None
                    want = oracle.poseidon_merkle(po, oracles, cs, False, salts)
                    return Case(oracles + ([salts] if zk else []), [want],
                                lambda lib, i, o: lib.merkle_tree_poseidon_dev(p, i[:2], L * cs, cs, o[0], 1, i[2] if zk else 0))
                rows.append(Row("merkle_tree_poseidon_dev", "Poseidon %s tree: %d leaves, cosets of %d%s" % (name, L, cs, ", salted" if zk else ""), build))
        for count in (1, 70, 257):
            def build_perm(name=name, count=count):
                p, po = PO.param_pair(name)
                t = p.state_size
                st = PO.rand_bn(11, count * t).reshape(count, t, 4)
                want = np.stack([oracle.poseidon_permute(po, st[k]) for k in range(count)])
                return Case([], [want], lambda lib, i, o: lib._check(lib.c.iopx_poseidon_permute_bn128_dev(ctypes.byref(p.c), _vp(o[0]), _sz(count))), init={0: st})
            rows.append(Row("iopx_poseidon_permute_bn128_dev", "Poseidon %s permutation of %d states" % (name, count), build_perm))
    for count in COUNTS:
        def build_mont(count=count):
            rng = np.random.default_rng(count)
            xs = [int.from_bytes(rng.bytes(32), "little") for _ in range(count)]
            xs[0] = (1 << 256) - 1
            return Case([B.ints_to_words(xs)], [oracle.bn_from_ints([x % oracle.BN128_R for x in xs])],
                        lambda lib, i, o: lib._check(lib.c.iopx_bn128_to_montgomery_dev(_vp(i[0]), _vp(o[0]), _sz(count))))
        rows.append(Row("iopx_bn128_to_montgomery_dev", "bn128_to_montgomery count=%d" % count, build_mont))
    return rows


def _extraction_rows():
    rows = []
    for elem_words in (1, 3, 4):
        def build_q(elem_words=elem_words):
            n, r = 257, 3
            oracles = [rand_elems(820 + k, n, elem_words) for k in range(r)]
            positions = [0, 256, 17, 17, 128, 255]
            want = np.stack([np.stack([o[p] for o in oracles]) for p in positions])
            return Case(oracles, [], lambda lib, i, o: lib.query_responses_dev(i, 8 * elem_words, n, positions), returns=want)
        rows.append(Row("query_responses_dev", "query responses, %d-byte elements" % (8 * elem_words), build_q))
    for L in LEAVES:
        def build_m(L=L):
            col = rand_elems(830, L, 3)
            nodes = oracle.merkle_build([col], 1, True)
            positions = sorted({0, L - 1, L // 2, min(3, L - 1)})
            idx = oracle.membership_proof_indices(L, positions)
            want = np.ascontiguousarray(nodes).reshape(-1, 32).view(np.uint8)[np.asarray(idx, dtype=np.int64)].reshape(-1, 32)
            return Case([nodes], [], lambda lib, i, o: lib.get_set_membership_proof_dev(i[0], L, positions), returns=want)
        rows.append(Row("get_set_membership_proof_dev", "membership proof, %d leaves" % L, build_m))
    return rows


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def _build_groups():
    g = {}
    for lo, hi in ((0, 8), (9, 11), (12, 12), (13, 13), (14, 14), (15, 15)):
        g["gf192 transforms d=%d..%d" % (lo, hi)] = [r for d in range(lo, hi + 1) for r in _gf192_fft_rows(d)]
    g["gf192 coset ranges, batches and re-extensions"] = _gf192_lde_rows()
    # the same forms where phase 2 takes its other paths (fft_add.hip run_phase2 / run_phase2_fwd_batch), in groups of their own
    g["gf192 coset ranges d=10 and d=13"] = [r for kind in ("aurora", "general") for r in _gf192_lde_rows(12, 10, 1, 3, kind, batches=(), forms=False)] + \
        _gf192_lde_rows(15, 13, 1, 3, "aurora", batches=(), forms=False)
    for kind in ("aurora", "general"):
        g["gf192 coset ranges, batches and re-extensions d=11 %s" % kind] = _gf192_lde_rows(13, 11, 1, 3, kind, batches=(3,))
    g["gf192 taylor, combine and pow_table"] = _gf192_block_rows()
    for lo, hi in ((0, 10), (11, 12), (13, 14)):
        g["gf64 transforms d=%d..%d" % (lo, hi)] = [r for d in range(lo, hi + 1) for r in _gf64_rows(d)]
    g["gf64 coset ranges, folds, LDT and products"] = _gf64_other_rows()
    for tag in ("fp3", "bn128"):
        for lo, hi in ((0, 9), (10, 11), (12, 12), (13, 13)):
            g["%s transforms log_n=%d..%d" % (tag, lo, hi)] = [r for k in range(lo, hi + 1) for r in _prime_fft_rows(tag, k)]
        g["%s folds and LDT" % tag] = _prime_fold_ldt_rows(tag)
        g["%s protocol layer" % tag] = _prime_protocol_rows(tag)
    g["gf192 folds and LDT"] = _gf192_fold_ldt_rows()
    g["gf192 protocol layer"] = _gf192_protocol_rows()
    g["entries behind host-array methods"] = _c_symbol_rows()
    g["BLAKE2b trees"] = _blake_tree_rows() + _sub32_rows()
    g["Poseidon trees and permutations"] = _poseidon_rows()
    g["transcript extraction"] = _extraction_rows()
    return g


GROUPS = _build_groups()


def entries_with_rows():
    return sorted({r.entry for rows in GROUPS.values() for r in rows})


LEFT_OUT_SYMBOLS = ("iopx_add_fft_gf192_dist_dev", "iopx_add_ifft_gf192_dist_dev", "iopx_comm_all_gather_dev", "iopx_comm_all_reduce_u64_dev",
                    "iopx_comm_broadcast_dev", "iopx_comm_all_to_all_dev", "iopx_comm_sendrecv_dev",
                    "iopx_gather_dev", "iopx_scatter_dev", "iopx_gather_stride_dev", "iopx_count_mismatch_dev", "iopx_interleave_dev",
                    "iopx_gather_rows_dev", "iopx_memset_dev")
LEFT_OUT = ("additive_FFT_dist_dev",)      # each with its reason in the module docstring


def check_coverage(lib):
    """every *_dev method of Library has a row, or is named in the docstring as left out"""
    have = set()
    for e in entries_with_rows():
        for part in e.split(" + "):
            have.add(part.split(" ")[0])
    methods = sorted(m for m in dir(type(lib)) if m.endswith("_dev") and not m.startswith("_"))
    assert len(methods) >= 70, len(methods)
    missing = [m for m in methods if m not in have and m not in LEFT_OUT]
    assert not missing, missing
    for m in LEFT_OUT:
        assert m in __doc__ and m not in have, m
    # ... and every exported iopx_*_dev symbol is called by a method with a row, named by a row, or left out with its reason
    import inspect
    import re
    import libiop_amd
    reached = {e.split(" ")[0] for e in have if e.startswith("iopx_")}
    for m in methods:
        if m in have:
            reached |= set(re.findall(r"iopx_[a-z0-9_]+_dev", inspect.getsource(getattr(type(lib), m))))
    reached |= {sym for F in _PRIME.values() for sym in F.symbols.values()}                     # the rows of _prime_protocol_rows call these
    reached |= {"iopx_fp3_inv_dev", "iopx_fp3_div_dev", "iopx_gf192_inv_dev", "iopx_gf192_div_dev"}      # chosen by prime_field inside field_inv_dev / field_div_dev
    symbols = [x for x in libiop_amd.EXPORTED_SYMBOLS if x.endswith("_dev")]
    missing = [x for x in symbols if x not in reached and x not in LEFT_OUT_SYMBOLS]
    assert not missing, missing
    for x in LEFT_OUT_SYMBOLS:
        assert x in __doc__ and x not in reached, x


def check_integer_model():
    """int_fft / int_ifft / int_fold / int_ldt with edwards_Fr's parameters against the oracle's transforms, fold and LDT combination"""
    F = PC.ED
    for log_n in (0, 1, 5, 9):
        n = 1 << log_n
        shift = F.generator
        sw = F.elem(shift)
        coeffs = F.data("model fft %d" % log_n, n)[:n // 2 + 1]
        assert np.array_equal(_enc_words(F, int_fft(F, _res(F, coeffs), log_n, shift)), oracle.multiplicative_fft(coeffs, n, sw)), log_n
        evals = F.data("model ifft %d" % log_n, n)
        assert np.array_equal(_enc_words(F, int_ifft(F, _res(F, evals), log_n, shift)), oracle.multiplicative_ifft(evals, sw)), log_n
    log_n, shift = 6, F.generator
    f = F.data("model fold", 1 << log_n)
    for eta in (1, 2, 4):
        for x in (PC._scalar(F, "model x"), PC._scalar(F, "model x'")):      # off the domain: there the reference's loop has a quirk the rows do not need
            want = oracle.fri_fold_multiplicative(f, F.elem(shift), 1 << eta, F.elem(x))
            assert np.array_equal(_enc_words(F, int_fold(F, _res(F, f), log_n, shift, 1 << eta, x)), want), (eta, x)
    degrees = [64, 63, 20, 64, 7]
    evals = [F.data("model ldt %d" % k, 1 << log_n) for k in range(len(degrees))]
    cs = [PC._scalar(F, "model ldt c %d" % k) for k in range(2 * len(degrees))]
    want = oracle.ldt_combine_fp(evals, degrees, F.to_words([F.enc(c) for c in cs]), 1 << log_n, F.elem(shift))
    assert np.array_equal(_enc_words(F, int_ldt(F, [_res(F, e) for e in evals], degrees, cs, log_n, shift)), want)


# ---- B3: the provers under the mode ------------------------------------------------------------------------------------------------
def _aurora_and_fractal(lib):
    import stream_schedule_cases as S
    S.check_aurora_and_fractal(lib)                     # gf192 and edwards_Fr, (8, 15) / (7, 0); a warmed instance proves twice


def _fri_snarks(lib):
    import bn128_fri_snark_cases as BF
    import stream_schedule_cases as S
    S.check_fri_snarks(lib, BF.load_fixture())          # gf192, edwards_Fr, alt_bn128 Fr with BLAKE2b and Poseidon


def _fri_snark_gf64(lib, on_gpu, proofs=2):
    """the Python prover over DeviceOps (the native one has no gf64 arm): torch owns the oracles, the library its temporaries and plans"""
    import torch
    from libiop_amd import domains, fri, r1cs
    if on_gpu:
        lib.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        _fri_snark_gf64_on(lib, torch, torch.device("cuda:0" if on_gpu else "cpu"), domains, fri, r1cs, proofs)
    finally:
        if on_gpu:
            lib.use_own_stream()


def _fri_snark_gf64_on(lib, torch, device, domains, fri, r1cs, proofs):
    ops = domains.DeviceOps(lib, torch, device, domains.GF64())
    (dim, rs_extra, loc, interactions, queries), size = G64.FRI_SNARK_TUPLES[0]
    params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
    coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (dim - rs_extra))
    ref = oracle.fri_snark_prove(oracle.FIELD_GF64, dim, rs_extra, loc, interactions, queries, 5)
    assert len(ref) == size
    for _ in range(proofs):                              # a second proof finds the first one's blocks in the pool
        assert fri.fri_snark_prover(ops, params, d_poly_coeffs=ops.upload(coeffs)).serialize() == ref


def _aurora_bn128(lib):
    import bn128_aurora_cases as BA
    import stream_schedule_cases as S
    fixture = BA.load_fixture()
    for hash_name in ("blake2b", "poseidon_starkware"):
        S.check_bn128_aurora(lib, fixture, hash_name, 1, 1)


def _fallback_schedule(lib):
    import stream_schedule_cases as S
    S.check_general_r1cs(lib, "auxiliary")              # an unsatisfied witness: head evaluation falls back to the reference's schedule


PROVER_CASES = {"aurora and fractal over gf192 and edwards_Fr, warm second proofs": _aurora_and_fractal, "fri snarks over gf192, edwards_Fr and alt_bn128 Fr": _fri_snarks,
                "fri snark over gf64": _fri_snark_gf64, "aurora over alt_bn128 Fr": _aurora_bn128, "unsatisfied witness on the fallback schedule": _fallback_schedule}


def check_prover(lib, case, on_gpu=False):
    for poison in POISONS:
        with memory_checks(lib, poison):
            if PROVER_CASES[case] is _fri_snark_gf64:
                _fri_snark_gf64(lib, on_gpu, proofs=1 if poison == POISONS[0] else 2)     # the warm second proof once
            else:
                PROVER_CASES[case](lib)


# ---- the mode itself: off, on, and switched while blocks are live ----------------------------------------------------------------------
def check_mode_off_and_mixing(lib, align=16):
    """align: what the allocator under the library aligns to (malloc on the CPU build, 256 bytes and more for hipMalloc)"""
    import stream_schedule_cases as S
    lib.init(0)
    lib.clear_plans()
    lib.mem_check_stats(reset=True)
    n = 10000
    p = S.pool_alloc(lib, n)
    S.pool_free(lib, p)
    assert S.pool_alloc(lib, n) == p, "mode off: the pool recycles as before"
    S.pool_free(lib, p)
    d = lib.malloc(n)
    lib.free(d)
    assert lib.mem_check_stats() == (0, 0, ""), "mode off: nothing is checked"
    lib.set_option("IOPX_MEM_CHECK", 1)
    lib.set_option("IOPX_MEM_CHECK_POISON", 0x5A)
    try:
        q = S.pool_alloc(lib, n)
        assert q != p and q % align == 0, "a plain block is not recycled as a guarded one; the payload keeps the allocation's alignment"
        assert np.array_equal(S.read(lib, q, n), S.filled(0x5A, n))
        mv.memset_dev(lib, q, 0x77, n)
        S.pool_free(lib, q)
        assert lib.mem_check_stats()[:2] == (1, 0)
        r = S.pool_alloc(lib, 6000)                     # the recycled block: the size-match rule on the payload, the slack behind it guard
        assert r == q
        assert np.array_equal(S.read(lib, r, 6000), S.filled(0x5A, 6000)), "a recycled block is poisoned again"
        mv.memset_dev(lib, r, 0x78, 6000)
        g = lib.malloc(n)
        lib.clear_option("IOPX_MEM_CHECK")              # off, with two guarded blocks live
        assert S.pool_alloc(lib, n) == p, "mode off again: the plain block, not the guarded one"
        S.pool_free(lib, p)
        S.pool_free(lib, r)
        lib.free(g)
        assert lib.mem_check_stats()[:2] == (3, 0), "a block keeps its layout: released with the mode off, still checked"
    finally:
        lib.clear_option("IOPX_MEM_CHECK")
        lib.clear_option("IOPX_MEM_CHECK_POISON")
        lib.clear_plans()
        lib.mem_check_stats(reset=True)
