"""The memory contract of the GF(2^64) protocol-layer entries (libiop_amd/csrc/gfx_ops.h, instantiated by gf64_ops.hip) and of one native gf64 Aurora proof, with the
harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes, every output in a frame pre-filled
with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it allocates, poisoned payloads), two
poison bytes, payload offsets 0 and 8 modulo 16 — the entries take two elements per lane at the first offset and one at the second.  After
each call the outputs equal the oracle's bytes, every frame is intact, the inputs read back unchanged, no guard is damaged and the bytes do
not follow the poison (no read of a temporary that was never written).  On the CPU build of the kernels and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import gf64_aurora_cases as C
import gf64_cases as G
import memory_contract_cases as mc
import oracle

N = 257         # above one workgroup, odd: the last pair of the two-element form is half empty


def _domain(m):
    return C.codeword_domain(m)


def _add():
    a, b = G.seeded("mem add a", N), G.seeded("mem add b", N)
    return mc.Case([a, b], [a ^ b], lambda lib, i, o: lib.field_add_dev(i[0], i[1], o[0], N, words=1))


def _pow_table():
    base, init = G.elem(int(G.seeded("mem pow", 1)[0, 0]) | C.BIT63), G.elem(0x1234567)
    want, cur = np.empty((N, 1), dtype=np.uint64), init.reshape(1, 1)
    for l in range(N):
        want[l] = cur[0]
        cur = oracle.gf_mul(cur, base.reshape(1, 1))
    return mc.Case([], [want], lambda lib, i, o: lib.pow_table_dev(o[0], N, base, init, words=1))


def _lincomb(affine):
    vecs, coef, constant = [G.seeded("mem lincomb %d" % k, N) for k in range(5)], G.seeded("mem lincomb c", 5), G.elem(77 | C.BIT63)
    want = C.xor_all([C.scaled(v, c) for v, c in zip(vecs, coef)])
    if affine:
        return mc.Case(vecs, [want ^ constant.reshape(1, 1)], lambda lib, i, o: lib.lincomb_affine_dev(i, coef, constant, N, o[0], words=1))
    return mc.Case(vecs, [want], lambda lib, i, o: lib.lincomb_dev(i, coef, N, o[0], words=1))


def _spmv():
    rows, cols = N, 40
    rng = np.random.default_rng(7)
    lengths = rng.integers(0, 4, size=rows)
    lengths[0], lengths[5] = 0, 50
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    col = rng.integers(0, cols, size=int(row_ptr[-1])).astype(np.uint32)
    coef, vec, old, scale = G.seeded("mem spmv c", col.shape[0]), G.seeded("mem spmv v", cols), G.seeded("mem spmv old", rows), G.elem(C.BIT63 | 3)
    prod = oracle.gf_mul(coef, vec[col])
    want = np.zeros((rows, 1), dtype=np.uint64)
    for r in range(rows):
        for t in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            want[r] ^= prod[t]
    return mc.Case([row_ptr, col, coef, vec], [C.scaled(want, scale) ^ old],
                   lambda lib, i, o: lib.spmv_dev(i[0], i[1], i[2], rows, i[3], o[0], scale=scale, accumulate=True, words=1), init={0: old})


def _lincheck():
    fz, p1, p2 = (G.seeded("mem lincheck %s" % t, N) for t in ("fz", "p1", "p2"))
    mz, r = [G.seeded("mem lincheck mz %d" % k, N) for k in range(3)], G.seeded("mem lincheck r", 3)
    return mc.Case([fz, p1, p2] + mz, [oracle.lincheck_combine(fz, mz, r, p1, p2)], lambda lib, i, o: lib.lincheck_dev(i[0], i[3:], r, i[1], i[2], N, o[0], words=1))


def _rowcheck():
    m, h = 9, 4
    basis, shift = _domain(m)
    cshift = G.elem(0x55)
    az, bz, cz = (G.seeded("mem rowcheck %s" % t, 1 << m) for t in "abc")
    return mc.Case([az, bz, cz], [oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)],
                   lambda lib, i, o: lib.rowcheck_dev(i[0], i[1], i[2], basis, shift, h, cshift, o[0], words=1))


def _fz():
    m = 9
    basis, shift = _domain(m)
    ib, ishift = basis[:3], G.elem(C.BIT63 | 9)
    fw, f1v = G.seeded("mem fz w", 1 << m), G.seeded("mem fz v", 1 << m)
    return mc.Case([fw, f1v], [oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)], lambda lib, i, o: lib.fz_dev(i[0], i[1], basis, shift, ib, ishift, o[0], words=1))


def _sumcheck_g(nonzero):
    m = 9
    basis, shift = _domain(m)
    sb, sshift = basis[:5], G.elem(0)
    mu = G.elem((C.BIT63 | 0xABCDEF) if nonzero else 0)
    f, h = G.seeded("mem sumcheck f", 1 << m), G.seeded("mem sumcheck h", 1 << m)
    return mc.Case([f, h], [oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, mu)],
                   lambda lib, i, o: lib.sumcheck_g_dev(i[0], i[1], basis, shift, sb, sshift, mu, o[0], words=1))


def _poly_div_vanishing():
    """three passes (a temporary between them): 2^9 - 3 coefficients by the vanishing polynomial of 2^5 points; the quotient is pinned by
    multiplying back"""
    basis, shift = G.std_basis(5), G.elem(C.BIT63 | 0x80)
    n_coeffs, N5 = 509, 32
    Z = C._vanishing_coefficients(basis, shift)
    q = G.seeded("mem polydiv q", n_coeffs - N5)
    poly = C._poly_mul(q, Z)
    poly[:N5] ^= G.seeded("mem polydiv r", N5)              # any remainder of degree below |H|
    return mc.Case([poly], [q], lambda lib, i, o: lib.poly_div_vanishing_dev(i[0], n_coeffs, basis, shift, o[0], words=1))


ROWS = [mc.Row("iopx_gf64_add_dev", "gf64 add", _add), mc.Row("iopx_gf64_pow_table_dev", "gf64 pow_table", _pow_table),
        mc.Row("iopx_lincomb_gf64_dev", "gf64 lincomb", lambda: _lincomb(False)), mc.Row("iopx_lincomb_affine_gf64_dev", "gf64 lincomb_affine", lambda: _lincomb(True)),
        mc.Row("iopx_spmv_gf64_dev", "gf64 spmv, scaled and accumulated", _spmv), mc.Row("iopx_lincheck_gf64_dev", "gf64 lincheck", _lincheck),
        mc.Row("iopx_rowcheck_gf64_dev", "gf64 rowcheck", _rowcheck), mc.Row("iopx_fz_gf64_dev", "gf64 fz", _fz),
        mc.Row("iopx_sumcheck_g_gf64_dev", "gf64 sumcheck_g, claimed sum zero", lambda: _sumcheck_g(False)),
        mc.Row("iopx_sumcheck_g_gf64_dev", "gf64 sumcheck_g, claimed sum non-zero", lambda: _sumcheck_g(True)),
        mc.Row("iopx_poly_div_vanishing_gf64_dev", "gf64 poly_div_vanishing", _poly_div_vanishing)]


def _native_proof(lib):
    """one native gf64 proof (7, 15) and a warm second one, per poison byte: the oracle's bytes each time"""
    import libiop_amd as la
    ref = oracle.aurora_prove(oracle.FIELD_GF64, 7, 15, C.SEED)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            inst = lib.aurora_example_instance(la.FIELD_GF64, 128, 15, 127, C.SEED)
            try:
                assert lib.aurora_prove(inst) == ref
                assert lib.aurora_prove(inst) == ref
            finally:
                lib.aurora_instance_free(inst)


def test_every_new_entry_has_a_row():
    import libiop_amd
    new = [s for s in libiop_amd.EXPORTED_SYMBOLS if "gf64" in s and s.endswith("_dev") and s not in
           ("iopx_add_fft_gf64_dev", "iopx_add_lde_gf64_dev", "iopx_add_ifft_gf64_dev", "iopx_fri_fold_add_gf64_dev", "iopx_ldt_combine_gf64_dev",
            "iopx_gf64_mul_dev", "iopx_gf64_inv_dev")]          # those have their rows in memory_contract_cases
    assert len(new) == 10 and sorted(set(r.entry for r in ROWS)) == sorted(new)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_").replace(",", ""))
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


def test_native_proof_on_the_cpu_build():
    from emu_lib import emu
    _native_proof(emu())


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_").replace(",", ""))
def test_entries_on_the_gpu(gpu, row):
    mc.run_row(gpu, row)


@pytest.mark.gpu
def test_native_proof_on_the_gpu(gpu):
    _native_proof(gpu)
