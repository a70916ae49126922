"""The memory contract of the GF(2^128) and GF(2^256) protocol-layer entries (libiop_amd/csrc/gfx_ops.h) and of one native Aurora proof per
field, with the harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes, every output in a frame
pre-filled with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it allocates, poisoned
payloads), two poison bytes, payload offsets 0 and 8 modulo 16 — at the second offset no buffer of a call is 16-byte aligned, so the entries
run their 64-bit-word form.  After each call the outputs equal the reference's bytes, every frame is intact, the inputs read back unchanged,
no guard is damaged and the bytes do not follow the poison.  On the CPU build of the kernels and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import gfx_aurora_cases as C
import gfx_aurora_model as M
import memory_contract_cases as mc
import oracle

N = 257         # above one workgroup, odd


def _pow_table(W):
    base, init = C.one_seeded("mem pow", W, True), C.elem(W, 0x1234567)
    return mc.Case([], [C.pow_reference(base, init, N)], lambda lib, i, o: lib.pow_table_dev(o[0], N, base, init, words=W))


def _lincomb(W, affine):
    vecs, coef, constant = [C.seeded("mem lincomb %d" % k, N, W) for k in range(5)], C.seeded("mem lincomb c", 5, W), C.elem(W, 77 | C.top(W))
    want = C.xor_all([C.scaled(v, c) for v, c in zip(vecs, coef)])
    if affine:
        return mc.Case(vecs, [want ^ constant.reshape(1, W)], lambda lib, i, o: lib.lincomb_affine_dev(i, coef, constant, N, o[0], words=W))
    return mc.Case(vecs, [want], lambda lib, i, o: lib.lincomb_dev(i, coef, N, o[0], words=W))


def _spmv(W):
    row_ptr, col, coef, vec = C.spmv_system(W, N, 40, 7)
    old, scale = C.seeded("mem spmv old", N, W), C.elem(W, C.top(W) | 3)
    want = C.spmv_reference(row_ptr, col, coef, vec, N)
    return mc.Case([row_ptr, col, coef, vec], [C.scaled(want, scale) ^ old],
                   lambda lib, i, o: lib.spmv_dev(i[0], i[1], i[2], N, i[3], o[0], scale=scale, accumulate=True, words=W), init={0: old})


def _lincheck(W):
    fz, p1, p2 = (C.seeded("mem lincheck %s" % t, N, W) for t in ("fz", "p1", "p2"))
    mz, r = [C.seeded("mem lincheck mz %d" % k, N, W) for k in range(3)], C.seeded("mem lincheck r", 3, W)
    return mc.Case([fz, p1, p2] + mz, [oracle.lincheck_combine(fz, mz, r, p1, p2)], lambda lib, i, o: lib.lincheck_dev(i[0], i[3:], r, i[1], i[2], N, o[0], words=W))


def _rowcheck(W):
    m, h = 9, 4
    basis, shift = C.codeword_domain(m, W)
    cshift = C.elem(W, 0x55)
    az, bz, cz = (C.seeded("mem rowcheck %s" % t, 1 << m, W) for t in "abc")
    return mc.Case([az, bz, cz], [oracle.rowcheck_additive(az, bz, cz, basis, shift, h, cshift)],
                   lambda lib, i, o: lib.rowcheck_dev(i[0], i[1], i[2], basis, shift, h, cshift, o[0], words=W))


def _fz(W):
    m = 9
    basis, shift = C.codeword_domain(m, W)
    ib, ishift = basis[:3], C.elem(W, C.top(W) | 9)
    fw, f1v = C.seeded("mem fz w", 1 << m, W), C.seeded("mem fz v", 1 << m, W)
    return mc.Case([fw, f1v], [oracle.fz_additive(fw, f1v, basis, shift, ib, ishift)], lambda lib, i, o: lib.fz_dev(i[0], i[1], basis, shift, ib, ishift, o[0], words=W))


def _sumcheck_g(W, nonzero):
    m = 9
    basis, shift = C.codeword_domain(m, W)
    sb, sshift = basis[:5], C.elem(W, 0)
    mu = C.elem(W, (C.top(W) | 0xABCDEF) if nonzero else 0)
    f, h = C.seeded("mem sumcheck f", 1 << m, W), C.seeded("mem sumcheck h", 1 << m, W)
    return mc.Case([f, h], [oracle.sumcheck_g_additive(f, h, basis, shift, sb, sshift, mu)],
                   lambda lib, i, o: lib.sumcheck_g_dev(i[0], i[1], basis, shift, sb, sshift, mu, o[0], words=W))


def _poly_div_vanishing(W):
    """several passes (a temporary between them): 2^9 - 3 coefficients by the vanishing polynomial of 2^5 points"""
    basis, shift = oracle.standard_basis(5, W), C.elem(W, C.top(W) | 0x80)
    n_coeffs = 509
    poly = C.seeded("mem polydiv", n_coeffs, W)
    return mc.Case([poly], [M.div_vanishing(poly, n_coeffs, basis, shift)], lambda lib, i, o: lib.poly_div_vanishing_dev(i[0], n_coeffs, basis, shift, o[0], words=W))


def _rows(W):
    f = C.NAME[W]
    return [mc.Row("iopx_%s_pow_table_dev" % f, f + " pow_table", lambda: _pow_table(W)),
            mc.Row("iopx_lincomb_%s_dev" % f, f + " lincomb", lambda: _lincomb(W, False)), mc.Row("iopx_lincomb_affine_%s_dev" % f, f + " lincomb_affine", lambda: _lincomb(W, True)),
            mc.Row("iopx_spmv_%s_dev" % f, f + " spmv, scaled and accumulated", lambda: _spmv(W)), mc.Row("iopx_lincheck_%s_dev" % f, f + " lincheck", lambda: _lincheck(W)),
            mc.Row("iopx_rowcheck_%s_dev" % f, f + " rowcheck", lambda: _rowcheck(W)), mc.Row("iopx_fz_%s_dev" % f, f + " fz", lambda: _fz(W)),
            mc.Row("iopx_sumcheck_g_%s_dev" % f, f + " sumcheck_g, claimed sum zero", lambda: _sumcheck_g(W, False)),
            mc.Row("iopx_sumcheck_g_%s_dev" % f, f + " sumcheck_g, claimed sum non-zero", lambda: _sumcheck_g(W, True)),
            mc.Row("iopx_poly_div_vanishing_%s_dev" % f, f + " poly_div_vanishing", lambda: _poly_div_vanishing(W))]


ROWS = _rows(2) + _rows(4)


def _native_proof(lib, W):
    """one native proof (7, 15) and a warm second one, per poison byte: the model's bytes each time"""
    want, _, inst = C.model(W, 7, 15)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            h = lib.aurora_instance(C.field_code(W), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
            try:
                assert lib.aurora_prove(h) == want
                assert lib.aurora_prove(h) == want
            finally:
                lib.aurora_instance_free(h)


def test_every_new_entry_has_a_row():
    import libiop_amd
    assert len(libiop_amd.GFX_OPS_SYMBOLS) == 18 and sorted(set(r.entry for r in ROWS)) == sorted(libiop_amd.GFX_OPS_SYMBOLS)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_").replace(",", ""))
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


@pytest.mark.parametrize("words", C.WORDS, ids=lambda w: C.NAME[w])
def test_native_proof_on_the_cpu_build(words):
    from emu_lib import emu
    _native_proof(emu(), words)


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
@pytest.mark.parametrize("words", C.WORDS, ids=lambda w: C.NAME[w])
def test_native_proof_on_the_gpu(gpu, words):
    _native_proof(gpu, words)
