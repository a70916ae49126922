"""The memory contract of the batched transforms and the fused re-extension over gf64, gf128 and gf256 (include/libiop_amd_batch.h) and of one
native gf128 proof through them, with the harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes,
every output in a frame pre-filled with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it
allocates, poisoned payloads), two poison bytes, payload offsets 0 and 8 modulo 16.  After each call the outputs equal the oracle's bytes, every
frame is intact, the inputs read back unchanged, no guard is damaged and the bytes do not follow the poison.  The rows run three vectors of 2^6
elements onto cosets [3, 8) of 2^10 points (a range that starts past the first coset and is no power of two); the multi-pass geometries are
tests/test_gfx_batch_emu.py's.  On the CPU build and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import gfx_batch_cases as B
import memory_contract_cases as mc
import oracle

M, D, BEGIN, COUNT, BATCH = 10, 6, 3, 5, 3


def _window(full):
    return full[BEGIN << D:(BEGIN + COUNT) << D]


def _ifft(W):
    basis, shift = B.domain(D, W)
    ev = [B.seeded("mem ifft %d" % k, 1 << D, W) for k in range(BATCH)]
    return mc.Case([np.concatenate(ev)], [np.concatenate([oracle.additive_ifft(e, basis, shift) for e in ev])],
                   lambda lib, i, o: lib.additive_IFFT_batch_dev(i[0], BATCH, basis, shift, o[0], words=W))


def _lde(W):
    basis, shift = B.domain(M, W)
    cs = [B.seeded("mem lde %d" % k, (1 << D) - 3, W) for k in range(BATCH)]
    return mc.Case(cs, [_window(oracle.additive_fft(c, basis, shift)) for c in cs],
                   lambda lib, i, o: lib.additive_LDE_batch_dev(i, (1 << D) - 3, basis, shift, BEGIN, COUNT, o, words=W))


def _reextend(W, n_polys):
    basis, shift = B.domain(M, W)
    es = B.seeded("mem re shift", 1, W)[0]
    ev = [B.seeded("mem re %d" % k, 1 << D, W) for k in range(BATCH)]
    polys = [B.seeded("mem re poly %d" % k, (1 << D) - 3, W) for k in range(n_polys)]
    outs = [_window(oracle.additive_fft(oracle.additive_ifft(e, basis[:D], es), basis, shift)) for e in ev] + [_window(oracle.additive_fft(c, basis, shift)) for c in polys]
    if n_polys:
        return mc.Case([np.concatenate(ev)] + polys, outs,
                       lambda lib, i, o: lib.additive_reextend_lde_batch_dev(i[0], BATCH, i[1:], (1 << D) - 3, basis, D, es, shift, BEGIN, COUNT, o, words=W))
    return mc.Case([np.concatenate(ev)], outs, lambda lib, i, o: lib.additive_reextend_batch_dev(i[0], BATCH, basis, D, es, shift, BEGIN, COUNT, o, words=W))


def _rows(W):
    f = B.NAME[W]
    return [mc.Row("iopx_add_ifft_%s_batch_dev" % f, f + " IFFT batch", lambda: _ifft(W)), mc.Row("iopx_add_lde_%s_batch_dev" % f, f + " LDE batch", lambda: _lde(W)),
            mc.Row("iopx_add_reextend_%s_batch_dev" % f, f + " re-extension batch", lambda: _reextend(W, 0)),
            mc.Row("iopx_add_reextend_lde_%s_batch_dev" % f, f + " re-extension batch with two polynomials", lambda: _reextend(W, 2))]


ROWS = [r for W in B.WORDS for r in _rows(W)]


def _native_proof(lib):
    """one native gf128 proof (7, 15) and a warm second one, per poison byte: the model's bytes each time"""
    import gfx_aurora_cases as C
    want, _, inst = C.model(2, 7, 15)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            h = lib.aurora_instance(C.field_code(2), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
            try:
                assert lib.aurora_prove(h) == want
                assert lib.aurora_prove(h) == want
            finally:
                lib.aurora_instance_free(h)


def test_every_batch_symbol_has_a_row():
    import libiop_amd
    assert len(libiop_amd.BATCH_SYMBOLS) == 12 and sorted(r.entry for r in ROWS) == sorted(libiop_amd.BATCH_SYMBOLS)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_"))
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


def test_native_gf128_proof_on_the_cpu_build():
    from emu_lib import emu
    _native_proof(emu())


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_"))
def test_entries_on_the_gpu(gpu, row):
    mc.run_row(gpu, row)


@pytest.mark.gpu
def test_native_gf128_proof_on_the_gpu(gpu):
    _native_proof(gpu)
