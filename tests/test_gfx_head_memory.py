"""The memory contract of the device entries of include/libiop_amd_head.h over gf64, gf128 and gf256 and of one native gf128 proof by the head route,
with the harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes, every output in a frame pre-filled
with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it allocates, poisoned payloads), two poison
bytes, payload offsets 0 and 8 modulo 16.  After each call the outputs equal the expected bytes, every frame is intact, the inputs read back
unchanged and no guard is damaged.  The division's input is built from its expected output (in = out * Z_S, a plain product); the re-extension's
expected values are the oracle's transforms.  On the CPU build and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import gfx_head_cases as H
import memory_contract_cases as mc
import oracle

M_DIM, D, BEGIN, COUNT = 10, 6, 3, 5


def _div(W):
    m, sub_dim = 9, 4
    basis, shift, sub_shift = H.div_domains(m, sub_dim, W, "seeded")
    Z = H.vanishing_over(oracle.all_subset_sums(basis, shift), oracle.all_subset_sums(basis[:sub_dim], sub_shift))
    assert Z.any(axis=1).all()
    quotient = H.seeded("mem div", 1 << m, W)
    return mc.Case([oracle.gf_mul(quotient, Z)], [quotient], lambda lib, i, o: lib.div_by_vanishing(i[0], basis, shift, sub_dim, sub_shift, o[0], words=W))


def _reextend2(W):
    basis = oracle.standard_basis(M_DIM, W)
    shift, sa, sb = H.reextend_shifts(M_DIM, W, "seeded")
    va = [H.seeded("mem re2 a %d" % k, 1 << D, W) for k in range(2)]
    vb = [H.seeded("mem re2 b %d" % k, 1 << D, W) for k in range(3)]
    outs = [oracle.additive_fft(oracle.additive_ifft(v, basis[:D], s), basis, shift)[BEGIN << D:(BEGIN + COUNT) << D] for vs, s in ((va, sa), (vb, sb)) for v in vs]
    return mc.Case([np.concatenate(va), np.concatenate(vb)], outs,
                   lambda lib, i, o: lib.additive_reextend2_batch_dev(i[0], 2, sa, i[1], 3, sb, basis, D, shift, BEGIN, COUNT, o, words=W))


def _rows(W):
    f = H.NAME[W]
    return [mc.Row("iopx_div_by_vanishing_%s_dev" % f, f + " division by Z_S", lambda: _div(W)),
            mc.Row("iopx_add_reextend2_%s_batch_dev" % f, f + " two-group re-extension", lambda: _reextend2(W))]


ROWS = [r for W in H.WORDS for r in _rows(W)]


def _native_proof(lib):
    """one native gf128 proof (7, 15) by the head route and a warm second one, per poison byte: the model's bytes each time, no damage"""
    import gfx_aurora_cases as C
    want, _, inst = C.model(2, 7, 15)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            h = lib.aurora_instance(C.field_code(2), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
            try:
                with C.options(lib, **{H.OPTION: 1}):
                    lib.profile_begin()
                    assert lib.aurora_prove(h) == want
                    assert H.launches(lib.profile_report(), "k128_", "div_by_vanishing") == 1
                    assert lib.aurora_prove(h) == want
            finally:
                lib.aurora_instance_free(h)


def test_every_device_entry_has_a_row():
    import libiop_amd
    names = [n for n in libiop_amd.HEAD_SYMBOLS if n.endswith("_dev")]
    assert len(names) == 6 and sorted(r.entry for r in ROWS) == sorted(names)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_"))
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


def test_native_gf128_head_proof_on_the_cpu_build():
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
def test_native_gf128_head_proof_on_the_gpu(gpu):
    _native_proof(gpu)
