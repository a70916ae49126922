"""The memory contract of the lean rational combination over gf128 and gf256 (IOPX_GFX_RATIONAL_FORM=2, and =1 beside it) and of one native Fractal
proof per wide field under IOPX_GFX_FRACTAL_WIDE=1, with the harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random
non-zero bytes, every output in a frame pre-filled with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every
block it allocates, poisoned payloads), two poison bytes, payload offsets 0 and 8 modulo 16.  After each call the outputs equal the expected bytes,
every frame is intact, the inputs read back unchanged and no guard is damaged.  On the CPU build and (-m gpu) on the MI355X."""
import pytest

import gfx_aurora_cases as C
import gfx_fractal_cases as F
import gfx_fractal_wide_cases as FW
import memory_contract_cases as mc


def _combine(W, form, num, n):
    Ns, Ds, coef, want = FW.instance(W, num, n, "wide mem")

    def call(lib, i, o):
        with C.options(lib, **{FW.OPTION: form}):
            lib.rational_combine_dev(i[:num], i[num:], coef, n, o[0], o[1], words=W)
    return mc.Case(Ns + Ds, list(want), call)


def _rows(W):
    f = FW.NAME[W]
    entry = "iopx_rational_combine_%s_dev" % f
    return [mc.Row(entry, "%s rational combine form %d, %d rationals over %d" % (f, form, num, n), lambda form=form, num=num, n=n: _combine(W, form, num, n))
            for form in FW.FORMS for num, n in ((4, 513), (1, 257))]


ROWS = [r for W in FW.WORDS for r in _rows(W)]


def _native_proof(lib, W):
    """one native index and two proofs per poison byte: the model's bytes each time, no damage"""
    case = FW.NATIVE_TUPLES[0]
    want, want_roots, inst = FW.model(W, case)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            roots, proofs, _ = FW.native_index_and_prove(lib, W, inst, case[2], case[3], proofs=2)
            assert roots == want_roots and proofs == [want, want]


W_PARAM = pytest.mark.parametrize("words", FW.WORDS, ids=lambda w: FW.NAME[w])


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_").replace(",", ""))
def test_combine_forms_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


@W_PARAM
def test_native_fractal_proof_on_the_cpu_build(words):
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
def test_combine_forms_on_the_gpu(gpu, row):
    mc.run_row(gpu, row)


@pytest.mark.gpu
@W_PARAM
def test_native_fractal_proof_on_the_gpu(gpu, words):
    _native_proof(gpu, words)
