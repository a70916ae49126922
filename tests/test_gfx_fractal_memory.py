"""The memory contract of the device entries of include/libiop_amd_fractal.h over gf64, gf128 and gf256 and of one native gf64 Fractal proof, with the
harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes, every output in a frame pre-filled with random
bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it allocates, poisoned payloads), two poison bytes, payload
offsets 0 and 8 modulo 16.  After each call the outputs equal the expected bytes, every frame is intact, the inputs read back unchanged and no guard
is damaged.  The constraint oracle's inputs are built from its expected output (N = out * Z_K + D (p + ...), plain products).  On the CPU build and
(-m gpu) on the MI355X."""
import numpy as np
import pytest

import gfx_aurora_cases as C
import gfx_fractal_cases as F
import gfx_head_cases as H
import memory_contract_cases as mc
import oracle


def _div(W):
    n = 256 * 16 + 3
    den, num = F.seeded("mem div den", n, W), F.seeded("mem div num", n, W)
    den[0] = 0
    den[n - 1] = 0
    return mc.Case([num, den], [F.div_expected(num, den)], lambda lib, i, o: lib.field_div_dev(i[0], i[1], o[0], n, words=W))


def _domain_offsets(W):
    basis, shift = F.domain(9, W, "seeded")
    point = F.seeded("mem point", 1, W)[0]
    return mc.Case([], [oracle.all_subset_sums(basis, shift) ^ point], lambda lib, i, o: lib.domain_offsets_dev(basis, shift, point, o[0], words=W))


def _vanishing_evals(W):
    basis, shift = F.domain(9, W, "seeded")
    vb, vshift, constant = basis[:4], F.seeded("mem vshift", 1, W)[0], F.seeded("mem constant", 1, W)[0]
    want = H.vanishing_over(oracle.all_subset_sums(basis, shift), oracle.all_subset_sums(vb, vshift)) ^ constant
    return mc.Case([], [want], lambda lib, i, o: lib.vanishing_evals_dev(basis, shift, vb, vshift, constant, o[0], words=W))


def _rational_combine(W):
    n, num = 513, 3
    Ns, Ds = [F.seeded("mem N %d" % k, n, W) for k in range(num)], [F.seeded("mem D %d" % k, n, W) for k in range(num)]
    coef = F.seeded("mem coef", num, W)
    return mc.Case(Ns + Ds, list(F.rational_expected(Ns, Ds, coef)), lambda lib, i, o: lib.rational_combine_dev(i[:num], i[num:], coef, n, o[0], o[1], words=W))


def _constraint(W):
    m, k = 9, 4
    mu = F.seeded("mem sum", 1, W)[0]
    basis, shift, kshift, xinv, p, N, D, Z, rhs = F.constraint_setup(W, m, k, "seeded", mu)
    quotient = F.seeded("mem quotient", 1 << m, W)
    N = N ^ rhs ^ oracle.gf_mul(quotient, Z)                     # out * Z_K = D (p + ...) + N holds for out = quotient
    return mc.Case([p, N, D, xinv], [quotient],
                   lambda lib, i, o: lib.rational_sumcheck_constraint_dev(i[0], i[1], i[2], i[3], basis, shift, k, kshift, mu, o[0], words=W))


def _rows(W):
    f = F.NAME[W]
    return [mc.Row("iopx_%s_div_dev" % f, f + " batch division", lambda: _div(W)),
            mc.Row("iopx_domain_offsets_%s_dev" % f, f + " domain offsets", lambda: _domain_offsets(W)),
            mc.Row("iopx_vanishing_evals_%s_dev" % f, f + " vanishing evals", lambda: _vanishing_evals(W)),
            mc.Row("iopx_rational_combine_%s_dev" % f, f + " rational combine", lambda: _rational_combine(W)),
            mc.Row("iopx_rational_sumcheck_constraint_%s_dev" % f, f + " rational sumcheck constraint", lambda: _constraint(W))]


ROWS = [r for W in F.WORDS for r in _rows(W)]


def _native_proof(lib):
    """one native gf64 Fractal index and two proofs per poison byte: the oracle's bytes each time, no damage"""
    case = F.NATIVE_TUPLES[0]
    ref, ref_roots = F.oracle_proof(case)
    for poison in mc.POISONS:
        with mc.memory_checks(lib, poison):
            roots, proofs, _ = F.native_index_and_prove(lib, *case, proofs=2)
            assert roots == ref_roots and proofs == [ref, ref]


def test_every_device_entry_has_a_row():
    import libiop_amd
    names = [n for n in libiop_amd.FRACTAL_SYMBOLS if n.endswith("_dev")]
    assert len(names) == 15 and sorted(r.entry for r in ROWS) == sorted(names)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name.replace(" ", "_"))
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


def test_native_gf64_fractal_proof_on_the_cpu_build():
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
def test_native_gf64_fractal_proof_on_the_gpu(gpu):
    _native_proof(gpu)
