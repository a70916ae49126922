"""The memory contract of the GF(2^256) entries (libiop_amd/csrc/gf256.hip) and of one Python and one native gf256 FRI proof, with the
harness of tests/memory_contract_cases.py: every input in a 4096-byte frame of random non-zero bytes, every output in a frame pre-filled
with random bytes, the library under its memory-check mode (IOPX_MEM_CHECK: guards around every block it allocates, poisoned payloads), two
poison bytes, payload offsets 0 and 8 modulo 16 — at the second offset no buffer of a call is 16-byte aligned, so the entries run their
64-bit instantiations there, and under the mode the library's own tables sit at 8 modulo 16 as well.  After each call the outputs equal the
oracle's bytes, every frame is intact, the inputs read back unchanged, no guard is damaged and the bytes do not follow the poison (no read
of a temporary that was never written).  On the CPU build of the kernels and (-m gpu) on the MI355X."""
import numpy as np
import pytest

import gf256_cases as G
import memory_contract_cases as mc
import oracle

T = G.TILE_BITS
COUNTS = (1, 1000)


def _fft_rows():
    rows = []
    for d in range(0, T + 2):                   # T + 1: the smallest plan with an upper pass
        basis, shift = G.std_basis(d), G.elem((1 << 255) | 0x55)
        for count in sorted({1 << d, (1 << d) // 2 + 1}):
            def build(d=d, count=count, basis=basis, shift=shift):
                coeffs = G.seeded("mc fft %d %d" % (d, count), count)
                return mc.Case([coeffs], [oracle.additive_fft(coeffs, basis, shift)], lambda lib, i, o: lib.additive_FFT_dev(i[0], count, basis, shift, o[0], words=4))
            rows.append(mc.Row("iopx_add_fft_gf256_dev", "gf256 FFT d=%d count=%d" % (d, count), build))
    return rows


def _ifft_rows():
    rows = []
    for d in (0, 1, 6, T, T + 1):
        basis, shift = G.std_basis(d), G.elem((1 << 255) | 0x55)

        def build_inv(d=d, basis=basis, shift=shift):
            evals = G.seeded("mc ifft %d" % d, 1 << d)
            return mc.Case([evals], [oracle.additive_ifft(evals, basis, shift)], lambda lib, i, o: lib.additive_IFFT_dev(i[0], basis, shift, o[0], words=4))
        rows.append(mc.Row("iopx_add_ifft_gf256_dev", "gf256 IFFT d=%d" % d, build_inv))

        def build_inplace(d=d, basis=basis, shift=shift):
            evals = G.seeded("mc ifft in place %d" % d, 1 << d)
            return mc.Case([], [oracle.additive_ifft(evals, basis, shift)], lambda lib, i, o: lib.additive_IFFT_dev(o[0], basis, shift, o[0], words=4), init={0: evals})
        rows.append(mc.Row("iopx_add_ifft_gf256_dev", "gf256 IFFT d=%d in place" % d, build_inplace))
    return rows


def _other_rows():
    rows = []
    m, d = 12, 7
    basis, shift = G.std_basis(m), G.elem((1 << 255) | 0x55)

    def build_lde():
        coeffs = G.seeded("mc lde", (1 << d) - 3)
        return mc.Case([coeffs], [oracle.additive_fft(coeffs, basis, shift)[5 << d:8 << d]],
                       lambda lib, i, o: lib.additive_LDE_dev(i[0], coeffs.shape[0], basis, shift, 5, 3, o[0], words=4))
    rows.append(mc.Row("iopx_add_lde_gf256_dev", "gf256 LDE m=12 d=7 cosets 5..7 (direct)", build_lde))
    # the smallest coefficient dimension whose plan has an upper pass: T + 1, with 2 cosets through run_phase2_fwd_x's staging
    ds = T + 1
    bs, ss = G.std_basis(ds + 1), G.elem((1 << 255) | 3)

    def build_staged():
        coeffs = G.seeded("mc staged", (1 << T) + 1)
        return mc.Case([coeffs], [oracle.additive_fft(coeffs, bs, ss)],
                       lambda lib, i, o: lib.additive_LDE_dev(i[0], coeffs.shape[0], bs, ss, 0, 2, o[0], words=4))
    rows.append(mc.Row("iopx_add_lde_gf256_dev", "gf256 LDE m=%d d=%d cosets 0..1 (staged)" % (ds + 1, ds), build_staged))
    fb, fs = G.std_basis(10), G.elem((1 << 255) | 0x77)
    for eta in (1, 2, 3, 4):
        def build_fold(eta=eta):
            f, x = G.seeded("mc fold %d" % eta, 1 << 10), G.seeded("mc fold x", 1)[0]
            return mc.Case([f], [oracle.fri_fold_additive(f, fb, fs, 1 << eta, x)], lambda lib, i, o: lib.fri_fold_dev(i[0], fb, fs, 1 << eta, x, o[0], words=4))
        rows.append(mc.Row("iopx_fri_fold_add_gf256_dev", "gf256 fold 2^10 by 2^%d" % eta, build_fold))
    for name, degrees in (("one", [256]), ("mixed", [256, 255, 128, 129, 256]), ("bump not a power of two", [250, 233, 250 - 7])):
        def build_ldt(degrees=degrees, name=name):
            lb, ls = G.std_basis(8), G.elem((1 << 255) | 0xF0F)
            evals = [G.seeded("mc ldt %s %d" % (name, k), 256) for k in range(len(degrees))]
            coef = G.seeded("mc ldt coef " + name, 2 * len(degrees))
            return mc.Case(evals, [oracle.ldt_combine_additive(evals, degrees, coef, lb, ls)], lambda lib, i, o: lib.ldt_combine_dev(i, degrees, coef, lb, ls, o[0], words=4))
        rows.append(mc.Row("iopx_ldt_combine_gf256_dev", "gf256 ldt_combine %s" % name, build_ldt))
    for count in COUNTS:
        def build_mul(count=count):
            a, b = G.seeded("mc mul a", count), G.seeded("mc mul b", count)
            return mc.Case([a, b], [oracle.gf_mul(a, b)], lambda lib, i, o: lib.gf192_mul_dev(i[0], i[1], o[0], count, words=4))
        rows.append(mc.Row("iopx_gf256_mul_dev", "gf256 mul count=%d" % count, build_mul))

        def build_inv(count=count):
            a = G.seeded("mc inv", count) | np.uint64(1)
            return mc.Case([a], [oracle.gf_inv(a)], lambda lib, i, o: lib.field_inv_dev(i[0], o[0], count, words=4))
        rows.append(mc.Row("iopx_gf256_inv_dev", "gf256 inv count=%d" % count, build_inv))

        def build_add(count=count):
            a, b = G.seeded("mc add a", count), G.seeded("mc add b", count)
            return mc.Case([a, b], [a ^ b], lambda lib, i, o: lib.field_add_dev(i[0], i[1], o[0], count, words=4))
        rows.append(mc.Row("iopx_gf256_add_dev", "gf256 add count=%d" % count, build_add))
    return rows


ROWS = _fft_rows() + _ifft_rows() + _other_rows()
_ids = lambda r: r.name.replace(" ", "_").replace(",", "").replace("(", "").replace(")", "")      # noqa: E731


def _proofs(lib, on_gpu):
    """one Python and one native gf256 FRI proof per poison byte: the model's bytes each time"""
    import torch
    import libiop_amd as la
    from libiop_amd import domains, fri, r1cs
    t = G.FRI_SNARK_TUPLES[0]
    want = G.model_bytes(4, t)
    if on_gpu:
        lib.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for poison in mc.POISONS:
            with mc.memory_checks(lib, poison):
                ops = domains.DeviceOps(lib, torch, torch.device("cuda:0" if on_gpu else "cpu"), domains.GF256())
                coeffs = r1cs.seeded_elements(ops.field, 5, 1 << (t[0] - t[1]))
                d_coeffs = ops.upload(coeffs)
                assert fri.fri_snark_prover(ops, fri.FRISnarkParameters(*t), d_poly_coeffs=d_coeffs).serialize() == want
                assert lib.fri_snark_prove(la.FIELD_GF256, d_coeffs.data_ptr(), coeffs.shape[0], *t) == want
    finally:
        if on_gpu:
            lib.use_own_stream()


def test_every_new_entry_has_a_row():
    import libiop_amd
    new = [s for s in libiop_amd.EXPORTED_SYMBOLS if "gf256" in s and s.endswith("_dev")]
    assert len(new) == 8 and sorted(set(r.entry for r in ROWS)) == sorted(new)


@pytest.mark.parametrize("row", ROWS, ids=_ids)
def test_entries_on_the_cpu_build(row):
    from emu_lib import emu
    mc.run_row(emu(), row)


def test_proofs_on_the_cpu_build():
    from emu_lib import emu
    _proofs(emu(), False)


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_ids)
def test_entries_on_the_gpu(gpu, row):
    mc.run_row(gpu, row)


@pytest.mark.gpu
def test_proofs_on_the_gpu(gpu):
    _proofs(gpu, True)
