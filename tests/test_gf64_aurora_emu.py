"""Aurora over GF(2^64) on the kernels compiled for the CPU (tests/emu): the cases of tests/gf64_aurora_cases.py.  The GPU leg is
tests/test_gpu_gf64_aurora.py."""
import pytest

import gf64_aurora_cases as C
from emu_lib import emu


def _torch():
    import torch
    return torch, torch.device("cpu")


def test_rowcheck():
    C.check_rowcheck(emu())


def test_fz():
    C.check_fz(emu())


def test_sumcheck_g():
    C.check_sumcheck_g(emu())


def test_lincheck():
    C.check_lincheck(emu())


def test_lincomb_and_affine():
    C.check_lincomb(emu())


def test_spmv():
    C.check_spmv(emu())


def test_poly_div_vanishing():
    C.check_poly_div_vanishing(emu())


def test_pow_table():
    C.check_pow_table(emu())


def test_add():
    C.check_add(emu())


def test_small_domains():
    C.check_small_domains(emu())


def test_short_vectors():
    C.check_short_vectors(emu())


def test_one_argument_off_the_boundary():
    C.check_mixed_placements(emu())


def test_output_over_an_input():
    C.check_aliased_outputs(emu())


def test_small_grid():
    C.check_small_grid(emu())


def test_domain_table_turnover():
    C.check_domain_table_turnover(emu())


def test_null_pointers_are_refused():
    C.check_null_pointers(emu())


def test_parameters_match_the_oracle():
    C.check_parameters()


@pytest.mark.parametrize("case", C.PYTHON_TUPLES, ids=lambda c: "n%d_k%d_s%x_rs%d_loc%d" % c)
def test_python_prover_transcript(case):
    C.check_python_prover(emu(), *_torch(), case)


def test_tampered_transcripts_are_rejected():
    C.check_tampering(emu(), *_torch())


def test_unsatisfied_witness():
    C.check_unsatisfied_witness(emu(), *_torch())


def test_fractal_operators_keep_raising():
    C.check_fractal_operators_refused(emu(), *_torch())


def test_other_fields_unchanged():
    C.check_other_fields_unchanged(emu(), *_torch())


@pytest.mark.parametrize("case", C.NATIVE_TUPLES, ids=lambda c: "n%d_k%d" % c)
def test_native_prover_transcript(case):
    C.check_native_prover(emu(), case)


def test_native_unsatisfied_witness():
    C.check_native_unsatisfied_witness(emu())


def test_native_fri_snark():
    C.check_native_fri_snark(emu())


def test_native_refusals():
    C.check_native_refusals(emu())


def test_native_other_fields_unchanged():
    C.check_native_other_fields_unchanged(emu())
