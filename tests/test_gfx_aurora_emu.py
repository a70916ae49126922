"""Aurora over GF(2^128) and GF(2^256) on the kernels compiled for the CPU (tests/emu): the cases of tests/gfx_aurora_cases.py, and first of
all the trust condition of tests/gfx_aurora_model.py — at one and three words the model reproduces the oracle's prover byte for byte, its
parameters field by field and its seeded instance — since every expected transcript below is the model's.  The GPU leg is
tests/test_gpu_gfx_aurora.py.

The oracle has no verifier over these fields: tamper-rejection tests are out of scope.  The native prover is also held to the recorded digests
(2^12 constraints, a codeword of 2^17 points: tests/golden/gfx_aurora.json) here: the emulation proves that instance in a few seconds per
field, and it is the only place where the many-tile transforms run under Aurora without a GPU.  The Python prover's digest is the GPU leg's."""
import pytest

import gfx_aurora_cases as C
from emu_lib import emu

W = pytest.mark.parametrize("words", C.WORDS, ids=lambda w: C.NAME[w])


def _torch():
    import torch
    return torch, torch.device("cpu")


@pytest.mark.parametrize("words", [1, 3], ids=["gf64", "gf192"])
@pytest.mark.parametrize("tup", C.TRUST_TUPLES, ids=lambda c: "n%d_k%d_s%x_rs%d_loc%d" % c)
def test_model_reproduces_the_oracle(words, tup):
    C.check_model_reproduces_the_oracle(words, tup)


@W
def test_rowcheck(words):
    C.check_rowcheck(emu(), words)


@W
def test_fz(words):
    C.check_fz(emu(), words)


@W
def test_sumcheck_g(words):
    C.check_sumcheck_g(emu(), words)


@W
def test_lincheck(words):
    C.check_lincheck(emu(), words)


@W
def test_lincomb_and_affine(words):
    C.check_lincomb(emu(), words)


@W
def test_spmv(words):
    C.check_spmv(emu(), words)


@W
def test_poly_div_vanishing(words):
    C.check_poly_div_vanishing(emu(), words)


@W
def test_pow_table(words):
    C.check_pow_table(emu(), words)


@W
def test_add(words):
    C.check_add(emu(), words)


@W
def test_small_domains(words):
    C.check_small_domains(emu(), words)


@W
def test_short_vectors(words):
    C.check_short_vectors(emu(), words)


@W
def test_one_argument_off_the_boundary(words):
    C.check_mixed_placements(emu(), words)


@W
def test_output_over_an_input(words):
    C.check_aliased_outputs(emu(), words)


@W
def test_third_trip_of_every_loop(words):
    C.check_small_grid(emu(), words)


@W
def test_domain_table_turnover(words):
    C.check_domain_table_turnover(emu(), words)


@W
def test_null_pointers_are_refused(words):
    C.check_null_pointers(emu(), words)


@W
def test_parameters_match_the_model(words):
    C.check_parameters(words)


@pytest.mark.parametrize("words, case", [(w, c) for w in C.WORDS for c in C.PYTHON_TUPLES[w]], ids=lambda v: C.NAME[v] if isinstance(v, int) else "n%d_k%d_s%x_rs%d_loc%d" % v)
def test_python_prover_transcript(words, case):
    C.check_python_prover(emu(), *_torch(), words, case)


@W
@pytest.mark.parametrize("case", C.NATIVE_TUPLES, ids=lambda c: "n%d_k%d" % c)
def test_native_prover_transcript(words, case):
    C.check_native_prover(emu(), *_torch(), words, case)


@W
def test_unsatisfied_assignment(words):
    C.check_unsatisfied_assignment(emu(), *_torch(), words)


@W
def test_fractal_operators_keep_raising(words):
    C.check_fractal_operators_refused(emu(), *_torch(), words)


@W
def test_native_refusals(words):
    C.check_native_refusals(emu(), words)


@W
def test_native_prover_matches_the_recorded_digest(words):
    C.check_native_digest(emu(), words)


def test_other_fields_unchanged():
    C.check_other_fields_unchanged(emu(), *_torch())
