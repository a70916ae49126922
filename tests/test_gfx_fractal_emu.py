"""What the Fractal prover needs over gf64, gf128 and gf256, and the gf64 Fractal provers under IOPX_GFX_FRACTAL=1, on the CPU build of the kernels:
tests/gfx_fractal_cases.py (the GPU leg is tests/test_gpu_gfx_fractal.py)."""
import pytest

import gfx_fractal_cases as F
from emu_lib import emu

W = pytest.mark.parametrize("words", F.WORDS, ids=lambda w: F.NAME[w])
CASES = pytest.mark.parametrize("case", F.NATIVE_TUPLES, ids=lambda c: "n%d-k%d-rs%d-l%d" % c)


def _torch():
    import torch
    return torch, torch.device("cpu")


@W
@pytest.mark.parametrize("n", F.DIV_SIZES)
def test_div(words, n):
    F.check_div(emu(), words, n)


@W
def test_div_over_several_strides(words):
    F.check_div_strides(emu(), words)


@W
def test_div_root_inverted_either_way(words):
    F.check_div_inversions(emu(), words)


@W
def test_div_refusals(words):
    F.check_div_refusals(emu(), words)


@W
@pytest.mark.parametrize("m", F.OFFSETS_DIMS)
def test_domain_offsets(words, m):
    F.check_domain_offsets(emu(), words, m)


@W
@pytest.mark.parametrize("shape", F.VANISHING_SHAPES, ids=lambda s: "m%d-d%d" % s)
def test_vanishing_evals(words, shape):
    F.check_vanishing_evals(emu(), words, *shape)


@W
def test_domain_refusals(words):
    F.check_domain_refusals(emu(), words)


@W
@pytest.mark.parametrize("n", F.RATIONAL_SIZES)
@pytest.mark.parametrize("num", (1, 2, 3, 4))
def test_rational_combine(words, num, n):
    F.check_rational_combine(emu(), words, num, n)


@W
def test_rational_combine_refusals(words):
    F.check_rational_refusals(emu(), words)


@W
@pytest.mark.parametrize("shape", F.CONSTRAINT_SHAPES, ids=lambda s: "m%d-k%d" % s)
def test_rational_sumcheck_constraint(words, shape):
    F.check_constraint(emu(), words, *shape)


@W
def test_rational_sumcheck_constraint_refusals(words):
    F.check_constraint_refusals(emu(), words)


@W
def test_rational_sumcheck_constraint_after_table_turnover(words):
    F.check_constraint_table_turnover(emu(), words)


@CASES
def test_native_fractal_gf64(case):
    F.check_native_prover(emu(), case)


def test_native_fractal_gf64_second_proof_and_warm():
    F.check_native_second_proof_and_warm(emu())


def test_native_fractal_gf64_hand_built_system():
    F.check_native_hand_built(emu())


def test_native_fractal_gf64_profile():
    F.check_native_profile(emu())


def test_native_fractal_gf64_recorded_digest():
    F.check_native_digest(emu(), 10)


@pytest.mark.parametrize("case", F.PYTHON_TUPLES, ids=lambda c: "n%d-k%d-rs%d-l%d" % c)
def test_python_fractal_gf64(case):
    F.check_python_prover(emu(), *_torch(), case)


def test_refusals():
    F.check_refusals(emu(), *_torch())


def test_other_fields_unchanged():
    F.check_other_fields_unchanged(emu(), *_torch())
