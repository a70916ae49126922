"""The two forms of the rational combination over gf128 and gf256 (IOPX_GFX_RATIONAL_FORM) on the CPU build of the kernels:
tests/gfx_fractal_wide_cases.py (the GPU leg is tests/test_gpu_gfx_fractal_wide.py)."""
import pytest

import gfx_fractal_wide_cases as FW
from emu_lib import emu

W = pytest.mark.parametrize("words", FW.WORDS, ids=lambda w: FW.NAME[w])


@W
@pytest.mark.parametrize("n", FW.SIZES)
@pytest.mark.parametrize("num", FW.COUNTS)
def test_rational_combine_forms(words, num, n):
    FW.check_forms(emu(), words, num, n)


@W
def test_rational_combine_forms_over_several_strides(words):
    FW.check_strides(emu(), words)


@W
def test_rational_combine_forms_zero_coefficients_and_denominators(words):
    FW.check_zeros(emu(), words)


@W
def test_rational_combine_forms_output_over_the_first_input(words):
    FW.check_output_over_first_input(emu(), words)


@W
def test_rational_combine_forms_refusals(words):
    FW.check_form_refusals(emu(), words)


@W
def test_rational_form_option_is_clamped(words):
    FW.check_option_range(emu(), words)


def test_lean_form_is_built():
    FW.check_lean_form_is_built(emu())


# ---- the model, then the provers over gf128 and gf256 under IOPX_GFX_FRACTAL_WIDE=1 ----
def _torch():
    import torch
    return torch, torch.device("cpu")


TUPLE_IDS = lambda c: "n%d-k%d-rs%d-l%d" % c      # noqa: E731


@pytest.mark.parametrize("words", FW.TRUST_WORDS, ids=lambda w: "w%d" % w)
@pytest.mark.parametrize("case", FW.TRUST_TUPLES, ids=TUPLE_IDS)
def test_model_reproduces_the_oracle(words, case):
    FW.check_model_reproduces_the_oracle(words, case)


@pytest.mark.parametrize("words", FW.TRUST_WORDS, ids=lambda w: "w%d" % w)
def test_model_reproduces_the_oracle_on_the_hand_built_system(words):
    FW.check_model_hand_built(words)


@W
@pytest.mark.parametrize("case", FW.NATIVE_TUPLES, ids=TUPLE_IDS)
def test_native_fractal(words, case):
    FW.check_native_prover(emu(), words, case)


@W
def test_native_fractal_hand_built_system(words):
    FW.check_native_hand_built(emu(), words)


@W
def test_recorded_hand_built_digests_are_the_models(words):
    FW.check_hand_built_digests_are_the_models(words)


@W
def test_native_fractal_second_proof_and_warm(words):
    FW.check_native_second_proof_and_warm(emu(), words)


@W
def test_native_fractal_flipped_bit_changes_the_transcript(words):
    FW.check_native_flipped_bit(emu(), words)


@W
def test_python_fractal(words):
    FW.check_python_prover(emu(), *_torch(), words)


@W
def test_native_fractal_profile(words):
    FW.check_native_profile(emu(), words)


@W
def test_native_fractal_recorded_digest(words):
    FW.check_native_digest(emu(), words)


def test_refusals():
    FW.check_refusals(emu(), *_torch())


def test_other_fields_unchanged():
    FW.check_other_fields_unchanged(emu(), *_torch())
