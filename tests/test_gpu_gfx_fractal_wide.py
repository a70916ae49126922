"""The two forms of the rational combination over gf128 and gf256 (IOPX_GFX_RATIONAL_FORM) on the MI355X: tests/gfx_fractal_wide_cases.py through
the product library (the CPU leg is tests/test_gfx_fractal_wide_emu.py)."""
import pytest

import gfx_fractal_wide_cases as FW

pytestmark = pytest.mark.gpu

W = pytest.mark.parametrize("words", FW.WORDS, ids=lambda w: FW.NAME[w])


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


@W
@pytest.mark.parametrize("n", FW.SIZES)
@pytest.mark.parametrize("num", FW.COUNTS)
def test_rational_combine_forms(lib, words, num, n):
    FW.check_forms(lib, words, num, n)


@W
def test_rational_combine_forms_over_several_strides(lib, words):
    FW.check_strides(lib, words)


@W
def test_rational_combine_forms_zero_coefficients_and_denominators(lib, words):
    FW.check_zeros(lib, words)


@W
def test_rational_combine_forms_output_over_the_first_input(lib, words):
    FW.check_output_over_first_input(lib, words)


@W
def test_rational_combine_forms_refusals(lib, words):
    FW.check_form_refusals(lib, words)


@W
def test_rational_form_option_is_clamped(lib, words):
    FW.check_option_range(lib, words)


def test_lean_form_is_built(lib):
    FW.check_lean_form_is_built(lib)


# ---- the provers over gf128 and gf256 under IOPX_GFX_FRACTAL_WIDE=1, held to tests/gfx_fractal_model.py (which the CPU leg holds to the oracle) ----
class on_torch_stream:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        import torch
        self.lib.set_stream(torch.cuda.current_stream().cuda_stream)
        return torch, torch.device("cuda:0")

    def __exit__(self, *exc):
        self.lib.use_own_stream()


@W
@pytest.mark.parametrize("case", FW.NATIVE_TUPLES, ids=lambda c: "n%d-k%d-rs%d-l%d" % c)
def test_native_fractal(lib, words, case):
    FW.check_native_prover(lib, words, case)


@W
def test_native_fractal_hand_built_system(lib, words):
    FW.check_native_hand_built(lib, words, through_digest=True)


@W
def test_native_fractal_second_proof_and_warm(lib, words):
    FW.check_native_second_proof_and_warm(lib, words)


@W
def test_native_fractal_flipped_bit_changes_the_transcript(lib, words):
    FW.check_native_flipped_bit(lib, words)


@W
def test_python_fractal(lib, words):
    with on_torch_stream(lib) as (torch, device):
        FW.check_python_prover(lib, torch, device, words)


@W
def test_native_fractal_profile(lib, words):
    FW.check_native_profile(lib, words)


@W
def test_native_fractal_recorded_digest(lib, words):
    FW.check_native_digest(lib, words)


def test_refusals(lib):
    with on_torch_stream(lib) as (torch, device):
        FW.check_refusals(lib, torch, device)


def test_other_fields_unchanged(lib):
    with on_torch_stream(lib) as (torch, device):
        FW.check_other_fields_unchanged(lib, torch, device)
