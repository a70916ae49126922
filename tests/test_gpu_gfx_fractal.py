"""What the Fractal prover needs over gf64, gf128 and gf256, and the gf64 Fractal provers under IOPX_GFX_FRACTAL=1, on the MI355X:
tests/gfx_fractal_cases.py through the product library (the CPU leg is tests/test_gfx_fractal_emu.py)."""
import pytest

import gfx_fractal_cases as F

pytestmark = pytest.mark.gpu

W = pytest.mark.parametrize("words", F.WORDS, ids=lambda w: F.NAME[w])
CASES = pytest.mark.parametrize("case", F.NATIVE_TUPLES, ids=lambda c: "n%d-k%d-rs%d-l%d" % c)


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


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
@pytest.mark.parametrize("n", F.DIV_SIZES)
def test_div(lib, words, n):
    F.check_div(lib, words, n)


@W
def test_div_over_several_strides(lib, words):
    F.check_div_strides(lib, words)


@W
def test_div_root_inverted_either_way(lib, words):
    F.check_div_inversions(lib, words)


@W
def test_div_refusals(lib, words):
    F.check_div_refusals(lib, words)


@W
@pytest.mark.parametrize("m", F.OFFSETS_DIMS)
def test_domain_offsets(lib, words, m):
    F.check_domain_offsets(lib, words, m)


@W
@pytest.mark.parametrize("shape", F.VANISHING_SHAPES, ids=lambda s: "m%d-d%d" % s)
def test_vanishing_evals(lib, words, shape):
    F.check_vanishing_evals(lib, words, *shape)


@W
def test_domain_refusals(lib, words):
    F.check_domain_refusals(lib, words)


@W
@pytest.mark.parametrize("n", F.RATIONAL_SIZES)
@pytest.mark.parametrize("num", (1, 2, 3, 4))
def test_rational_combine(lib, words, num, n):
    F.check_rational_combine(lib, words, num, n)


@W
def test_rational_combine_refusals(lib, words):
    F.check_rational_refusals(lib, words)


@W
@pytest.mark.parametrize("shape", F.CONSTRAINT_SHAPES, ids=lambda s: "m%d-k%d" % s)
def test_rational_sumcheck_constraint(lib, words, shape):
    F.check_constraint(lib, words, *shape)


@W
def test_rational_sumcheck_constraint_refusals(lib, words):
    F.check_constraint_refusals(lib, words)


@W
def test_rational_sumcheck_constraint_after_table_turnover(lib, words):
    F.check_constraint_table_turnover(lib, words)


@CASES
def test_native_fractal_gf64(lib, case):
    F.check_native_prover(lib, case)


def test_native_fractal_gf64_second_proof_and_warm(lib):
    F.check_native_second_proof_and_warm(lib)


def test_native_fractal_gf64_hand_built_system(lib):
    F.check_native_hand_built(lib)


def test_native_fractal_gf64_profile(lib):
    F.check_native_profile(lib)


@pytest.mark.parametrize("log_n", F.DIGEST_SIZES)
def test_native_fractal_gf64_recorded_digest(lib, log_n):
    F.check_native_digest(lib, log_n)


@pytest.mark.parametrize("case", F.PYTHON_TUPLES, ids=lambda c: "n%d-k%d-rs%d-l%d" % c)
def test_python_fractal_gf64(lib, case):
    with on_torch_stream(lib) as (torch, device):
        F.check_python_prover(lib, torch, device, case)


def test_refusals(lib):
    with on_torch_stream(lib) as (torch, device):
        F.check_refusals(lib, torch, device)


def test_other_fields_unchanged(lib):
    with on_torch_stream(lib) as (torch, device):
        F.check_other_fields_unchanged(lib, torch, device)
