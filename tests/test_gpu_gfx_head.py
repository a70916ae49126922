"""Head evaluation over gf64, gf128 and gf256 on the MI355X: tests/gfx_head_cases.py through the product library (the CPU leg is
tests/test_gfx_head_emu.py)."""
import pytest

import gfx_head_cases as H

pytestmark = pytest.mark.gpu

W = pytest.mark.parametrize("words", H.WORDS, ids=lambda w: H.NAME[w])
DIV = pytest.mark.parametrize("shape", H.DIV_SHAPES, ids=lambda s: "m%d-s%d" % s)
RE = pytest.mark.parametrize("shape", H.REEXTEND_SHAPES, ids=lambda s: "m%d-d%d" % s)
CASES = pytest.mark.parametrize("case", H.NATIVE_CASES, ids=lambda c: "n%d-k%d-s%d-rs%d-l%d" % c)


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
@DIV
def test_div_by_vanishing(lib, words, shape):
    H.check_div_by_vanishing(lib, words, *shape)


def test_div_by_vanishing_construction_reproduces_gf192(lib):
    H.check_div_trust(lib)


@W
def test_div_by_vanishing_under_a_grid_cap(lib, words):
    H.check_div_grid_cap(lib, words)


@W
def test_div_by_vanishing_refusals(lib, words):
    H.check_div_refusals(lib, words)


@pytest.mark.parametrize("words", H.WORDS + (3,), ids=lambda w: {3: "gf192"}.get(w) or H.NAME[w])
def test_vanishing_host(lib, words):
    H.check_vanishing_host(lib, words)


@W
@RE
def test_reextend2(lib, words, shape):
    H.check_reextend2(lib, words, *shape)


@W
def test_reextend2_in_rounds_of_vectors(lib, words):
    H.check_reextend2_staging_rounds(lib, words)


@W
def test_reextend2_one_output_off_the_boundary(lib, words):
    H.check_reextend2_alignment(lib, words)


@W
def test_reextend2_launches(lib, words):
    H.check_reextend2_profile(lib, words)


@W
def test_reextend2_refusals(lib, words):
    H.check_reextend2_refusals(lib, words)


@W
@CASES
def test_native_prover_by_the_head_route(lib, words, case):
    H.check_native_head(lib, words, case)


@W
def test_native_prover_fewer_variables_than_constraints(lib, words):
    H.check_native_head_short_instance(lib, words)


@W
def test_unsatisfied_assignment(lib, words):
    H.check_unsatisfied(lib, words)


@W
def test_defaults_unchanged(lib, words):
    H.check_defaults_unchanged(lib, words)


@W
def test_warm_with_the_option(lib, words):
    H.check_warm_with_the_option(lib, words)


@W
def test_recorded_digest(lib, words):
    H.check_native_digest(lib, words)


def test_other_fields_after_head_proofs(lib):
    with on_torch_stream(lib) as (torch, device):
        H.check_other_fields_after_head_proofs(lib, torch, device)
