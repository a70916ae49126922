"""Head evaluation over gf64, gf128 and gf256 on the CPU build of the kernels: tests/gfx_head_cases.py (the GPU leg is tests/test_gpu_gfx_head.py)."""
import pytest

import gfx_head_cases as H
from emu_lib import emu

W = pytest.mark.parametrize("words", H.WORDS, ids=lambda w: H.NAME[w])
DIV = pytest.mark.parametrize("shape", H.DIV_SHAPES, ids=lambda s: "m%d-s%d" % s)
RE = pytest.mark.parametrize("shape", H.REEXTEND_SHAPES, ids=lambda s: "m%d-d%d" % s)
CASES = pytest.mark.parametrize("case", H.NATIVE_CASES, ids=lambda c: "n%d-k%d-s%d-rs%d-l%d" % c)


def _torch():
    import torch
    return torch, torch.device("cpu")


@W
@DIV
def test_div_by_vanishing(words, shape):
    H.check_div_by_vanishing(emu(), words, *shape)


def test_div_by_vanishing_construction_reproduces_gf192():
    H.check_div_trust(emu())


@W
def test_div_by_vanishing_under_a_grid_cap(words):
    H.check_div_grid_cap(emu(), words)


@W
def test_div_by_vanishing_refusals(words):
    H.check_div_refusals(emu(), words)


@pytest.mark.parametrize("words", H.WORDS + (3,), ids=lambda w: {3: "gf192"}.get(w) or H.NAME[w])
def test_vanishing_host(words):
    H.check_vanishing_host(emu(), words)


@W
@RE
def test_reextend2(words, shape):
    H.check_reextend2(emu(), words, *shape)


@W
def test_reextend2_in_rounds_of_vectors(words):
    H.check_reextend2_staging_rounds(emu(), words)


@W
def test_reextend2_one_output_off_the_boundary(words):
    H.check_reextend2_alignment(emu(), words)


@W
def test_reextend2_launches(words):
    H.check_reextend2_profile(emu(), words)


@W
def test_reextend2_refusals(words):
    H.check_reextend2_refusals(emu(), words)


@W
@CASES
def test_native_prover_by_the_head_route(words, case):
    H.check_native_head(emu(), words, case)


@W
def test_native_prover_fewer_variables_than_constraints(words):
    H.check_native_head_short_instance(emu(), words)


@W
def test_unsatisfied_assignment(words):
    H.check_unsatisfied(emu(), words)


@W
def test_defaults_unchanged(words):
    H.check_defaults_unchanged(emu(), words)


@W
def test_warm_with_the_option(words):
    H.check_warm_with_the_option(emu(), words)


def test_other_fields_after_head_proofs():
    H.check_other_fields_after_head_proofs(emu(), *_torch())
