"""Aurora over GF(2^128) and GF(2^256) on the MI355X: the cases of tests/gfx_aurora_cases.py (the CPU leg, tests/test_gfx_aurora_emu.py, also
holds the trust condition of the model the expected transcripts come from), and the provers against the recorded digests
(tests/golden/gfx_aurora.json, written by tools/make_gfx_aurora_digests.py): the native prover over both fields and the Python prover
over gf128 at 2^12 constraints, a codeword of 2^17 points — many tiles of the transform.

Covered besides the kernels' ordinary shapes: the smallest domains (m = 0 and 1, h = 0 and m, input_dim = m, summation_dim = 0), vectors of
1, 2, 3, 255, 257, 511 and 513 elements, exactly one argument (each in turn, the output too) off the 16-byte boundary with the form that ran
read from the library's profile, the output over each input, the third trip of every grid-stride loop under a small grid cap, and more
domains in a row than the library keeps tables for.

The oracle has no verifier over these fields: tamper-rejection tests are out of scope."""
import pytest

import gfx_aurora_cases as C

pytestmark = pytest.mark.gpu

W = pytest.mark.parametrize("words", C.WORDS, ids=lambda w: C.NAME[w])


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
def test_rowcheck(lib, words):
    C.check_rowcheck(lib, words)


@W
def test_fz(lib, words):
    C.check_fz(lib, words)


@W
def test_sumcheck_g(lib, words):
    C.check_sumcheck_g(lib, words)


@W
def test_lincheck(lib, words):
    C.check_lincheck(lib, words)


@W
def test_lincomb_and_affine(lib, words):
    C.check_lincomb(lib, words)


@W
def test_spmv(lib, words):
    C.check_spmv(lib, words)


@W
def test_poly_div_vanishing(lib, words):
    C.check_poly_div_vanishing(lib, words)


@W
def test_pow_table(lib, words):
    C.check_pow_table(lib, words)


@W
def test_add(lib, words):
    C.check_add(lib, words)


@W
def test_small_domains(lib, words):
    C.check_small_domains(lib, words)


@W
def test_short_vectors(lib, words):
    C.check_short_vectors(lib, words)


@W
def test_one_argument_off_the_boundary(lib, words):
    C.check_mixed_placements(lib, words)


@W
def test_output_over_an_input(lib, words):
    C.check_aliased_outputs(lib, words)


@W
def test_third_trip_of_every_loop(lib, words):
    C.check_small_grid(lib, words)


@W
def test_domain_table_turnover(lib, words):
    C.check_domain_table_turnover(lib, words)


@W
def test_null_pointers_are_refused(lib, words):
    C.check_null_pointers(lib, words)


@pytest.mark.parametrize("words, case", [(w, c) for w in C.WORDS for c in C.PYTHON_TUPLES[w]], ids=lambda v: C.NAME[v] if isinstance(v, int) else "n%d_k%d_s%x_rs%d_loc%d" % v)
def test_python_prover_transcript(lib, words, case):
    with on_torch_stream(lib) as (torch, device):
        C.check_python_prover(lib, torch, device, words, case)


@W
@pytest.mark.parametrize("case", C.NATIVE_TUPLES, ids=lambda c: "n%d_k%d" % c)
def test_native_prover_transcript(lib, words, case):
    with on_torch_stream(lib) as (torch, device):
        C.check_native_prover(lib, torch, device, words, case)


@W
def test_unsatisfied_assignment(lib, words):
    with on_torch_stream(lib) as (torch, device):
        C.check_unsatisfied_assignment(lib, torch, device, words)


@W
def test_fractal_operators_keep_raising(lib, words):
    with on_torch_stream(lib) as (torch, device):
        C.check_fractal_operators_refused(lib, torch, device, words)


@W
def test_native_refusals(lib, words):
    C.check_native_refusals(lib, words)


def test_other_fields_unchanged(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_other_fields_unchanged(lib, torch, device)


@W
def test_native_prover_matches_the_recorded_digest(lib, words):
    C.check_native_digest(lib, words)


def test_python_prover_matches_the_recorded_digest(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_python_digest(lib, torch, device, 2)
