"""Aurora over GF(2^64) on the MI355X: the cases of tests/gf64_aurora_cases.py (the CPU leg is tests/test_gf64_aurora_emu.py), and the
provers against the oracle's recorded digests (tests/golden/gf64_aurora.json, written by tools/make_gf64_aurora_digests.py): the native prover
at 2^12, 2^14, 2^16 and 2^18 constraints, the Python prover at 2^12.  2^14 coefficients are more than one tile of the transform, so the
multi-pass phase 1 of the LDE runs inside that proof; 2^16 is the smaller of the two sizes tools/gf64_aurora_bench.py quotes; 2^18 has a
codeword of 2^24 points, so every pair-form kernel takes its second trip inside a real proof.  No whole-transcript oracle call happens at
those sizes.

Covered besides the kernels' ordinary shapes: the smallest domains (m = 0 and 1, h = 0 and m, input_dim = m, summation_dim = 0), vectors of
1, 2, 3, 511 and 513 elements, exactly one argument (each in turn, the output too) off the 16-byte boundary with the launch read from the
library's profile, the output over each input, and more domains in a row than the library keeps tables for.  The same entries past their
launch caps and the LDE over two staging groups are tests/test_gpu_gf64_large.py.

Not pinned: a proof at 2^20 constraints, the larger size the timing tool quotes (the oracle needs hours for it).  What only that size
reaches - the second trip of every grid-stride loop, index bits above 20, the later staging groups of the LDE - is what
tests/test_gpu_gf64_large.py drives directly."""
import pytest

import gf64_aurora_cases as C

pytestmark = pytest.mark.gpu


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


def test_rowcheck(lib):
    C.check_rowcheck(lib)


def test_fz(lib):
    C.check_fz(lib)


def test_sumcheck_g(lib):
    C.check_sumcheck_g(lib)


def test_lincheck(lib):
    C.check_lincheck(lib)


def test_lincomb_and_affine(lib):
    C.check_lincomb(lib)


def test_spmv(lib):
    C.check_spmv(lib)


def test_poly_div_vanishing(lib):
    C.check_poly_div_vanishing(lib)


def test_pow_table(lib):
    C.check_pow_table(lib)


def test_add(lib):
    C.check_add(lib)


def test_small_domains(lib):
    C.check_small_domains(lib)


def test_short_vectors(lib):
    C.check_short_vectors(lib)


def test_one_argument_off_the_boundary(lib):
    C.check_mixed_placements(lib)


def test_output_over_an_input(lib):
    C.check_aliased_outputs(lib)


def test_small_grid(lib):
    C.check_small_grid(lib)


def test_domain_table_turnover(lib):
    C.check_domain_table_turnover(lib)


def test_null_pointers_are_refused(lib):
    C.check_null_pointers(lib)


@pytest.mark.parametrize("case", C.PYTHON_TUPLES, ids=lambda c: "n%d_k%d_s%x_rs%d_loc%d" % c)
def test_python_prover_transcript(lib, case):
    with on_torch_stream(lib) as (torch, device):
        C.check_python_prover(lib, torch, device, case)


def test_tampered_transcripts_are_rejected(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_tampering(lib, torch, device)


def test_unsatisfied_witness(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_unsatisfied_witness(lib, torch, device)


def test_fractal_operators_keep_raising(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_fractal_operators_refused(lib, torch, device)


def test_other_fields_unchanged(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_other_fields_unchanged(lib, torch, device)


@pytest.mark.parametrize("case", C.NATIVE_TUPLES, ids=lambda c: "n%d_k%d" % c)
def test_native_prover_transcript(lib, case):
    C.check_native_prover(lib, case)


def test_native_unsatisfied_witness(lib):
    C.check_native_unsatisfied_witness(lib)


def test_native_fri_snark(lib):
    C.check_native_fri_snark(lib)


def test_native_refusals(lib):
    C.check_native_refusals(lib)


def test_native_other_fields_unchanged(lib):
    C.check_native_other_fields_unchanged(lib)


@pytest.mark.parametrize("log_n", [12, 14, 16, 18])
def test_native_prover_matches_the_recorded_digest(lib, log_n):
    C.check_native_digest(lib, log_n, 15)


def test_python_prover_matches_the_recorded_digest(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_python_digest(lib, torch, device, 12, 15)
