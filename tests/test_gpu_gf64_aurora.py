"""Aurora over GF(2^64) on the MI355X: the cases of tests/gf64_aurora_cases.py (the CPU leg is tests/test_gf64_aurora_emu.py), and the
provers at 2^12 and 2^14 constraints against the oracle's recorded digests (tests/golden/gf64_aurora.json, written by
tools/make_gf64_aurora_digests.py): 2^14 coefficients are more than one tile of the transform, so the multi-pass phase 1 of the LDE runs inside
that proof.  No whole-transcript oracle call happens at those sizes."""
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


@pytest.mark.parametrize("log_n", [12, 14])
def test_native_prover_matches_the_recorded_digest(lib, log_n):
    C.check_native_digest(lib, log_n, 15)


def test_python_prover_matches_the_recorded_digest(lib):
    with on_torch_stream(lib) as (torch, device):
        C.check_python_digest(lib, torch, device, 12, 15)
