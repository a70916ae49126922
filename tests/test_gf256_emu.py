"""The GF(2^256) kernels (libiop_amd/csrc/gf256.hip) compiled for the CPU (tests/emu) against the oracle and a pure-Python product model: the
cases of tests/gf256_cases.py.  The GPU leg is tests/test_gpu_gf256.py."""
import pytest

import gf256_cases as C
from emu_lib import emu


def test_product():
    C.check_product(emu())


def test_inverse():
    C.check_inverse(emu())


def test_fft():
    C.check_fft(emu())


def test_fft_schedules():
    C.check_schedules(emu())


def test_lde_coset_ranges():
    C.check_lde_ranges(emu())


def test_lde_upper_pass_whole():
    C.check_lde_upper_pass_whole(emu())


def test_ifft():
    C.check_ifft(emu())


def test_ifft_in_place_and_known_degree():
    C.check_ifft_in_place_and_known_degree(emu())


def test_access_paths_by_alignment():
    C.check_alignment(emu())


def test_fold():
    C.check_fold(emu())


def test_fold_chain():
    C.check_fold_chain(emu())


def test_domain_chain():
    C.check_domain_chain(emu())


def test_ldt_combination():
    C.check_ldt(emu())


def test_generic_merkle_and_query_responses_on_32_byte_binary_elements():
    """The generic path at elem_bytes = 32 on raw binary words (until now only alt_bn128 Fr's Montgomery words went through it)."""
    C.check_merkle_and_queries(emu())


def test_host_and_device_forms_agree():
    C.check_host_and_device_forms(emu())


def test_argument_checks():
    C.check_argument_checks(emu())


def test_model_reproduces_the_oracle_prover():
    """the trust condition of tests/gf128_fri_snark_model.py, at one and three words"""
    emu()                               # builds the oracle's neighbours; the model itself needs only `oracle`
    C.check_model_reproduces_oracle()


@pytest.mark.parametrize("k", range(len(C.FRI_SNARK_TUPLES)))
def test_fri_snark_transcripts(k):
    import torch
    C.check_fri_snark(emu(), torch, torch.device("cpu"), trust=(k == 0), tuples=[k])      # the trust condition is re-checked once, before the first tuple


def test_native_refusals():
    import torch
    C.check_native_refusals(emu(), torch, torch.device("cpu"))


def test_dispatch_of_the_other_fields_is_unchanged():
    import torch
    C.check_dispatch_guard(emu(), torch, torch.device("cpu"))
