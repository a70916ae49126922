"""The GF(2^256) kernels (libiop_amd/csrc/gf256.hip) on the MI355X: the cases of tests/gf256_cases.py against the oracle, the pure-Python
product model and the FRI SNARK model of tests/gf128_fri_snark_model.py at four words (the CPU leg is tests/test_gf256_emu.py)."""
import pytest

import gf256_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


def _on_torch_stream(lib, check):
    import torch
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        check(lib, torch, torch.device("cuda:0"))
    finally:
        lib.use_own_stream()


def test_product(lib):
    C.check_product(lib)


def test_inverse(lib):
    C.check_inverse(lib)


def test_fft(lib):
    C.check_fft(lib)


def test_fft_schedules(lib):
    C.check_schedules(lib)


def test_lde_coset_ranges(lib):
    C.check_lde_ranges(lib)


def test_lde_upper_pass_whole(lib):
    C.check_lde_upper_pass_whole(lib)


def test_ifft(lib):
    C.check_ifft(lib)


def test_ifft_in_place_and_known_degree(lib):
    C.check_ifft_in_place_and_known_degree(lib)


def test_access_paths_by_alignment(lib):
    C.check_alignment(lib)


def test_fold(lib):
    C.check_fold(lib)


def test_fold_chain(lib):
    C.check_fold_chain(lib)


def test_domain_chain(lib):
    C.check_domain_chain(lib)


def test_ldt_combination(lib):
    C.check_ldt(lib)


def test_generic_merkle_and_query_responses_on_32_byte_binary_elements(lib):
    """The generic path at elem_bytes = 32 on raw binary words (until now only alt_bn128 Fr's Montgomery words went through it)."""
    C.check_merkle_and_queries(lib)


def test_host_and_device_forms_agree(lib):
    C.check_host_and_device_forms(lib)


def test_argument_checks(lib):
    C.check_argument_checks(lib)


@pytest.mark.parametrize("k", range(len(C.FRI_SNARK_TUPLES)))
def test_fri_snark_transcripts(lib, k):
    _on_torch_stream(lib, lambda *a: C.check_fri_snark(*a, trust=False, tuples=[k]))      # the model's trust condition: tests/test_gf256_emu.py


def test_native_refusals(lib):
    _on_torch_stream(lib, C.check_native_refusals)


def test_dispatch_of_the_other_fields_is_unchanged(lib):
    _on_torch_stream(lib, C.check_dispatch_guard)
