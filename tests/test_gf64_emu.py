"""The GF(2^64) kernels (libiop_amd/csrc/gf64.hip) compiled for the CPU (tests/emu) against the oracle and a pure-Python product model: the
cases of tests/gf64_cases.py.  The GPU leg is tests/test_gpu_gf64.py."""
import gf64_cases as C
from emu_lib import emu


def test_product():
    C.check_product(emu())


def test_inverse():
    C.check_inverse(emu())


def test_fft():
    C.check_fft(emu())


def test_fft_schedules():
    C.check_schedules(emu())


def test_placement_and_profile():
    C.check_placement_and_profile(emu())


def test_lde_coset_ranges():
    C.check_lde_ranges(emu())


def test_lde_upper_pass_whole():
    C.check_lde_upper_pass_whole(emu())


def test_ifft():
    C.check_ifft(emu())


def test_ifft_in_place_and_known_degree():
    C.check_ifft_in_place_and_known_degree(emu())


def test_fold():
    C.check_fold(emu())


def test_fold_chain():
    C.check_fold_chain(emu())


def test_domain_chain():
    C.check_domain_chain(emu())


def test_ldt_combination():
    C.check_ldt(emu())


def test_generic_merkle_and_query_responses_on_8_byte_elements():
    """A pin of the existing generic path (elem_bytes = 8): passes without the gf64 kernels."""
    C.check_merkle_and_queries(emu())


def test_host_and_device_forms_agree():
    C.check_host_and_device_forms(emu())


def test_argument_checks():
    C.check_argument_checks(emu())


def test_fri_snark_transcripts():
    import torch
    C.check_fri_snark(emu(), torch, torch.device("cpu"))


def test_fri_snark_other_fields_unchanged():
    import torch
    C.check_fri_snark_other_fields_unchanged(emu(), torch, torch.device("cpu"))
