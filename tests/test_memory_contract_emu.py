"""The memory contract (tests/memory_contract_cases.py) on the CPU build: every device entry inside frames, under the library's
memory-check mode with two poison bytes; the provers under the mode; the checker against writes and reads it must notice (CPU build only);
the integer model of the prime fields' transforms against the oracle.  The device leg is tests/test_gpu_memory_contract.py."""
import ctypes

import numpy as np
import pytest

import memory_contract_cases as mc
import oracle
from emu_lib import emu


@pytest.mark.parametrize("group", sorted(mc.GROUPS))
def test_direct_entries(group):
    mc.run_group(emu(), group)


@pytest.mark.parametrize("tag", ["fp3", "bn128"])
def test_three_pass_transform(tag):
    mc.check_three_pass_fft(emu(), tag)


def test_every_dev_method_has_a_row_or_a_reason():
    mc.check_coverage(emu())


def test_the_integer_model_of_the_prime_field_transforms_is_the_oracles():
    mc.check_integer_model()


@pytest.mark.parametrize("case", sorted(mc.PROVER_CASES))
def test_provers(case):
    mc.check_prover(emu(), case)


def test_option_off_allocates_as_before():
    mc.check_mode_off_and_mixing(emu())


# ---- the checker checks itself (never on the device: these write outside a payload, inside the block's own guards) ----
def _toy(lib, what, n):
    word = ctypes.c_uint64(0)
    lib.c.iopx_emu_mem_check_toy.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    assert lib.c.iopx_emu_mem_check_toy(what, n, ctypes.byref(word)) == 0
    return word.value


@pytest.mark.parametrize("what,n,text", [(0, 1000, "tmp_alloc block of 1000 bytes: back guard damaged, first at payload offset 1000"),
                                         (0, 4099, "tmp_alloc block of 4099 bytes: back guard damaged, first at payload offset 4099"),
                                         (1, 1000, "tmp_alloc block of 1000 bytes: front guard damaged, first at payload offset -8")])
def test_a_write_outside_the_payload_is_one_recorded_violation(what, n, text):
    lib = emu()
    with pytest.raises(AssertionError, match="1 damaged guards; the first: " + text.replace("-", r"\-")):
        with mc.memory_checks(lib):
            _toy(lib, what, n)
    assert lib.mem_check_stats() == (0, 0, "")          # the context manager read and reset them


@pytest.mark.parametrize("poison", mc.POISONS)
def test_a_read_of_a_word_nobody_wrote_returns_the_poison(poison):
    lib = emu()
    with mc.memory_checks(lib, poison):
        assert _toy(lib, 2, 64) == int.from_bytes(bytes([poison]) * 8, "little")


def test_the_toy_refuses_to_run_with_the_mode_off():
    lib = emu()
    lib.init(0)
    lib.c.iopx_emu_mem_check_toy.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
    assert lib.c.iopx_emu_mem_check_toy(0, 64, None) == -1


def test_a_run_that_never_reaches_the_allocator_fails():
    with pytest.raises(AssertionError, match="never reached the allocator"):
        with mc.memory_checks(emu()):
            pass
