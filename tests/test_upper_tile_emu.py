"""The comb upper butterfly pass (k_bfly_upper_comb: first and last level of a tile in global memory, wave-owned rows between) on the CPU-compiled
kernels, byte for byte against the oracle: tests/upper_tile_cases.py lists the shapes and which tile forms each one reaches.

Which orderings this covers.  The emulation runs a workgroup as ONE thread that takes every trip of each strided loop in turn (blockDim = 1,
tests/emu/fakehip/hip/hip_runtime.h), so within a workgroup there is one order only, the program's:
  * inside an ownership (two levels without a barrier) it is task-major: wave task 0 finishes both levels on its four rows, lane after lane,
    before task 1 starts its first.  A row-to-wave map under which a task's second level touched a row of another task's would read that
    row before its first level ran (or after both of its levels): wrong bytes, every time.  The same holds for a map that leaves a butterfly
    out or takes one twice, for a wrong global index at the first or the last level, and for a twiddle kept for a second butterfly that
    needs another.
  * between two ownerships every task has finished before the next loop starts, barrier or not: a MISSING barrier does not show here.  The
    barriers sit where upper_own's level pair changes (one place in the source); on the GPU their absence is a race that
    tests/test_gpu_upper_tile.py runs over whole tiles of eight wavefronts.
The same cases with every thread of the launch, in ascending, descending and seeded order, where a missing barrier and a row that two
wavefronts share do show: tests/test_thread_orders_emu.py.
"""
import numpy as np
import pytest

import oracle
import upper_tile_cases as uc
from emu_lib import emu


def test_pins_are_the_oracles():
    assert uc.digest(uc.ref_coset(17, "standard", 0)) == uc.PINS["fft17"]
    assert uc.digest(uc.ref_cosets(17, "standard", 1, 3)) == uc.PINS["lde17_1_3"]


def test_coset_references_are_slices_of_the_whole_codeword():
    basis, shift = uc.domain(12, "random")
    assert np.array_equal(uc.ref_cosets(12, "random", 0, 4), oracle.additive_fft(uc.coeffs(12), basis, shift))


@pytest.mark.parametrize("d,kind", [(d, "standard") for d in uc.DIMS] + [(12, "random")])
def test_forward_and_inverse(d, kind):
    uc.check_fft_ifft(emu(), d, kind)


@pytest.mark.parametrize("cb,cc", uc.LDE_COSETS)
@pytest.mark.parametrize("d,kind", [(11, "standard"), (12, "standard"), (17, "standard"), (12, "random"), (14, "random")])
def test_coset_lde(d, kind, cb, cc):
    uc.check_lde(emu(), False, d, kind, cb, cc)


def test_reextension_batch():
    uc.check_reextend(emu(), False)
