"""The threaded mode of the CPU emulation detects what it claims to: toy kernels (tests/emu/toy_kernels.cpp) with and without the barrier
they need, under every thread order.  With its barrier each gives the right bytes under every order; without it, the orders named below must
give wrong ones.  Were __syncthreads() an empty function again, the kernels with a barrier would fail here under the threaded orders."""
import ctypes

import numpy as np
import pytest

from emu_lib import emu
from thread_order_cases import (ALL_ORDERS, ASCENDING, DESCENDING, GROUPS_DESCENDING, ONE_THREAD, barrier_mismatches, thread_order)

READ_NEXT, READ_PREV, READ_OTHER_WAVE, READ_THEN_OVERWRITE, TWO_GROUPS, SKIPPED_BARRIER = range(6)
N = 128                     # two wavefronts


def toy_a(i):
    return 0x1000 + 7 * i


def toy_b(i):
    return 0x900000 + 13 * i


# what each kernel must write, from its definition and not from a run of it
EXPECTED = {
    READ_NEXT: [toy_a(min(i + 1, N - 1)) for i in range(N)],
    READ_PREV: [toy_a(max(i - 1, 0)) for i in range(N)],
    READ_OTHER_WAVE: [toy_a(i ^ 64) for i in range(N)],
    READ_THEN_OVERWRITE: [toy_a(min(i + 1, N - 1)) + toy_b(i) for i in range(N)],
}


def run_toy(which, barrier, order, expect_mismatches=0):
    lib = emu()
    out = np.zeros(2 * N if which == TWO_GROUPS else N, dtype=np.uint64)
    if which == TWO_GROUPS:
        out[:N] = [toy_a(i) for i in range(N)]
    with thread_order(lib, order, expect_mismatches=expect_mismatches):
        assert lib.c.iopx_emu_toy(which, int(barrier), N, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out.tolist()


@pytest.mark.parametrize("order", sorted(ALL_ORDERS))
@pytest.mark.parametrize("which", sorted(EXPECTED))
def test_with_its_barrier_every_order_is_right(which, order):
    # (thread_order also asserts that no launch broke barrier discipline)
    assert run_toy(which, True, ALL_ORDERS[order]) == EXPECTED[which]


def test_read_next_without_barrier():
    assert run_toy(READ_NEXT, False, ASCENDING) != EXPECTED[READ_NEXT]
    assert run_toy(READ_NEXT, False, DESCENDING) == EXPECTED[READ_NEXT]


def test_read_prev_without_barrier_needs_the_descending_order():
    """Why both orders exist: ascending order runs every writer before its reader here."""
    assert run_toy(READ_PREV, False, ASCENDING) == EXPECTED[READ_PREV]
    assert run_toy(READ_PREV, False, DESCENDING) != EXPECTED[READ_PREV]


@pytest.mark.parametrize("which", [READ_OTHER_WAVE, READ_THEN_OVERWRITE])
def test_without_barrier_one_of_the_two_orders_fails(which):
    got = [run_toy(which, False, order) for order in (ASCENDING, DESCENDING)]
    assert any(g != EXPECTED[which] for g in got)


def test_one_thread_per_workgroup_sees_none_of_it():
    """Order 0, the suite's default, is unchanged: blockDim = 1, thread 0 alone.  It cannot tell a kernel from the same kernel without its
    barrier, which is the gap the other orders close."""
    for which in sorted(EXPECTED):
        assert run_toy(which, False, ONE_THREAD)[0] == run_toy(which, True, ONE_THREAD)[0]


def test_workgroup_order():
    first = [toy_a(i) + toy_b(i) for i in range(N)]
    for threads in (ONE_THREAD, ASCENDING, DESCENDING):
        assert run_toy(TWO_GROUPS, True, threads) == first + first
        assert run_toy(TWO_GROUPS, True, threads | GROUPS_DESCENDING) == first + [toy_a(i) for i in range(N)]


@pytest.mark.parametrize("order", sorted(ALL_ORDERS))
def test_skipped_barrier_is_counted(order):
    lib = emu()
    run_toy(SKIPPED_BARRIER, True, ALL_ORDERS[order], expect_mismatches=1)
    assert barrier_mismatches(lib) == 0             # reading the count cleared it
    run_toy(SKIPPED_BARRIER, True, ONE_THREAD)      # one thread per workgroup has nobody to miss


def test_orders_that_do_not_exist():
    lib = emu()
    with thread_order(lib, ONE_THREAD):
        assert lib.c.iopx_emu_set_threads(8, 0) == -1 and lib.c.iopx_emu_set_threads(-1, 0) == -1
