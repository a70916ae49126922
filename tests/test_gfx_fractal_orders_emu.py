"""The entries of include/libiop_amd_fractal.h on the CPU emulation's threaded mode (tests/thread_order_cases.py): every workgroup with the block size
of its launch, one fiber per thread, in ascending, descending and one seeded order of thread index, and with the workgroups in descending order
too — the batch division's LDS tree has seventeen barriers per workgroup.  And one native gf64 Fractal proof (IOPX_GFX_FRACTAL=1) under the deferred
stream schedules of tests/stream_schedule_cases.py.  Expected values as in tests/gfx_fractal_cases.py."""
import pytest

import gfx_fractal_cases as F
import stream_schedule_cases as S
import thread_order_cases as T
from emu_lib import emu

W = pytest.mark.parametrize("words", F.WORDS, ids=lambda w: F.NAME[w])
ORDERS = pytest.mark.parametrize("order", sorted(T.ALL_ORDERS))


@W
@ORDERS
def test_entries_under_thread_orders(words, order):
    """the division over two ragged workgroups and over several strides with both inversions, the two subset-sum entries, three rationals, and the
    constraint oracle on both sides of a coset per wavefront"""
    lib = emu()
    with T.thread_order(lib, T.ALL_ORDERS[order]):
        F.check_div(lib, words, 257)
        F.check_div(lib, words, 256 * 16 + 3)
        F.check_div_inversions(lib, words)
        F.check_domain_offsets(lib, words, 9)
        F.check_vanishing_evals(lib, words, 9, 4)
        F.check_rational_combine(lib, words, 3, 100)
        F.check_constraint(lib, words, 7, 5)
        F.check_constraint(lib, words, 7, 7)


@pytest.mark.parametrize("name", S.DEFERRED)
def test_native_gf64_fractal_proof_under_stream_schedules(name):
    lib = emu()
    case = F.NATIVE_TUPLES[0]
    ref, ref_roots = F.oracle_proof(case)
    with S.schedule(lib, name):
        roots, proofs, _ = F.native_index_and_prove(lib, *case, proofs=2)
    assert roots == ref_roots and proofs == [ref, ref]
