"""Both forms of the rational combination over gf128 and gf256, and one native Fractal proof per wide field (IOPX_GFX_FRACTAL_WIDE=1), on the CPU emulation's threaded mode (tests/thread_order_cases.py): every workgroup
with the block size of its launch, one fiber per thread, in ascending, descending and one seeded order of thread index, and with the workgroups in
descending order too; and under the deferred stream schedules of tests/stream_schedule_cases.py.  The lean form's rolled product loop carries its
phase per thread: no order of the threads may be seen in the bytes.  Expected values as in tests/gfx_fractal_wide_cases.py."""
import pytest

import gfx_aurora_cases as C
import gfx_fractal_wide_cases as FW
import stream_schedule_cases as S
import thread_order_cases as T
from emu_lib import emu

W = pytest.mark.parametrize("words", FW.WORDS, ids=lambda w: FW.NAME[w])
ORDERS = pytest.mark.parametrize("order", sorted(T.ALL_ORDERS))


@W
@ORDERS
def test_forms_under_thread_orders(words, order):
    """two ragged workgroups at one and at four rationals, and the third trip of the grid-stride loop"""
    lib = emu()
    with T.thread_order(lib, T.ALL_ORDERS[order]):
        FW.check_forms(lib, words, 1, 257)
        FW.check_forms(lib, words, 4, 257)
        FW.check_strides(lib, words)


@W
@pytest.mark.parametrize("name", S.DEFERRED)
def test_forms_under_stream_schedules(words, name):
    lib = emu()
    with S.schedule(lib, name):
        FW.check_forms(lib, words, 3, 257)
        FW.check_output_over_first_input(lib, words)


@W
@pytest.mark.parametrize("name", S.DEFERRED)
def test_native_wide_fractal_proof_under_stream_schedules(words, name):
    lib = emu()
    case = FW.NATIVE_TUPLES[0]
    want, want_roots, inst = FW.model(words, case)
    with S.schedule(lib, name):
        roots, proofs, _ = FW.native_index_and_prove(lib, words, inst, case[2], case[3], proofs=2)
    assert roots == want_roots and proofs == [want, want]


@W
def test_native_wide_fractal_proof_under_a_hostile_thread_order(words):
    """the whole proof with the threads of every workgroup in descending order (the division's LDS tree, the lean combination at gf256's default or
    behind the option): the model's bytes"""
    lib = emu()
    case = FW.NATIVE_TUPLES[0]
    want, want_roots, inst = FW.model(words, case)
    order = sorted(T.ALL_ORDERS)[1]
    with T.thread_order(lib, T.ALL_ORDERS[order]), C.options(lib, **{FW.OPTION: 2}):
        roots, proofs, _ = FW.native_index_and_prove(lib, words, inst, case[2], case[3])
    assert roots == want_roots and proofs == [want]
