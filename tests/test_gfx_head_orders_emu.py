"""The entries of include/libiop_amd_head.h on the CPU emulation's threaded mode (tests/thread_order_cases.py): every workgroup with the block size
of its launch, one fiber per thread, in ascending, descending and one seeded order of thread index, and with the workgroups in descending order
too.  And one native proof per field by the head route (IOPX_GFX_HEAD_EVAL=1) under the deferred stream schedules of
tests/stream_schedule_cases.py.  Expected values as in tests/gfx_head_cases.py."""
import pytest

import gfx_batch_cases as B
import gfx_head_cases as H
import stream_schedule_cases as S
import thread_order_cases as T
from emu_lib import emu

W = pytest.mark.parametrize("words", H.WORDS, ids=lambda w: H.NAME[w])
ORDERS = pytest.mark.parametrize("order", sorted(T.ALL_ORDERS))


@W
@ORDERS
def test_entries_under_thread_orders(words, order):
    """the division at (9, 4) and in place at (5, 5), the host's Z_S (no kernel: the same values), and the two-group re-extension at (9, 5) under the
    smallest tiles (two upper passes each way) onto all cosets and a window"""
    lib = emu()
    with T.thread_order(lib, T.ALL_ORDERS[order]):
        H.check_div_by_vanishing(lib, words, 9, 4)
        H.check_div_by_vanishing(lib, words, 5, 5)
        H.check_vanishing_host(lib, words)
    m, d = 9, 5
    basis = H.oracle.standard_basis(m, words)
    shift, sa, sb = H.reextend_shifts(m, words, "prover")
    va = [H.seeded("orders a %d" % k, 1 << d, words) for k in range(3)]
    vb = [H.seeded("orders b", 1 << d, words)]
    with B.options(lib, words, tiles=B.SMALLEST_TILES):
        want = {w: B.run_reextend(lib, words, va, basis, d, sa, shift, *w)[0] + B.run_reextend(lib, words, vb, basis, d, sb, shift, *w)[0] for w in ((0, 16), (7, 2))}
        with T.thread_order(lib, T.ALL_ORDERS[order]):
            for w in want:
                B.same(H.run_reextend2(lib, words, va, vb, basis, d, sa, sb, shift, *w)[0], want[w], (order, w))


@W
@pytest.mark.parametrize("name", S.DEFERRED)
def test_native_head_proof_under_stream_schedules(words, name):
    lib = emu()
    inst = H.M.example(words, 7, 15, H.C.SEED)
    want = H.expected_transcript(words, inst)
    h = lib.aurora_instance(H.field_code(words), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
    try:
        with H.C.options(lib, **{H.OPTION: 1}), S.schedule(lib, name):
            lib.profile_begin()
            assert lib.aurora_prove(h) == want
            assert H.launches(lib.profile_report(), H.STEM[words], "div_by_vanishing") == 1
            assert lib.aurora_prove(h) == want
    finally:
        lib.aurora_instance_free(h)
