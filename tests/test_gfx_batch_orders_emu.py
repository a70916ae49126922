"""The batched kernels of libiop_amd/csrc/gfx_additive.h on the CPU emulation's threaded mode (tests/thread_order_cases.py): every workgroup with
the block size of its launch, one fiber per thread, in ascending, descending and one seeded order of thread index, and with the workgroups in
descending order too — the upper passes of a one-coset re-extension work in place on the batch's work buffer.  And one native proof per field
through the fused route under the deferred stream schedules of tests/stream_schedule_cases.py.  Expected values as in tests/gfx_batch_cases.py."""
import pytest

import gfx_batch_cases as B
import stream_schedule_cases as S
import thread_order_cases as T
from emu_lib import emu

W = pytest.mark.parametrize("words", B.WORDS, ids=lambda w: B.NAME[w])
ORDERS = pytest.mark.parametrize("order", sorted(T.ALL_ORDERS))


@W
@ORDERS
def test_transforms_under_thread_orders(words, order):
    """every entry at d_dim = 5 under the default tiles (one tile, vectors sharing it) and the smallest ones (two upper passes each way): three
    vectors and two polynomials, all cosets and a window; the single-coset case runs its upper passes in place"""
    lib = emu()
    d, m = 5, 7
    basis, shift = B.domain(m, words)
    es = B.C.elem(words, 0xABC)
    vectors = [B.seeded("orders v %d" % k, 1 << d, words) for k in range(3)]
    polys = [B.seeded("orders p %d" % k, (1 << d) - 3, words) for k in range(2)]
    padded = [B.np.concatenate([c, B.np.zeros((3, words), dtype=B.np.uint64)]) for c in polys]
    for tiles in (None, B.SMALLEST_TILES):
        with B.options(lib, words, tiles=tiles):
            coeffs = B.expected_ifft(lib, words, vectors, basis[:d], es)
            want = {w: B.expected_lde(lib, words, coeffs + padded, basis, shift, *w) for w in ((0, 4), (2, 1))}
            one = B.expected_lde(lib, words, coeffs, basis[:d], shift, 0, 1)
            with T.thread_order(lib, T.ALL_ORDERS[order]):
                B.same(B.run_ifft_batch(lib, words, vectors, basis[:d], es, in_place=True), coeffs, (order, tiles, "ifft"))
                B.same(B.run_lde_batch(lib, words, polys, basis, shift, 0, 4), want[(0, 4)][3:], (order, tiles, "lde"))
                for w in want:
                    B.same(B.run_reextend(lib, words, vectors, basis, d, es, shift, *w, polys=polys)[0], want[w], (order, tiles, w))
                B.same(B.run_reextend(lib, words, vectors, basis[:d], d, es, shift, 0, 1)[0], one, (order, tiles, "one coset"))


@W
@pytest.mark.parametrize("name", S.DEFERRED)
def test_native_proof_under_stream_schedules(words, name):
    lib = emu()
    h, want = B.native_instance(lib, words, 7, 15)
    try:
        with S.schedule(lib, name):
            assert lib.aurora_prove(h) == want
            assert lib.aurora_prove(h) == want
    finally:
        lib.aurora_instance_free(h)
