"""Thread orders of the CPU emulation's threaded mode (tests/emu/emu_runtime.cpp, iopx_emu_set_threads), shared by the tests that use them.

Order 0 is the suite's default: one thread per workgroup.  In the others every workgroup runs with the block size of its launch, one fiber per
thread, each alone up to its next barrier: ascending and descending thread index between them run the reader of any cross-thread dependence
inside one barrier interval before its writer, and reversed workgroup order does the same for an in-place pass across tiles."""
import contextlib
import ctypes

ONE_THREAD, ASCENDING, DESCENDING, SEEDED = 0, 1, 2, 3
GROUPS_DESCENDING = 4               # added to one of the above
SEED = 0x5EED2204

THREAD_ORDERS = {"ascending": ASCENDING, "descending": DESCENDING, "seeded": SEEDED}
ALL_ORDERS = dict(THREAD_ORDERS, **{k + "-groups-descending": v | GROUPS_DESCENDING for k, v in THREAD_ORDERS.items()})


def _bind(lib):
    lib.c.iopx_emu_set_threads.argtypes = [ctypes.c_int, ctypes.c_uint64]
    lib.c.iopx_emu_set_threads.restype = ctypes.c_int
    lib.c.iopx_emu_barrier_mismatches.argtypes = []
    lib.c.iopx_emu_barrier_mismatches.restype = ctypes.c_long


def barrier_mismatches(lib):
    """Launches since the last call whose threads did not all meet at the same barriers (the call clears the count)."""
    _bind(lib)
    return int(lib.c.iopx_emu_barrier_mismatches())


@contextlib.contextmanager
def thread_order(lib, order, seed=SEED, expect_mismatches=0):
    """Every launch inside runs under `order`; the order that held before comes back whatever happens, and the launches inside must have
    kept barrier discipline (expect_mismatches=None: the caller looks at the count itself)."""
    _bind(lib)
    before = lib.c.iopx_emu_set_threads(order, seed)
    assert before >= 0, "order %r does not exist" % (order,)
    barrier_mismatches(lib)
    try:
        yield
        if expect_mismatches is not None:
            assert barrier_mismatches(lib) == expect_mismatches, "threads of one workgroup passed different barriers"
    finally:
        assert lib.c.iopx_emu_set_threads(before, seed) == order
        barrier_mismatches(lib)
