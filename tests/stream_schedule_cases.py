"""Adversarial stream schedules on the CPU emulation of HIP (tests/emu/emu_runtime.cpp): what the product orders by streams and events alone
-- the side stream, the temporary pool and its quarantine, the pinned staging chunks, the deferred read-back arena, deferred roots, the
proof-of-work search in two halves -- must give the same bytes whichever legal way the streams interleave.

Schedules (iopx_emu_set_schedule): "eager" is the default of the whole suite; on "all-late" nothing executes before the host synchronises;
"main-late" / "side-late" delay one stream (creation index 0: the library's own; 1: its side stream) while the others run each operation at
once.  For any two streams these are the two extreme legal interleavings.

Only the C++ prover behind the C ABI runs here, on buffers from iopx_malloc.  The Python prover over DeviceOps keeps its data in torch CPU
tensors, which are not ordered with the emulated streams: it stays on the eager schedule, as do the communicator and gloo tests."""
import contextlib
import ctypes
import functools

import numpy as np

import bn128_aurora_cases as BA
import bn128_fri_snark_cases as BF
import movement_cases as mv
import oracle
import r1cs_general as rg
from libiop_amd import domains, r1cs

EAGER, ALL_LATE, ONE_LATE = 0, 1, 2
SCHEDULES = {"eager": (EAGER, -1), "all-late": (ALL_LATE, -1), "main-late": (ONE_LATE, 0), "side-late": (ONE_LATE, 1)}
DEFERRED = [s for s in SCHEDULES if s != "eager"]
_vp, _sz = ctypes.c_void_p, ctypes.c_size_t


def prime(lib):
    """The library's own stream is the first stream created and its side stream the second: the one-stream-late schedules go by that order."""
    lib.init(0)
    if lib.c.iopx_emu_live_streams() < 2:
        lib._check(lib.c.iopx_side_stream_begin())
        lib._check(lib.c.iopx_side_stream_end())
        lib._check(lib.c.iopx_side_stream_join())
    assert lib.c.iopx_emu_live_streams() == 2


@contextlib.contextmanager
def schedule(lib, name, late_stream=None):
    """`name` of SCHEDULES, or a (schedule, stream) pair; back to eager, with every injected fault off, on the way out (a switch drains first)."""
    prime(lib)
    sched = SCHEDULES[name] if isinstance(name, str) else name
    assert lib.c.iopx_emu_set_schedule(*sched) == 0
    try:
        yield lib
    finally:
        lib.c.iopx_emu_drop_waits(-1, -1)
        lib.c.iopx_emu_force_query_complete(0)
        assert lib.c.iopx_emu_set_schedule(EAGER, -1) == 0


def selftest(lib, which):
    lib.c.iopx_emu_selftest.restype = ctypes.c_long
    return int(lib.c.iopx_emu_selftest(int(which)))


def peek(d, nbytes):
    """Device memory as it is NOW, without a copy on any stream (the emulation's device memory is host memory)."""
    return np.frombuffer(ctypes.string_at(d, nbytes), dtype=np.uint8)


def filled(value, nbytes):
    return np.full(nbytes, value, dtype=np.uint8)


def read(lib, d, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    lib.d2h(out, d)
    return out


def pool_alloc(lib, nbytes):
    p = _vp()
    lib._check(lib.c.iopx_pool_alloc(ctypes.byref(p), _sz(nbytes)))
    return p.value


def pool_free(lib, p):
    lib._check(lib.c.iopx_pool_free(_vp(p)))


@contextlib.contextmanager
def side_section(lib):
    lib._check(lib.c.iopx_side_stream_begin())
    try:
        yield
    finally:
        lib._check(lib.c.iopx_side_stream_end())


def join(lib):
    lib._check(lib.c.iopx_side_stream_join())


# ---- b. side-stream sections through the C ABI ---------------------------------------------------------------------------------------
N = 4096 + 24


def check_section_consumes_what_the_main_stream_produced(lib):
    """Fork: the section's consumer sees what the main stream had queued before it, not what the buffer held earlier; join: the main stream's
    later reader sees the section's result, and an overwrite of the source after the join does not reach the consumer.  (Overwriting the
    source between _end and _join is a race of the caller's in HIP itself -- main stream early, side stream late, the section reads the new
    bytes -- so no schedule-independent result exists for it: DESIGN.md 8.1.)"""
    src, dst = lib.malloc(N), lib.malloc(N)
    try:
        lib.h2d(src, filled(0x01, N))
        lib.h2d(dst, filled(0x02, N))
        mv.memset_dev(lib, src, 0x11, N)                    # produced on the main stream, not waited for
        with side_section(lib):
            mv.memcpy_d2d(lib, dst, src, N)                 # consumed on the side stream
        join(lib)
        mv.memset_dev(lib, src, 0x22, N)                    # the main stream goes on
        assert np.array_equal(read(lib, dst, N), filled(0x11, N))
        assert np.array_equal(read(lib, src, N), filled(0x22, N))
    finally:
        lib.free(src)
        lib.free(dst)


def check_pool_block_freed_in_a_section_is_quarantined(lib):
    """A block freed inside a section is still read by the side stream: the pool hands it out again only after the join.  By address, and by
    contents: the main stream fills the block it got instead before the join, and the section's copy still holds the old bytes."""
    dst = lib.malloc(N)
    lib.clear_plans()                                       # an empty free list: which block fits best is then decided by this test alone
    p = pool_alloc(lib, N)
    try:
        mv.memset_dev(lib, p, 0x31, N)
        with side_section(lib):
            mv.memcpy_d2d(lib, dst, p, N)
            pool_free(lib, p)
        q = pool_alloc(lib, N)
        assert q != p, "the pool handed out a block the side stream still reads"
        mv.memset_dev(lib, q, 0x32, N)
        join(lib)
        r = pool_alloc(lib, N)
        assert r == p, "after the join the quarantined block is the best fit again"
        mv.memset_dev(lib, r, 0x33, N)
        assert np.array_equal(read(lib, dst, N), filled(0x31, N))
        assert np.array_equal(read(lib, q, N), filled(0x32, N)) and np.array_equal(read(lib, r, N), filled(0x33, N))
        pool_free(lib, q)
        pool_free(lib, r)
    finally:
        lib.free(dst)


def check_synchronize_covers_unjoined_side_work(lib):
    buf = lib.malloc(N)
    try:
        lib.h2d(buf, filled(0x03, N))
        with side_section(lib):
            mv.memset_dev(lib, buf, 0x44, N)
        lib.synchronize()
        assert np.array_equal(peek(buf, N), filled(0x44, N))
    finally:
        lib.free(buf)


def check_stream_switches_drain(lib):
    """iopx_set_stream / iopx_use_own_stream: the old stream, and unjoined side work, have executed when the call returns (the pool's blocks
    are recycled in the order of ONE stream)."""
    a, b, c = lib.malloc(N), lib.malloc(N), lib.malloc(N)
    try:
        for d in (a, b, c):
            lib.h2d(d, filled(0x04, N))
        mv.memset_dev(lib, a, 0x51, N)
        with side_section(lib):
            mv.memset_dev(lib, b, 0x52, N)
        lib.set_stream(0)                                   # the legacy stream
        try:
            assert np.array_equal(peek(a, N), filled(0x51, N)) and np.array_equal(peek(b, N), filled(0x52, N))
            mv.memset_dev(lib, c, 0x53, N)
        finally:
            lib.use_own_stream()
        assert np.array_equal(peek(c, N), filled(0x53, N))
    finally:
        for d in (a, b, c):
            lib.free(d)


def check_deferred_read_back_from_a_section(lib, end_inside):
    """A deferrable read-back queued inside a section.  iopx_defer_downloads_end after the section joins the side stream before the arena is
    copied.  Inside the section it cannot join: it is refused (IOPX_ERR_LOGIC, AssertionError here) and the window stays open, so the same
    call after the section delivers the bytes."""
    src = lib.malloc(N)
    host = filled(0x05, N + 2 * mv.PAD)
    try:
        lib.h2d(src, filled(0x06, N))
        lib.defer_downloads_begin()
        refused = False
        try:
            lib._check(lib.c.iopx_side_stream_begin())
            try:
                mv.memset_dev(lib, src, 0x61, N)
                mv.memcpy_d2h_deferrable(lib, host[mv.PAD:mv.PAD + N], src)
                if end_inside:
                    try:
                        lib._check(lib.c.iopx_defer_downloads_end())
                    except AssertionError as e:
                        refused = "side-stream section" in str(e)
            finally:
                lib._check(lib.c.iopx_side_stream_end())
        finally:
            lib.defer_downloads_end()
        assert refused == bool(end_inside)
        want = filled(0x05, N + 2 * mv.PAD)
        want[mv.PAD:mv.PAD + N] = 0x61
        assert np.array_equal(host, want)
    finally:
        lib.free(src)


# ---- c. the native provers -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_aurora(code, log_n, inputs, seed):
    return oracle.aurora_prove(code, log_n, inputs, seed)


@functools.lru_cache(maxsize=None)
def reference_fractal(code, log_n, inputs, seed):
    return oracle.fractal_prove(code, log_n, inputs, seed)


def check_aurora_and_fractal(lib):
    """tests/test_round5_env_emu.py's PROVERS, with a warmed instance and two proofs on one instance (the pool's blocks go round between them)."""
    for field, code in ((0, oracle.FIELD_GF192), (1, oracle.FIELD_EDWARDS)):
        ref = reference_aurora(code, 8, 15, 0x2204)
        inst = lib.aurora_example_instance(field, 256, 15, 255, 0x2204)
        try:
            assert lib.aurora_prove(inst) == ref
            lib.aurora_instance_warm(inst)
            assert lib.aurora_prove(inst) == ref and lib.aurora_prove(inst) == ref
        finally:
            lib.aurora_instance_free(inst)
        ref, ref_roots = reference_fractal(code, 7, 0, 0x2205)
        inst = lib.aurora_example_instance(field, 128, 0, 127, 0x2205)
        try:
            assert lib.fractal_index(inst) == ref_roots
            lib.aurora_instance_warm(inst, fractal=True)
            assert lib.fractal_prove(inst) == ref and lib.fractal_prove(inst) == ref
        finally:
            lib.aurora_instance_free(inst)


FRI_SNARKS = [("gf192", (8, 2, 2, 1, 6)), ("edwards_Fr", (8, 2, 2, 1, 6))]          # tests/test_fri_e2e_emu.py's smallest tuples; alt_bn128: BF.TUPLES[0]


@functools.lru_cache(maxsize=None)
def _fri_reference(field_name, tup):
    code, cls = {"gf192": (oracle.FIELD_GF192, domains.GF192), "edwards_Fr": (oracle.FIELD_EDWARDS, domains.EdwardsFr)}[field_name]
    dim, rs_extra, loc, interactions, queries = tup
    coeffs = np.ascontiguousarray(r1cs.seeded_elements(cls(), 5, 1 << (dim - rs_extra)), dtype=np.uint64)
    return coeffs, oracle.fri_snark_prove(code, dim, rs_extra, loc, interactions, queries, 5)


def check_fri_snarks(lib, bn128_fixture):
    for field_name, tup in FRI_SNARKS:
        coeffs, ref = _fri_reference(field_name, tup)
        d = lib.malloc(coeffs.nbytes)
        try:
            lib.h2d(d, coeffs)
            assert lib.fri_snark_prove(0 if field_name == "gf192" else 1, d, coeffs.shape[0], *tup) == ref, (field_name, tup)
        finally:
            lib.free(d)
    for hash_name in ("blake2b", "poseidon_starkware"):
        BF.check_transcript(lib, bn128_fixture, BF.TUPLES[0], hash_name)


def check_bn128_aurora(lib, fixture, hash_name, head_eval, windows):
    tup = BA.TUPLES[1]
    lib.cold_stats(reset=True)
    BA.check_digest(lib, fixture, tup, hash_name, head_eval=head_eval, windows=windows)
    assert BF.roots_read_at_round_end(lib) == (BA.num_trees(tup) if hash_name.startswith("poseidon") else 0)


@functools.lru_cache(maxsize=None)
def _general(kind):
    good = rg.generate("gf192", 64, 63, 7, 35)
    inst = good if kind is None else rg.perturbed(good, kind, 36)
    mats, z = inst.matrices, inst.assignment
    violated, *_ = oracle.r1cs_check_csr(oracle.FIELD_GF192, mats, inst.num_variables, inst.num_inputs, z)
    assert (violated == 0) == (kind is None)
    return mats, z, inst.num_variables, inst.num_inputs, oracle.aurora_prove_csr(oracle.FIELD_GF192, mats, inst.num_variables, inst.num_inputs, z)


def check_general_r1cs(lib, kind=None):
    """A general constraint system through iopx_aurora_instance_create; kind = "auxiliary": one wrong auxiliary variable, so that head
    evaluation notices on its confirmation window and falls back to the reference's schedule.  The oracle prover defines the bytes."""
    mats, z, num_variables, num_inputs, ref = _general(kind)
    for head_eval in (1, 0):
        inst = lib.aurora_instance(0, mats, num_variables, num_inputs, z)
        try:
            with BA.options(lib, IOPX_HEAD_EVAL=head_eval):
                assert lib.aurora_prove(inst) == ref, (kind, head_eval)
        finally:
            lib.aurora_instance_free(inst)


# ---- d. the child process of the mutation tests ---------------------------------------------------------------------------------------
MUTANT = r"""
import sys
import oracle
import stream_schedule_cases as S
from emu_lib import emu
lib = emu()
ref = S.reference_aurora(oracle.FIELD_GF192, 8, 15, 0x2204)
inst = lib.aurora_example_instance(0, 256, 15, 255, 0x2204)
lib.aurora_instance_warm(inst)          # the first proof's allocations are over: a hipFree would drain every stream, as on the device
assert lib.aurora_prove(inst) == ref
with S.schedule(lib, "side-late"):
    nth, on_stream = int(sys.argv[1]), int(sys.argv[2])
    if nth >= 0:
        lib.c.iopx_emu_drop_waits(nth, on_stream)
    got = lib.aurora_prove(inst)
print("same" if got == ref else "differs")
"""
