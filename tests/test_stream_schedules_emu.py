"""The product's stream-ordered machinery under adversarial schedules of the emulated HIP streams (tests/stream_schedule_cases.py): CPU only.
a. the scheduler itself; b. the runtime's primitives and side-stream sections; c. the native provers, byte-equal to the oracle / the committed
fixtures under every schedule; d. mutations of the emulation (lost event waits, an event query that always says "complete") that b and c must
notice."""
import os
import subprocess
import sys

import pytest

import bn128_aurora_cases as BA
import bn128_fri_snark_cases as BF
import movement_cases as mv
import pow_cases as pw
import stream_schedule_cases as S
from emu_lib import emu

ALL = list(S.SCHEDULES)


# ---- a. the scheduler ----------------------------------------------------------------------------------------------------------------
# the self-tests' two streams A and B are created after the library's two: creation indices 2 and 3
A_LATE, B_LATE = (S.ONE_LATE, 2), (S.ONE_LATE, 3)


def _self(schedule, which):
    with S.schedule(emu(), schedule) as lib:
        return S.selftest(lib, which)


def test_unordered_streams_show_under_a_late_schedule():
    """A writes 5 over 1, B copies the value: no event between them, so B may read either; a launch keeps the arguments it was given."""
    assert _self("eager", 0) == 5 and _self("all-late", 0) == 1 and _self(A_LATE, 0) == 1 and _self(B_LATE, 0) == 5


@pytest.mark.parametrize("schedule", ALL + [A_LATE, B_LATE], ids=str)
def test_record_and_wait_order_two_streams(schedule):
    assert _self(schedule, 1) == 5


def test_a_wait_holds_the_record_current_at_the_call():
    """A: write 5, record, [B: wait, copy], write 7, record again; only B is synchronised.  B's copy follows the first record (5, never 1), and
    the wait pulls A up to that record and no further: x is still 5 where A is late."""
    for schedule in ("all-late", A_LATE):
        assert _self(schedule, 2) == 505
    assert _self("eager", 2) == 507
    assert _self(B_LATE, 2) == 707            # legal: A's second write is not ordered with B's copy


def test_synchronizing_one_stream_leaves_the_other_pending():
    assert _self("eager", 3) == 50905
    for schedule in ("all-late", A_LATE):
        assert _self(schedule, 3) == 10905      # x still 1 after hipStreamSynchronize(B), 5 after hipStreamSynchronize(A)


def test_pinned_copies_read_at_execution_pageable_ones_at_the_call():
    assert _self("eager", 4) == 511
    for schedule in ("all-late", A_LATE):
        assert _self(schedule, 4) == 521        # pinned source: the later 2; pageable source: 1; a pageable destination is filled at once (5)


@pytest.mark.parametrize("schedule", ALL + [A_LATE, B_LATE], ids=str)
def test_hipfree_drains_every_stream(schedule):
    assert _self(schedule, 5) == 59


def test_event_queries():
    assert _self("eager", 6) == 500005
    # not ready; three queries execute nothing (x still 1); a polling loop is let through after 64 answers in all
    assert _self("all-late", 6) == 1000000 + 100000 + 61 * 100 + 5


# ---- b. runtime primitives -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", S.DEFERRED)
def test_uploads(schedule):
    with S.schedule(emu(), schedule) as lib:
        mv.check_upload(lib)
        mv.check_upload_back_to_back(lib)


@pytest.mark.parametrize("schedule", S.DEFERRED)
def test_copies_fills_and_deferred_pieces(schedule):
    with S.schedule(emu(), schedule) as lib:
        mv.check_copy(lib)
        mv.check_fill(lib)
        mv.check_deferred_pieces(lib)


@pytest.mark.parametrize("schedule", ALL)
def test_side_stream_sections(schedule):
    with S.schedule(emu(), schedule) as lib:
        S.check_section_consumes_what_the_main_stream_produced(lib)
        S.check_pool_block_freed_in_a_section_is_quarantined(lib)
        S.check_synchronize_covers_unjoined_side_work(lib)
        S.check_stream_switches_drain(lib)


@pytest.mark.parametrize("schedule", ALL)
@pytest.mark.parametrize("end_inside", [False, True], ids=["end-after-the-section", "end-inside-the-section"])
def test_deferred_read_back_queued_in_a_section(schedule, end_inside):
    with S.schedule(emu(), schedule) as lib:
        S.check_deferred_read_back_from_a_section(lib, end_inside)


# ---- c. the native provers -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fri_fixture():
    return BF.load_fixture()


@pytest.fixture(scope="module")
def aurora_fixture():
    return BA.load_fixture()


@pytest.mark.parametrize("schedule", S.DEFERRED)
@pytest.mark.parametrize("merkle_stream,defer_roots", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_aurora_and_fractal(schedule, merkle_stream, defer_roots):
    with S.schedule(emu(), schedule) as lib, BA.options(lib, IOPX_MERKLE_STREAM=merkle_stream, IOPX_DEFER_ROOTS=defer_roots):
        S.check_aurora_and_fractal(lib)


@pytest.mark.parametrize("schedule", S.DEFERRED)
def test_fri_snarks(schedule, fri_fixture):
    with S.schedule(emu(), schedule) as lib:
        S.check_fri_snarks(lib, fri_fixture)


@pytest.mark.parametrize("schedule", S.DEFERRED)
@pytest.mark.parametrize("hash_name", ["blake2b", "poseidon_starkware"])
def test_bn128_aurora(schedule, hash_name, aurora_fixture):
    with S.schedule(emu(), schedule) as lib:
        # head evaluation and the windowed last pass, each on and off; every combination for the cheaper hash
        for head_eval, windows in ((1, 1), (0, 1), (1, 0), (0, 0)) if hash_name == "blake2b" else ((1, 1), (0, 0)):
            S.check_bn128_aurora(lib, aurora_fixture, hash_name, head_eval, windows)


@pytest.mark.parametrize("schedule", S.DEFERRED)
@pytest.mark.parametrize("kind", [None, "auxiliary"], ids=["satisfied", "wrong-auxiliary-variable"])
def test_general_r1cs(schedule, kind):
    with S.schedule(emu(), schedule) as lib:
        S.check_general_r1cs(lib, kind)


@pytest.mark.parametrize("schedule", S.DEFERRED)
def test_pow_search_in_two_halves(schedule):
    with S.schedule(emu(), schedule) as lib:
        pw.check_search_in_two_halves(lib)


# ---- d. b and c can fail -----------------------------------------------------------------------------------------------------------------
def _mutant(nth, on_stream):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    for name in ("IOPX_MERKLE_STREAM", "IOPX_DEFER_ROOTS"):
        env.pop(name, None)
    return subprocess.run([sys.executable, "-c", S.MUTANT, str(nth), str(on_stream)], env=env, cwd=root, capture_output=True, text=True, timeout=1200)


def test_the_mutation_child_reproduces_the_transcript_when_nothing_is_dropped():
    out = _mutant(-1, -1)
    assert out.returncode == 0 and out.stdout.strip().endswith("same"), out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("nth,on_stream", [(0, -1), (1, 0)], ids=["every-wait-dropped", "the-first-join-dropped"])
def test_lost_event_waits_change_the_proof(nth, on_stream):
    """Side stream late, main stream early, BLAKE2b Aurora over gf192 with its trees on the side stream.  A wrong transcript, an error or a crash
    of the child all count; the eager transcript does not.  (1, 0): only the first wait enqueued on the main stream -- the join's."""
    out = _mutant(nth, on_stream)
    assert not (out.returncode == 0 and out.stdout.strip().endswith("same")), "the schedules did not notice the lost edge"
    assert out.returncode != 0 or out.stdout.strip().endswith("differs"), out.stdout[-2000:] + out.stderr[-4000:]


def test_a_query_that_always_says_complete_breaks_back_to_back_uploads():
    with S.schedule(emu(), "all-late") as lib:
        lib.c.iopx_emu_force_query_complete(1)
        with pytest.raises(AssertionError, match="bytes differ"):
            mv.check_upload_back_to_back(lib)
    mv.check_upload_back_to_back(emu())
