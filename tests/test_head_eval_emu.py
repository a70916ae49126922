"""The native provers' two schedules (libiop_amd/cpp/aurora.hpp, FRI_protocol::first_round_from_head and batch_sumcheck_protocol): virtual oracles
over the HEAD of the codeword domain only (default) and over the whole domain as the reference evaluates them (IOPX_HEAD_EVAL=0) give the
oracle prover's bytes; an instance whose virtual oracles are not polynomials (an unsatisfied witness) is detected on the confirmation window
and proved by the reference's schedule, so its (rejected) transcript is still the reference's.  Kernel sources compiled for the CPU
(tests/emu); the same cases run on the MI355X in tests/test_gpu_head_eval.py."""
import numpy as np
import pytest
import torch

import emu_lib
import head_cases as hc
import layout_cases as lc
from libiop_amd import domains, r1cs

CPU = torch.device("cpu")


@pytest.mark.parametrize("protocol,field_name,log_n,num_inputs", [("aurora", "gf192", 9, 15), ("aurora", "edwards_Fr", 9, 15), ("fractal", "gf192", 7, 15),
                                                                  ("fractal", "edwards_Fr", 8, 0)])
def test_both_schedules_give_the_oracle_transcript(protocol, field_name, log_n, num_inputs, monkeypatch):
    hc.check_both_schedules(emu_lib.emu(), monkeypatch, protocol, field_name, log_n, num_inputs)


@pytest.mark.parametrize("field_name", ["gf192", "edwards_Fr"])
def test_unsatisfied_witness_is_proved_by_the_reference_schedule(field_name, monkeypatch):
    hc.check_unsatisfied_witness(emu_lib.emu(), torch, CPU, monkeypatch, field_name)


@pytest.mark.parametrize("m,sub_dim", [(6, 2), (9, 4), (10, 7), (5, 5)])
def test_div_by_vanishing(m, sub_dim):
    hc.check_div_by_vanishing(emu_lib.emu(), torch, CPU, m, sub_dim, 40 + m)


@pytest.mark.parametrize("m,d,batch_a,batch_b,general", [(8, 5, 3, 1, False), (9, 6, 1, 1, False), (7, 6, 2, 3, False), (8, 4, 3, 1, True)])
def test_reextend_two_groups_in_one_batch(m, d, batch_a, batch_b, general):
    hc.check_reextend2(emu_lib.emu(), torch, CPU, m, d, batch_a, batch_b, 90 + m, general)


@pytest.mark.parametrize("protocol,field_name,log_n,num_inputs", [("aurora", "gf192", 8, 15), ("fractal", "edwards_Fr", 7, 0)])
def test_query_phase_behind_the_grind(protocol, field_name, log_n, num_inputs, monkeypatch):
    """The query phase enqueued behind the proof-of-work batch (IOPX_POW_BEHIND_LOG2=0: behind the very first batch, as the 2^20 proof does behind its
    2^24-candidate batch) and after the grind (the default at test sizes, whose grinds end within the short batches): the same bytes."""
    hc.check_query_phase_behind_the_grind(emu_lib.emu(), monkeypatch, protocol, field_name, log_n, num_inputs)


def test_instance_create_argument_checks():
    lib = emu_lib.emu()
    ops = domains.DeviceOps(lib, torch, CPU, domains.GF192())
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, 64, 3, 63, 5)
    mats = [hc.csr(ops, M) for M in (cs.A, cs.B, cs.C)]
    z = np.concatenate([primary, auxiliary])
    broken = [list(m) for m in mats]
    broken[1][0] = broken[1][0].copy()
    broken[1][0][3] = broken[1][0][2] - 1 if broken[1][0][2] else 7            # offsets must not decrease
    broken[1][0][0] = 0
    with pytest.raises(ValueError):
        lib.aurora_instance(0, broken, 63, 3, z)
    wide = [list(m) for m in mats]
    wide[2][1] = wide[2][1].copy()
    wide[2][1][0] = 64                                                          # column 64 > num_variables
    with pytest.raises(ValueError):
        lib.aurora_instance(0, wide, 63, 3, z)
    with pytest.raises(ValueError):
        lib.aurora_instance(9, mats, 63, 3, z)                                  # unknown field


@pytest.mark.parametrize("count,stride,words", [(1, 1, 3), (100, 8, 3), (4096, 3, 3), (257, 16, 1)])
def test_gather_stride(count, stride, words):
    """Through the shared cases (tests/layout_cases.py; more strides and the size past the grid cap: tests/test_layout_kernels_emu.py)."""
    lc.check_gather_stride(emu_lib.emu(), count, stride, words)


def test_count_mismatch():
    lc.check_count_mismatch(emu_lib.emu(), 15000, [], 1)                                              # equal buffers: zero
    lc.check_count_mismatch(emu_lib.emu(), 15000, [17 * 3 + 1, 4999 * 3 + 2, 4999 * 3], 2)            # three words differ, two calls accumulate; 12 bytes refused
