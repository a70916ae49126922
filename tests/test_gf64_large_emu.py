"""The CPU leg of tests/gf64_large_cases.py.  The host-side reference (whole-vector values built from oracle.gf_mul, short inversions and XOR, for
sizes at which the oracle's own functions take minutes) against those functions at m = 12: fz, rowcheck, both arms of sumcheck_g, the power
table.  And what the emulation can afford of the large cases themselves: fz and the zero arm of sumcheck_g at m = 21, the smallest domain with
positions at and above 2^20, and add at 2^23 + 3 elements under the block size of its launch (the default emulation runs one thread per
workgroup, so every loop there takes many trips at any size; with 256 threads the second trip starts where it does on the device)."""
import gf64_large_cases as L
import thread_order_cases as tc
from emu_lib import emu


def test_reference_matches_the_oracle_at_m12():
    L.check_reference_against_oracle(12)


def test_fz_with_index_bits_above_20():
    L.check_fz(emu(), m=21)


def test_sumcheck_g_with_index_bits_above_20():
    L.check_sumcheck_g(emu(), L.SUMCHECK_ARMS[0], m=21)


def test_add_past_the_cap_with_real_block_sizes():
    lib = emu()
    with tc.thread_order(lib, tc.ASCENDING):
        L.check_add(lib)
