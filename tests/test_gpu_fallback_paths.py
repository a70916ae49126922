"""Kernel paths the headline proofs never reach, called through the C ABI on a real MI355X and compared bit for bit with the CPU oracle (or
with numpy bytes): unfused FRI folds over cosets of 16 and more, the windowed multiplicative FFT, the data-movement primitives, the Merkle leaf
dispatch for misaligned sub-buffers, and LDT combines over many workgroups.  Each path is reached by its input shape alone."""
import pytest

import fold_cases as fo
import ldt_cases as lc
import merkle_cases as mk
import movement_cases as mv
import window_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()          # raises if the HIP library is missing: no fallback
    lib.init(0)
    return lib


# ---- unfused FRI folds (k_fri_fold2 / k_fri_fold2_mul) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,cs,kind", fo.ADDITIVE)
def test_unfused_fold_additive(gpu, m, cs, kind):
    fo.check_additive(gpu, m, cs, kind)


@pytest.mark.parametrize("m,cs", [(8, 16), (12, 256)])
def test_unfused_fold_additive_x_in_domain(gpu, m, cs):
    fo.check_additive_x_in_domain(gpu, m, cs)


@pytest.mark.parametrize("log_n,cs,shift", fo.MULTIPLICATIVE)
def test_unfused_fold_multiplicative(gpu, log_n, cs, shift):
    fo.check_multiplicative(gpu, log_n, cs, shift)


def test_unfused_then_fused_fold_chain(gpu):
    fo.check_additive_chain(gpu, 12, 8, [4, 2, 1], 3)
    fo.check_multiplicative_chain(gpu, 12, 8, [4, 2, 1], 3)


def test_unfused_then_fused_fold_chain_keeps_low_degree_at_2p20(gpu):
    fo.check_additive_chain(gpu, 20, 16, [5, 3], 4, low_degree_only=True)
    fo.check_multiplicative_chain(gpu, 20, 16, [5, 3], 4, low_degree_only=True)


# ---- windowed multiplicative FFT (iopx_mul_fft_fp3_windows_dev) --------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,shift", wc.CASES)
def test_mult_fft_windows(gpu, log_n, shift):
    wc.check(gpu, log_n, shift)


def test_mult_fft_windows_argument_checks(gpu):
    wc.check_errors(gpu)
    wc.check_errors(gpu, log_n=13)


# ---- data movement (runtime.hip) -----------------------------------------------------------------------------------------------------------
def test_upload_small(gpu):
    mv.check_upload(gpu)


def test_upload_small_back_to_back(gpu):
    mv.check_upload_back_to_back(gpu)


def test_memcpy_d2d(gpu):
    mv.check_copy(gpu)


def test_memcpy_d2d_past_the_grid_cap(gpu):
    mv.check_big_copy(gpu)


def test_memset_dev(gpu):
    mv.check_fill(gpu)


def test_deferred_read_backs_overflowing_the_arena(gpu):
    mv.check_deferred_pieces(gpu)


# ---- Merkle leaves of misaligned sub-buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,cs,L", mk.ALIGN)
def test_merkle_misaligned_pointers(gpu, r, cs, L):
    mk.check_alignments(gpu, r, cs, L)


# ---- LDT combine over many workgroups --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,degrees,seed,kind", lc.ADDITIVE_LARGE)
def test_ldt_combine_many_gaps_at_2p14(gpu, m, degrees, seed, kind):
    lc.check_additive(gpu, m, degrees, seed, kind)


@pytest.mark.parametrize("log_n,degrees,seed,shifted", lc.MULTIPLICATIVE_LARGE)
def test_ldt_combine_multiplicative_twenty_degrees(gpu, log_n, degrees, seed, shifted):
    lc.check_multiplicative(gpu, log_n, degrees, seed, shifted)
