"""The fallback-path cases of test_gpu_fallback_paths.py at sizes the CPU build of the kernels takes in seconds: unfused FRI folds, the
windowed multiplicative FFT, the data-movement primitives and the Merkle leaf dispatch for misaligned sub-buffers, bit for bit against the
oracle or numpy."""
import pytest

import fold_cases as fo
import merkle_cases as mk
import movement_cases as mv
import window_cases as wc
from emu_lib import emu


@pytest.mark.parametrize("m,cs,kind", fo.ADDITIVE_EMU)
def test_unfused_fold_additive(m, cs, kind):
    fo.check_additive(emu(), m, cs, kind)


def test_unfused_fold_additive_x_in_domain():
    fo.check_additive_x_in_domain(emu(), 8, 16)


@pytest.mark.parametrize("log_n,cs,shift", fo.MULTIPLICATIVE_EMU)
def test_unfused_fold_multiplicative(log_n, cs, shift):
    fo.check_multiplicative(emu(), log_n, cs, shift)


def test_unfused_then_fused_fold_chain():
    fo.check_additive_chain(emu(), 12, 8, [4, 2, 1], 3)
    fo.check_multiplicative_chain(emu(), 12, 8, [4, 2, 1], 3)


@pytest.mark.parametrize("log_n,shift", wc.CASES_EMU)
def test_mult_fft_windows(log_n, shift):
    wc.check(emu(), log_n, shift)


def test_mult_fft_windows_argument_checks():
    wc.check_errors(emu())


def test_upload_small():
    mv.check_upload(emu())
    mv.check_upload_back_to_back(emu())


def test_memcpy_d2d_and_memset():
    mv.check_copy(emu())
    mv.check_fill(emu())


def test_deferred_read_backs_overflowing_the_arena():
    mv.check_deferred_pieces(emu())


@pytest.mark.parametrize("r,cs,L", mk.ALIGN)
def test_merkle_misaligned_pointers(r, cs, L):
    mk.check_alignments(emu(), r, cs, L)
