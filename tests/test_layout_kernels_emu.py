"""The layout kernels (tests/layout_cases.py) with the product sources compiled for the CPU; the same cases run on the MI355X in
tests/test_gpu_layout_kernels.py, past-the-grid-cap sizes included."""
import pytest

import layout_cases as lc
from emu_lib import emu


@pytest.mark.parametrize("kind", lc.GATHER_KINDS)
@pytest.mark.parametrize("words", lc.WORDS)
def test_gather(words, kind):
    for count in lc.COUNTS:
        lc.check_gather(emu(), count, words, kind)


def test_gather_past_the_grid_cap():
    lc.check_gather(emu(), lc.BIG_GATHER, 1, "random")


def test_gather_edges():
    lc.check_gather_edges(emu())


@pytest.mark.parametrize("kind", lc.SCATTER_KINDS)
@pytest.mark.parametrize("words", lc.WORDS)
def test_scatter(words, kind):
    for count in lc.COUNTS:
        lc.check_scatter(emu(), count, words, kind)


def test_scatter_past_the_grid_cap():
    lc.check_scatter(emu(), lc.BIG_GATHER, 1, "random")


def test_scatter_edges():
    lc.check_scatter_edges(emu())


@pytest.mark.parametrize("count,stride,words", lc.STRIDE_SHAPES + [lc.BIG_STRIDE])
def test_gather_stride(count, stride, words):
    lc.check_gather_stride(emu(), count, stride, words)


@pytest.mark.parametrize("parts,count,words", lc.INTERLEAVE_SHAPES + [lc.BIG_INTERLEAVE])
def test_interleave(parts, count, words):
    lc.check_interleave(emu(), parts, count, words)


@pytest.mark.parametrize("num_srcs,words,n,rows,count", lc.ROWS_SHAPES + [lc.BIG_ROWS])
def test_gather_rows(num_srcs, words, n, rows, count):
    lc.check_gather_rows(emu(), num_srcs, words, n, rows, count)


def test_gather_rows_repeated_source_and_unordered_rows():
    lc.check_gather_rows(emu(), 3, 4, 50, 9, 4, explicit=([49, 0, 7, 7], [8, 2, 0, 5]))


@pytest.mark.parametrize("words,flips,calls", lc.MISMATCH_CASES + [lc.BIG_MISMATCH])
def test_count_mismatch(words, flips, calls):
    lc.check_count_mismatch(emu(), words, flips, calls)
