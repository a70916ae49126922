"""The layout kernels (tests/layout_cases.py) on a real MI355X: gather, scatter, strided gather, interleave, row gather and the mismatch
count, each against numpy indexing inside a guarded frame, at one, three and four words per element, and once past each kernel's grid cap so
that the grid-stride loop takes a second trip."""
import pytest

import layout_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()          # raises if the HIP library is missing: no fallback
    lib.init(0)
    return lib


@pytest.mark.parametrize("kind", lc.GATHER_KINDS)
@pytest.mark.parametrize("words", lc.WORDS)
def test_gather(gpu, words, kind):
    for count in lc.COUNTS:
        lc.check_gather(gpu, count, words, kind)


def test_gather_past_the_grid_cap(gpu):
    lc.check_gather(gpu, lc.BIG_GATHER, 1, "random")


def test_gather_edges(gpu):
    lc.check_gather_edges(gpu)


@pytest.mark.parametrize("kind", lc.SCATTER_KINDS)
@pytest.mark.parametrize("words", lc.WORDS)
def test_scatter(gpu, words, kind):
    for count in lc.COUNTS:
        lc.check_scatter(gpu, count, words, kind)


def test_scatter_past_the_grid_cap(gpu):
    lc.check_scatter(gpu, lc.BIG_GATHER, 1, "random")


def test_scatter_edges(gpu):
    lc.check_scatter_edges(gpu)


@pytest.mark.parametrize("count,stride,words", lc.STRIDE_SHAPES + [lc.BIG_STRIDE])
def test_gather_stride(gpu, count, stride, words):
    lc.check_gather_stride(gpu, count, stride, words)


@pytest.mark.parametrize("parts,count,words", lc.INTERLEAVE_SHAPES + [lc.BIG_INTERLEAVE])
def test_interleave(gpu, parts, count, words):
    lc.check_interleave(gpu, parts, count, words)


@pytest.mark.parametrize("num_srcs,words,n,rows,count", lc.ROWS_SHAPES + [lc.BIG_ROWS])
def test_gather_rows(gpu, num_srcs, words, n, rows, count):
    lc.check_gather_rows(gpu, num_srcs, words, n, rows, count)


def test_gather_rows_repeated_source_and_unordered_rows(gpu):
    lc.check_gather_rows(gpu, 3, 4, 50, 9, 4, explicit=([49, 0, 7, 7], [8, 2, 0, 5]))


@pytest.mark.parametrize("words,flips,calls", lc.MISMATCH_CASES + [lc.BIG_MISMATCH])
def test_count_mismatch(gpu, words, flips, calls):
    lc.check_count_mismatch(gpu, words, flips, calls)
