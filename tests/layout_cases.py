"""The index-arithmetic kernels that move elements between layouts, called directly through the C ABI: iopx_gather_dev / iopx_scatter_dev /
iopx_gather_stride_dev / iopx_count_mismatch_dev (prover_support.hip: k_gather_words, k_scatter_words, k_gather_stride_words,
k_count_mismatch_words; grids capped at 16384 blocks of 256) and iopx_interleave_dev / iopx_gather_rows_dev (comm.hip: k_interleave capped at
4096 blocks, k_gather_rows at 1024).  Shared by the CPU-emulation and GPU suites.  The expected value is always numpy indexing; every
destination sits between guard bytes, on a random pattern that the bytes outside the written elements must keep.  Element sizes: 8, 24 and
32 bytes (one, three and four words: gf64, gf192 / the 181-bit field, alt_bn128 Fr / digests)."""
import ctypes

import numpy as np
import pytest

from movement_cases import PAD, Guarded

_vp, _sz = ctypes.c_void_p, ctypes.c_size_t
WORDS = (1, 3, 4)
COUNTS = (1, 255, 256, 257)
CAP_16384 = 16384 * 256            # work items one trip of k_gather_words / k_scatter_words / k_gather_stride_words / k_count_mismatch_words covers
CAP_4096 = 4096 * 256              # k_interleave
CAP_1024 = 1024 * 256              # k_gather_rows

GATHER_KINDS = ("random", "identity", "reversal", "last")
SCATTER_KINDS = ("random", "identity", "reversal")
BIG_GATHER = CAP_16384 + 3         # 8-byte elements: 32 MiB of destination, the largest buffer of this module
STRIDE_SHAPES = [(1, 1, 3), (100, 8, 3), (4096, 3, 3), (257, 16, 1),          # (count, stride, words); the first four: the shapes this kernel was first tested at
                 (255, 1, 4), (256, 1, 1), (257, 5, 4), (100, 7, 1)]
BIG_STRIDE = (CAP_16384 // 3 + 2, 1, 3)                                         # count * words = cap + 2
INTERLEAVE_SHAPES = [(p, c, w) for p in (1, 2, 8) for c in (1, 255, 257) for w in WORDS] + [(4, 37, 3)]
BIG_INTERLEAVE = (2, CAP_4096 // 6 + 1, 3)                                      # parts * count * words = cap + 2
ROWS_SHAPES = [(1, 3, 50, 9, 4), (3, 4, 50, 9, 4), (3, 3, 300, 400, 257), (1, 4, 300, 400, 255)]     # (sources, words, source length, rows, count)
BIG_ROWS = (3, 4, 1000, CAP_1024 // 12 + 100, CAP_1024 // 12 + 2)              # count * sources * words = cap + 24


def _u64(seed, *shape):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 2**64, size=shape, dtype=np.uint64)


class _Dev:
    """Device copies of host arrays, freed together."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.lib.malloc(max(arr.nbytes, 8))
        self.ptrs.append(d)
        if arr.nbytes:
            self.lib.h2d(d, arr)
        return d

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.ptrs:
            self.lib.free(d)


def _gather(lib, d_src, d_index, count, elem_bytes, d_dst):
    lib.c.iopx_gather_dev.argtypes = [_vp, _vp, _sz, _sz, _vp]
    lib._check(lib.c.iopx_gather_dev(d_src, d_index, count, elem_bytes, d_dst))


def _scatter(lib, d_src, d_index, count, elem_bytes, d_dst):
    lib.c.iopx_scatter_dev.argtypes = [_vp, _vp, _sz, _sz, _vp]
    lib._check(lib.c.iopx_scatter_dev(d_src, d_index, count, elem_bytes, d_dst))


def _gather_stride(lib, d_src, count, stride, elem_bytes, d_dst):
    lib.c.iopx_gather_stride_dev.argtypes = [_vp, _sz, _sz, _sz, _vp]
    lib._check(lib.c.iopx_gather_stride_dev(d_src, count, stride, elem_bytes, d_dst))


def _interleave(lib, d_src, parts, count, elem_bytes, d_dst):
    lib.c.iopx_interleave_dev.argtypes = [_vp, _sz, _sz, _sz, _vp]
    lib._check(lib.c.iopx_interleave_dev(d_src, parts, count, elem_bytes, d_dst))


def _gather_rows(lib, ptrs, num_srcs, elem_bytes, src_index, dst_row, count, d_out):
    lib.c.iopx_gather_rows_dev.argtypes = [_vp, _sz, _sz, _vp, _vp, _sz, _vp]
    lib._check(lib.c.iopx_gather_rows_dev(ptrs, num_srcs, elem_bytes, src_index.ctypes.data, dst_row.ctypes.data, count, d_out))


def _count_mismatch(lib, d_a, d_b, nbytes, d_count):
    lib.c.iopx_count_mismatch_dev.argtypes = [_vp, _vp, _sz, _vp]
    lib._check(lib.c.iopx_count_mismatch_dev(d_a, d_b, nbytes, d_count))


def _as_bytes(arr):
    return np.ascontiguousarray(arr).view(np.uint8).reshape(-1)


# ---- iopx_gather_dev: dst[i] = src[index[i]] ----------------------------------------------------------------------------------------------
def _gather_index(kind, count, n_src, seed):
    if kind == "random":
        return np.random.Generator(np.random.PCG64(seed)).integers(0, n_src, size=count, dtype=np.uint64)       # n_src < count: repeats
    if kind == "identity":
        return np.arange(count, dtype=np.uint64)
    if kind == "reversal":
        return np.arange(count, dtype=np.uint64)[::-1].copy()
    return np.full(count, n_src - 1, dtype=np.uint64)


def check_gather(lib, count, words, kind):
    n_src = count if kind in ("identity", "reversal") else max(2, min(count // 2 + 1, 1000))
    src, index = _u64(count + words, n_src, words), _gather_index(kind, count, n_src, 5 * count + words)
    g = Guarded(lib, count * words * 8, count + 7)
    with _Dev(lib) as dev:
        try:
            _gather(lib, dev.put(src), dev.put(index), count, words * 8, g.dst(0))
            g.expect(0, _as_bytes(src[index.astype(np.int64)]))
            g.check("gather of %d elements of %d words, %s indices" % (count, words, kind))
        finally:
            g.free()


def check_gather_edges(lib):
    """count == 0 leaves the destination alone; element sizes that are no multiple of 8 bytes are refused, and write nothing."""
    src, index = _u64(1, 16, 3), np.arange(16, dtype=np.uint64)
    g = Guarded(lib, 16 * 24, 3)
    with _Dev(lib) as dev:
        try:
            d_src, d_index = dev.put(src), dev.put(index)
            _gather(lib, d_src, d_index, 0, 24, g.dst(0))
            for bad in (0, 12, 20):
                with pytest.raises(ValueError):
                    _gather(lib, d_src, d_index, 16, bad, g.dst(0))
            g.check("gather of nothing")
        finally:
            g.free()


# ---- iopx_scatter_dev: dst[index[i]] = src[i] ---------------------------------------------------------------------------------------------
def check_scatter(lib, count, words, kind):
    """The indices are distinct (a permutation of a larger range, cut to `count`): duplicates would be a write race."""
    n_dst = count + count // 2 + 5
    if kind == "random":
        index = np.random.Generator(np.random.PCG64(3 * count + words)).permutation(n_dst)[:count].astype(np.uint64)
    elif kind == "identity":
        index = np.arange(count, dtype=np.uint64)
    else:
        index = (n_dst - 1 - np.arange(count)).astype(np.uint64)
    src = _u64(count + 10 * words, count, words)
    g = Guarded(lib, n_dst * words * 8, count + 11)
    with _Dev(lib) as dev:
        try:
            _scatter(lib, dev.put(src), dev.put(index), count, words * 8, g.dst(0))
            frame = g.image[PAD:PAD + n_dst * words * 8].view(np.uint64).reshape(n_dst, words)        # untouched elements keep their pattern
            frame[index.astype(np.int64)] = src
            g.check("scatter of %d elements of %d words, %s indices" % (count, words, kind))
        finally:
            g.free()


def check_scatter_edges(lib):
    src, index = _u64(2, 16, 3), np.arange(16, dtype=np.uint64)
    g = Guarded(lib, 16 * 24, 4)
    with _Dev(lib) as dev:
        try:
            d_src, d_index = dev.put(src), dev.put(index)
            _scatter(lib, d_src, d_index, 0, 24, g.dst(0))
            for bad in (0, 12, 20):
                with pytest.raises(ValueError):
                    _scatter(lib, d_src, d_index, 16, bad, g.dst(0))
            g.check("scatter of nothing")
        finally:
            g.free()


# ---- iopx_gather_stride_dev: dst[i] = src[i * stride] -------------------------------------------------------------------------------------
def check_gather_stride(lib, count, stride, words):
    src = _u64(count + stride, (count - 1) * stride + 6, words)
    g = Guarded(lib, count * words * 8, count + 13)
    with _Dev(lib) as dev:
        try:
            d_src = dev.put(src)
            _gather_stride(lib, d_src, count, stride, words * 8, g.dst(0))
            g.expect(0, _as_bytes(src[:(count - 1) * stride + 1:stride]))
            g.check("strided gather of %d elements of %d words, stride %d" % (count, words, stride))
            with pytest.raises(ValueError):
                _gather_stride(lib, d_src, count, 0, words * 8, g.dst(0))
            with pytest.raises(ValueError):
                _gather_stride(lib, d_src, count, stride, 12, g.dst(0))
            _gather_stride(lib, d_src, 0, stride, words * 8, g.dst(0))
            g.check("refused strided gathers")
        finally:
            g.free()


# ---- iopx_interleave_dev: dst[i * parts + r] = src[r * count + i] -------------------------------------------------------------------------
def check_interleave(lib, parts, count, words):
    src = _u64(parts + count + words, parts, count, words)
    g = Guarded(lib, src.nbytes, count + 17)
    with _Dev(lib) as dev:
        try:
            d_src = dev.put(src)
            _interleave(lib, d_src, parts, count, words * 8, g.dst(0))
            g.expect(0, _as_bytes(src.transpose(1, 0, 2)))
            g.check("interleave of %d parts of %d elements of %d words" % (parts, count, words))
            with pytest.raises(ValueError):
                _interleave(lib, d_src, parts, count, words * 8, d_src)             # in place
            with pytest.raises(ValueError):
                _interleave(lib, d_src, parts, count, 12, g.dst(0))
            _interleave(lib, d_src, parts, 0, words * 8, g.dst(0))
            g.check("refused interleaves")
        finally:
            g.free()


# ---- iopx_gather_rows_dev: out[dst_row[i]][k] = srcs[k][src_index[i]] ---------------------------------------------------------------------
def check_gather_rows(lib, num_srcs, words, n, rows, count, explicit=None):
    rng = np.random.Generator(np.random.PCG64(num_srcs + words + count))
    if explicit is not None:
        src_index, dst_row = (np.array(v, dtype=np.uint64) for v in explicit)
    else:
        src_index = rng.integers(0, n, size=count, dtype=np.uint64)                      # repeats allowed
        dst_row = rng.permutation(rows)[:count].astype(np.uint64)                        # a non-monotone subset of the rows
    srcs = [_u64(100 + k + count, n, words) for k in range(num_srcs)]
    g = Guarded(lib, rows * num_srcs * words * 8, count + 19)
    with _Dev(lib) as dev:
        try:
            d_srcs = [dev.put(a) for a in srcs]
            ptrs = (ctypes.c_void_p * num_srcs)(*d_srcs)
            _gather_rows(lib, ptrs, num_srcs, words * 8, src_index, dst_row, count, g.dst(0))
            frame = g.image[PAD:PAD + rows * num_srcs * words * 8].view(np.uint64).reshape(rows, num_srcs, words)      # rows not named stay as they were
            for k in range(num_srcs):
                frame[dst_row.astype(np.int64), k] = srcs[k][src_index.astype(np.int64)]
            g.check("gather_rows: %d sources of %d words, %d of %d rows" % (num_srcs, words, count, rows))
            with pytest.raises(ValueError):
                _gather_rows(lib, ptrs, num_srcs, 12, src_index, dst_row, count, g.dst(0))
            holed = (ctypes.c_void_p * num_srcs)(*(d_srcs[:-1] + [None]))
            with pytest.raises(ValueError):
                _gather_rows(lib, holed, num_srcs, words * 8, src_index, dst_row, count, g.dst(0))       # a null source
            g.check("refused gather_rows")
        finally:
            g.free()


# ---- iopx_count_mismatch_dev: *count += the number of 8-byte words at which a and b differ ------------------------------------------------
def check_count_mismatch(lib, words, flips, calls=1):
    """`flips`: word indices at which b differs from a, or "all"."""
    a = _u64(words, words)
    b = a.copy()
    if isinstance(flips, str):
        b ^= np.uint64(1) << (np.arange(words, dtype=np.uint64) % np.uint64(64))
        expect = words
    else:
        for i in flips:
            b[i] ^= np.uint64(1 << (i % 64))
        expect = len(set(flips))
    g = Guarded(lib, 8, words + 23)
    start = int(g.image[PAD:PAD + 8].view(np.uint64)[0])
    with _Dev(lib) as dev:
        try:
            d_a, d_b = dev.put(a), dev.put(b)
            for _ in range(calls):
                _count_mismatch(lib, d_a, d_b, a.nbytes, g.dst(0))
            _count_mismatch(lib, d_a, d_a, a.nbytes, g.dst(0))                      # equal buffers add nothing
            with pytest.raises(ValueError):
                _count_mismatch(lib, d_a, d_b, 12, g.dst(0))
            g.image[PAD:PAD + 8] = np.array([(start + calls * expect) % (1 << 64)], dtype=np.uint64).view(np.uint8)
            g.check("count_mismatch over %d words, %d call(s)" % (words, calls))
        finally:
            g.free()


MISMATCH_CASES = [(15000, [], 1), (15000, [0, 14999], 1), (15000, [17 * 3 + 1, 4999 * 3 + 2, 4999 * 3], 2), (1, [0], 1), (257, "all", 2)]
BIG_MISMATCH = (CAP_16384 + 5, "all", 1)
