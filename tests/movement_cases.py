"""Data-movement primitives every internal copy and fill goes through (runtime.hip): iopx_upload_small (kernel-argument path up to 3840 bytes
to 4-byte aligned destinations, pinned staging chunks above), iopx_memcpy_d2d (k_copy_d2d: 16-, 8- and 1-byte branches with byte tails, grid
capped at 8192 blocks), iopx_memset_dev (k_fill_bytes, value truncated to a byte) and the deferred read-back arena.  Shared by the
CPU-emulation and GPU suites.  The expected value is always the numpy bytes; every destination sits between guard bytes that must survive."""
import ctypes

import numpy as np

_vp, _sz = ctypes.c_void_p, ctypes.c_size_t
PAD = 64                # guard bytes on each side of a destination (the allocation itself is at least 16-byte aligned)

UPLOAD_SIZES = list(range(1, 8)) + list(range(3836, 3845)) + [4096, (1 << 20) + 5]
COPY_SIZES = [1, 15, 16, 17, 4095, 65537]
FILL_VALUES = [0x00, 0x7F, 0x80, 0xFF, 0x1AB]
BIG_COPY = (1 << 27) + 37          # above 8192 blocks x 16 KiB: the grid-stride loops take more than one trip


def upload_small(lib, d, host):
    lib._check(lib.c.iopx_upload_small(_vp(d), _vp(host.ctypes.data), _sz(host.nbytes)))


def memcpy_d2d(lib, d_dst, d_src, nbytes):
    lib._check(lib.c.iopx_memcpy_d2d(_vp(d_dst), _vp(d_src), _sz(nbytes)))


def memset_dev(lib, d, value, nbytes):
    lib._check(lib.c.iopx_memset_dev(_vp(d), ctypes.c_int(value), _sz(nbytes)))


def memcpy_d2h_deferrable(lib, host, d_src):
    lib._check(lib.c.iopx_memcpy_d2h_deferrable(_vp(host.ctypes.data), _vp(d_src), _sz(host.nbytes)))


def _bytes(seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=n, dtype=np.uint8)


class Guarded:
    """A device buffer of `span` bytes framed by `pad` (default PAD) guard bytes on each side; dst(off) is the address `off` bytes into the span."""

    def __init__(self, lib, span, seed, pad=PAD):
        self.lib, self.span, self.pad = lib, span, pad
        self.total = span + 2 * pad
        self.d = lib.malloc(self.total)
        self.image = _bytes(seed, self.total)       # what the whole allocation should hold: guard pattern, then the expected writes
        self.reset()

    def reset(self):
        self.lib.h2d(self.d, self.image)

    def dst(self, off):
        return self.d + self.pad + off

    def expect(self, off, data):
        self.image[self.pad + off:self.pad + off + len(data)] = data

    def check(self, what):
        got = np.empty(self.total, dtype=np.uint8)
        self.lib.d2h(got, self.d)
        bad = np.flatnonzero(got != self.image)
        assert bad.size == 0, "%s: %d bytes differ, the first at byte %d of the span" % (what, bad.size, bad[0] - self.pad)

    def free(self):
        self.lib.free(self.d)


def check_upload(lib, sizes=UPLOAD_SIZES):
    for size in sizes:
        g = Guarded(lib, size + 16, size)
        try:
            for off in range(16):
                host = _bytes(1000 * size + off, size)
                upload_small(lib, g.dst(off), host)
                want = host.copy()
                host[:] = 0                             # the library copied the bytes before returning
                g.expect(off, want)
                g.check("upload of %d bytes at offset %d" % (size, off))
                g.image[PAD:PAD + size + 16] = _bytes(size + off, size + 16)
                g.reset()
        finally:
            g.free()


def check_upload_back_to_back(lib, count=64):
    """64 uploads of different patterns into distinct buffers before any read-back: a staging chunk is reused only after its copy has completed."""
    sizes = [(1 << 16) + 4099 * k if k % 3 else 100 + 37 * k for k in range(count)]       # staging chunks and kernel-argument uploads, interleaved
    bufs = [Guarded(lib, s + 8, 7000 + k) for k, s in enumerate(sizes)]
    try:
        for k, (s, g) in enumerate(zip(sizes, bufs)):
            host = _bytes(9000 + k, s)
            upload_small(lib, g.dst(4 * (k % 3)), host)
            g.expect(4 * (k % 3), host.copy())
            host[:] = 0xEE
        for k, g in enumerate(bufs):
            g.check("upload %d of %d" % (k, count))
    finally:
        for g in bufs:
            g.free()


def check_copy(lib, sizes=COPY_SIZES, offsets=range(16)):
    for size in sizes:
        src = lib.malloc(size + 32)
        data = _bytes(size, size + 32)
        g = Guarded(lib, size + 16, size + 1)
        try:
            lib.h2d(src, data)
            for so in offsets:
                for do in offsets:
                    memcpy_d2d(lib, g.dst(do), src + so, size)
                    g.expect(do, data[so:so + size])
                    g.check("copy of %d bytes from offset %d to offset %d" % (size, so, do))
                    g.image[PAD:PAD + size + 16] = _bytes(100 * so + do, size + 16)
                    g.reset()
        finally:
            lib.free(src)
            g.free()


def check_big_copy(lib, size=BIG_COPY):
    """16-, 8- and 1-byte aligned copies past the 8192-block grid cap."""
    src = lib.malloc(size + 16)
    data = _bytes(77, size + 16)
    g = Guarded(lib, size + 16, 78)
    try:
        lib.h2d(src, data)
        for so, do in ((0, 0), (8, 0), (3, 5)):
            memcpy_d2d(lib, g.dst(do), src + so, size)
            g.expect(do, data[so:so + size])
            g.check("copy of %d bytes from offset %d to offset %d" % (size, so, do))
    finally:
        lib.free(src)
        g.free()


def check_fill(lib, sizes=COPY_SIZES, values=FILL_VALUES):
    for size in sizes:
        g = Guarded(lib, size + 16, size + 2)
        try:
            for off in range(16):
                for value in values:
                    memset_dev(lib, g.dst(off), value, size)
                    g.expect(off, np.full(size, value & 0xFF, dtype=np.uint8))
                    g.check("fill of %d bytes with %#x at offset %d" % (size, value, off))
                    g.image[PAD:PAD + size + 16] = _bytes(size + 16 * off + value, size + 16)
                    g.reset()
        finally:
            g.free()


# about 3 MiB in odd sizes: the first piece is above the arena's 1 MiB start (the arena grows for it), later ones overflow it and are read back at once
DEFERRED_PIECES = [(1 << 20) + (1 << 19) + 3, 100003, 77777, 250001, 4095, 333333, 65537, 1, 17, 524289, 63, 65, 191, 129
                   ] + [12345 + 1000 * k for k in range(8)]


def check_deferred_pieces(lib, pieces=DEFERRED_PIECES, windows=2):
    total = sum(pieces) + 16 * len(pieces)
    src = lib.malloc(total)
    data = _bytes(5, total)
    try:
        lib.h2d(src, data)
        for w in range(windows):                # the second window finds the arena in its grown state
            hosts, pos = [], w              # the second window's pieces start one byte further
            lib.defer_downloads_begin()
            try:
                for k, size in enumerate(pieces):
                    frame = _bytes(40 + k, size + 2 * PAD)
                    view = frame[PAD:PAD + size]
                    memcpy_d2h_deferrable(lib, view, src + pos)
                    hosts.append((frame, frame.copy(), pos, size))
                    pos += size + 16
            finally:
                lib.defer_downloads_end()
            for k, (frame, before, p, size) in enumerate(hosts):
                want = before
                want[PAD:PAD + size] = data[p:p + size]
                assert np.array_equal(frame, want), "window %d, piece %d (%d bytes)" % (w, k, size)
    finally:
        lib.free(src)
