"""Shapes that put every tile form of the comb upper butterfly pass (k_bfly_upper_comb) to work, shared by the CPU emulation's test
(tests/test_upper_tile_emu.py) and the GPU's (tests/test_gpu_upper_tile.py).

With the default geometry the last pass takes pair bits 0..5 (phase2_geom: a_low = 10 - 4), and run_phase2 cuts the pair bits [6, d) from the top
into tiles of at most five levels on 64 columns, all of them comb passes (c = 6):
    d = 11   one tile of 5 levels        (ownerships: two levels, two levels, the fifth with the fourth's bit)
    d = 12   5 + 1                       (a one-level tile: global memory to global memory, no LDS)
    d = 13, 14, 15   5 + 2, 5 + 3, 5 + 4 (a pair alone; a pair and a single level; two pairs)
    d = 17   5 + 5 + 1
References are the oracle's, byte for byte.  At d = 17 the oracle takes seconds, so the GPU test compares BLAKE2b digests of its outputs with
PINS; the CPU test computes the oracle's outputs in full, compares the emulation's bytes with them and checks that PINS are their digests."""
import functools
import hashlib

import numpy as np

import libiop_amd
import oracle
from helpers import rand_elems

W = 3
DIMS = (11, 12, 13, 14, 15, 17)
LDE_COSETS = ((0, 1), (1, 3))               # (first coset, count) out of the four of a domain of dimension d + 2

# BLAKE2b-256 of the oracle's output bytes at d = 17 (checked against the oracle by tests/test_upper_tile_emu.py::test_pins_are_the_oracles)
PINS = {
    "fft17": "29ea04b06ea92876bf9fdd817cd802e52436787a4487687e254d73df0c0f34a8",
    "lde17_1_3": "278499b53e7cf32dba19ba1ffc88d0bf42b3fc5115eaacbec9764c6ac2a13e41",
}


# the options the schedule above follows from, at their defaults (libiop_amd/csrc/fft_add.hip, tuning())
SCHEDULE_OPTIONS = {"IOPX_TILE_BITS": 11, "IOPX_P2_COLS": 6, "IOPX_P2_TOP": 4, "IOPX_COMB": 1}


def assert_comb_schedule(lib, options=None):
    """The library exposes no plan, so the tests hold the schedule by its inputs: with any of these options overridden (the environment, an
    earlier test's set_option) the dimensions above would reach other tiles or the general product, and the tests would pass without
    running k_bfly_upper_comb.  That is a failure here, not a skip.
    options: the values the case assumes where they are not the defaults (a geometry of GEOMETRIES, set in a child process's environment);
    the option table answers with the default it is asked with when nothing is set, so a value that was NOT set fails as well."""
    for name, dflt in SCHEDULE_OPTIONS.items():
        want = dflt if options is None else options[name]
        assert lib.get_option(name, dflt) == want, "%s is not %d: these shapes no longer reach the comb upper pass they are meant for" % (name, want)


# The comb upper pass at geometries the defaults never reach (the options are read once per process, so each row runs in a child process with
# them in its environment).  run_phase2 cuts the pair bits [a_low, d) from the top into tiles of at most A = TILE_BITS - P2_COLS levels, with
# a_low = min(TILE_BITS, 10) - P2_TOP (phase2_geom) and 2^c columns, c = min(TILE_BITS - levels, a_low); IOPX_P1_COLS stays at 3.
#   (TILE_BITS, P2_COLS, P2_TOP): dimensions, first dimension with two tiles        tiles (levels, c) per dimension
GEOMETRIES = {
    "six-levels": ((12, 6, 4), (12, 13, 16), 13),       # (6,6); (6,6)+(1,6); (6,6)+(4,6): three pairs, 96 KiB, 16 wave tasks on 8 waves (two per wave and pair)
    "256-columns": ((12, 8, 2), (12, 13, 15), 13),      # (4,8); +(1,8); +(3,8): column chunks (cbits = 2), a one-level tile on 256 columns
    "mixed-columns": ((11, 6, 3), (12, 13, 14, 15), 13),    # (5,6); +(1,7); +(2,7); +(3,7): two column widths in one transform
    "one-wave": ((8, 6, 2), (8, 9, 11), 9),             # (2,6); +(1,6); (2,6)+(2,6)+(1,6): one wavefront per workgroup
    "256-threads": ((10, 6, 4), (11, 13), 11),          # (4,6)+(1,6); (4,6)+(3,6): workgroups of 256 threads
}


def geometry_options(name):
    (tile, cols, top), _, _ = GEOMETRIES[name]
    return {"IOPX_TILE_BITS": tile, "IOPX_P2_COLS": cols, "IOPX_P2_TOP": top, "IOPX_COMB": 1}


def geometry_env(name):
    """what a child process needs in its environment to run the geometry `name`"""
    env = {k: str(v) for k, v in geometry_options(name).items()}
    env["IOPX_UPPER_GEOMETRY"] = name
    return env


def check_geometry(lib, on_gpu, name):
    """Per dimension the transform and its inverse on the standard basis and on a random basis with a random shift; at the first dimension with
    two tiles, cosets (1, 3) of the LDE (the first upper pass reads the shared phase-1 output) and one re-extension batch of 3 over 4 cosets:
    2^(d + 2) <= 2^15 elements per vector there, so nothing exceeds the 2^16 elements of the largest transform."""
    _, dims, two_tiles = GEOMETRIES[name]
    options = geometry_options(name)
    for d in dims:
        for kind in ("standard", "random"):
            check_fft_ifft(lib, d, kind, options=options)
    for kind in ("standard", "random"):
        check_lde(lib, on_gpu, two_tiles, kind, 1, 3, options=options)
    check_reextend(lib, on_gpu, d=two_tiles, options=options)


def digest(arr):
    return hashlib.blake2b(np.ascontiguousarray(arr).tobytes(), digest_size=32).hexdigest()


def domain(d, kind):
    """(basis of dimension d + 2, shift): the standard basis or random vectors, with a random three-word shift.  Transforms of dimension d use
    its first d vectors; the low-degree extension takes cosets of their span inside the whole domain."""
    m = d + 2
    basis = libiop_amd.standard_basis(m) if kind == "standard" else rand_elems(900 + d, m, W)
    return basis, rand_elems(700 + d, 1, W)[0]


def coeffs(d):
    return rand_elems(100 + d, 1 << d, W)


def coset_shift(basis, shift, d, c):
    s = shift.copy()
    for k in range(basis.shape[0] - d):
        if (c >> k) & 1:
            s ^= basis[d + k]
    return s


@functools.lru_cache(maxsize=None)
def ref_coset(d, kind, c):
    """The oracle's evaluations on coset c: span(basis[:d]) + shift + (the combination of basis[d:] that c's bits select)."""
    basis, shift = domain(d, kind)
    out = oracle.additive_fft(coeffs(d), basis[:d], coset_shift(basis, shift, d, c))
    out.setflags(write=False)
    return out


def ref_cosets(d, kind, cb, cc):
    return np.concatenate([ref_coset(d, kind, c) for c in range(cb, cb + cc)])


class Mem:
    """Buffers the library's *_dev entry points can take: device memory on the GPU, numpy arrays under the emulation."""

    def __init__(self, lib, on_gpu):
        self.lib, self.on_gpu, self.held = lib, on_gpu, {}

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        if self.on_gpu:
            p = self.lib.malloc(arr.nbytes)
            self.held[p] = None
            self.lib.h2d(p, arr)
            return p
        a = arr.copy()
        self.held[a.ctypes.data] = a
        return a.ctypes.data

    def new(self, count):
        return self.up(np.zeros((count, W), dtype=np.uint64))

    def down(self, p, count):
        if not self.on_gpu:
            return self.held[p][:count].copy()
        out = np.empty((count, W), dtype=np.uint64)
        self.lib.d2h(out, p)
        return out

    def close(self):
        if self.on_gpu:
            for p in self.held:
                self.lib.free(p)
        self.held = {}


def check_fft_ifft(lib, d, kind, pinned=False, options=None):
    assert_comb_schedule(lib, options)
    basis, shift = domain(d, kind)
    got = lib.additive_FFT(coeffs(d), basis[:d], shift)
    if pinned:
        assert digest(got) == PINS["fft%d" % d], ("fft", d, kind)
    else:
        assert np.array_equal(got, ref_coset(d, kind, 0)), ("fft", d, kind)
    # the inverse of a checked codeword has the coefficients themselves for its reference
    assert np.array_equal(lib.additive_IFFT(got, basis[:d], shift), coeffs(d)), ("ifft", d, kind)


def check_lde(lib, on_gpu, d, kind, cb, cc, pinned=False, options=None):
    """Cosets [cb, cb + cc) of the codeword over the whole domain: with more than one coset the first upper pass reads the shared phase-1
    output (src_shared) and writes one copy per coset."""
    assert_comb_schedule(lib, options)
    basis, shift = domain(d, kind)
    mem = Mem(lib, on_gpu)
    try:
        d_in, d_out = mem.up(coeffs(d)), mem.new(cc << d)
        lib.additive_LDE_dev(d_in, 1 << d, basis, shift, cb, cc, d_out)
        got = mem.down(d_out, cc << d)
    finally:
        mem.close()
    if pinned:
        # coset 0 alone is the transform over span(basis[:d]) + shift
        assert digest(got) == PINS["fft%d" % d if (cb, cc) == (0, 1) else "lde%d_%d_%d" % (d, cb, cc)], ("lde", d, kind, cb, cc)
    else:
        assert np.array_equal(got, ref_cosets(d, kind, cb, cc)), ("lde", d, kind, cb, cc)


@functools.lru_cache(maxsize=None)
def reextend_refs(d, batch):
    """(the batch's evaluations over span(basis[:d]) + eval_shift, the oracle's codeword of each polynomial over the whole domain), computed once
    and shared by every run of check_reextend on (d, batch)"""
    basis, shift = domain(d, "standard")
    eval_shift = rand_elems(800 + d, 1, W)[0]
    polys = [rand_elems(300 + k, 1 << d, W) for k in range(batch)]
    evals = np.concatenate([oracle.additive_fft(p, basis[:d], eval_shift) for p in polys])
    want = [oracle.additive_fft(p, basis, shift) for p in polys]
    for a in [evals] + want:
        a.setflags(write=False)
    return evals, want


def check_reextend(lib, on_gpu, d=12, batch=3, cc=4, options=None):
    """`batch` vectors of evaluations over span(basis[:d]) + eval_shift, re-extended onto the four cosets of the whole domain: the batched
    inverse upper passes (the vectors of a batch in the place of cosets), then the forward ones per polynomial."""
    assert_comb_schedule(lib, options)
    basis, shift = domain(d, "standard")
    eval_shift = rand_elems(800 + d, 1, W)[0]
    evals, want = reextend_refs(d, batch)
    mem = Mem(lib, on_gpu)
    try:
        d_in = mem.up(evals)
        outs = [mem.new(cc << d) for _ in range(batch)]
        lib.additive_reextend_batch_dev(d_in, batch, basis, d, eval_shift, shift, 0, cc, outs)
        got = [mem.down(o, cc << d) for o in outs]
    finally:
        mem.close()
    for k in range(batch):
        assert np.array_equal(got[k], want[k]), ("reextend", k)
