"""Cases for the batched transforms and the fused re-extension over GF(2^64), GF(2^128) and GF(2^256) (include/libiop_amd_batch.h; the kernels
and entry bodies of libiop_amd/csrc/gfx_additive.h), parametrised by the words per element W in {1, 2, 4}.  Shared by tests/test_gfx_batch_emu.py
(CPU emulation) and tests/test_gpu_gfx_batch.py (MI355X): every function takes the Library under test.

Every comparison is byte equality of whole vectors.  The expected values are what the single-vector entries of the same build give (they are held
to the oracle by tests/gf64_cases.py, gf128_cases.py and gf256_cases.py) and, for one case per field and entry, the oracle's own additive FFT / IFFT.
Elements are (n, W) uint64 arrays; a re-extension of `batch` vectors over H = span(basis[:d]) + eval_shift onto cosets [begin, begin + count) of
L = span(basis[:m]) + shift is expected to be, per vector, LDE(IFFT(v, H), 2^d coefficients, L)[begin * 2^d : (begin + count) * 2^d]."""
import contextlib

import numpy as np
import pytest

import gfx_aurora_cases as C
import oracle

WORDS = (1, 2, 4)
NAME = {1: "gf64", 2: "gf128", 4: "gf256"}
STEM = {1: "k64_", 2: "k128_", 4: "k256_"}
TILE_OPTIONS = ("TILE_BITS", "P1_COLS", "P2_COLS", "P2_TOP")
STAGE_OPTION = "IOPX_GFX_BATCH_STAGE_BITS"
SMALLEST_TILES = (3, 1, 1, 1)           # 2^3-element tiles: at d = 9 four upper passes and the last one, six phase-1 chunks per early level
OFFSETS = (0, 8)
DIMS, EXTRA, BATCHES = (0, 1, 2, 5, 9), (0, 1, 4), (1, 2, 3, 5)


def seeded(tag, n, W):
    return C.seeded("batch " + tag, n, W)


def domain(m, W):
    return oracle.standard_basis(m, W), C.elem(W, C.top(W) | 0x7654321 | (1 << m))


@contextlib.contextmanager
def options(lib, W, tiles=None, stage_bits=None):
    """the field's four tile options and the staging bound of the batched forward passes, for the calls inside; plans are per geometry"""
    names = {}
    if tiles is not None:
        names.update({"IOPX_%s_%s" % (NAME[W].upper(), k): v for k, v in zip(TILE_OPTIONS, tiles)})
    if stage_bits is not None:
        names[STAGE_OPTION] = stage_bits
    try:
        for k, v in names.items():
            lib.set_option(k, v)
        lib.clear_plans()
        yield
    finally:
        for k in names:
            lib.clear_option(k)
        lib.clear_plans()


# ---- the single-vector entries: what the batched ones must reproduce ----
def ifft_one(lib, W, d_evals, basis, shift, d_out):
    if W == 1:
        lib.additive_IFFT_gf64_dev(d_evals, basis, shift, d_out)
    else:
        lib.additive_IFFT_dev(d_evals, basis, shift, d_out, words=W)


def lde_one(lib, W, d_coeffs, n_coeffs, basis, shift, begin, count, d_out):
    if W == 1:
        lib.additive_LDE_gf64_dev(d_coeffs, n_coeffs, basis, shift, begin, count, d_out)
    else:
        lib.additive_LDE_dev(d_coeffs, n_coeffs, basis, shift, begin, count, d_out, words=W)


def expected_ifft(lib, W, vectors, basis, shift):
    outs = []
    with C.Device(lib, W) as dev:
        for v in vectors:
            p, o = dev.put(v), dev.empty(8 * W * v.shape[0])
            ifft_one(lib, W, p, basis, shift, o)
            outs.append(dev.get(o, v.shape[0]))
    return outs


def expected_lde(lib, W, polys, basis, shift, begin, count):
    n_coeffs = polys[0].shape[0]
    d = max(n_coeffs - 1, 0).bit_length()
    outs = []
    with C.Device(lib, W) as dev:
        for c in polys:
            p, o = dev.put(c), dev.empty(8 * W * (count << d))
            lde_one(lib, W, p, n_coeffs, basis, shift, begin, count, o)
            outs.append(dev.get(o, count << d))
    return outs


def expected_reextend(lib, W, vectors, basis, d, eval_shift, shift, begin, count):
    return expected_lde(lib, W, expected_ifft(lib, W, vectors, basis[:d], eval_shift), basis, shift, begin, count)


# ---- the batched entries, every buffer `off` bytes past a 16-byte boundary (out_offs: per output) ----
def run_reextend(lib, W, vectors, basis, d, eval_shift, shift, begin, count, polys=(), off=0, out_offs=None, profile=False):
    """iopx_add_reextend_FIELD_batch_dev (no polynomials) or iopx_add_reextend_lde_FIELD_batch_dev; (outputs, profile)"""
    n_out = count << d
    total = len(vectors) + len(polys)
    with C.Device(lib, W, off) as dev:
        d_in = dev.put(np.concatenate(vectors))
        d_polys = [dev.put(c) for c in polys]
        outs = []
        for k in range(total):
            dev.off = off if out_offs is None else out_offs[k]
            outs.append(dev.empty(8 * W * n_out))
        if profile:
            lib.profile_begin()
        if polys:
            lib.additive_reextend_lde_batch_dev(d_in, len(vectors), d_polys, polys[0].shape[0], basis, d, eval_shift, shift, begin, count, outs, words=W)
        else:
            lib.additive_reextend_batch_dev(d_in, len(vectors), basis, d, eval_shift, shift, begin, count, outs, words=W)
        prof = lib.profile_report() if profile else None
        return [dev.get(o, n_out) for o in outs], prof


def run_lde_batch(lib, W, polys, basis, shift, begin, count, off=0):
    n_coeffs = polys[0].shape[0]
    n_out = count << max(n_coeffs - 1, 0).bit_length()
    with C.Device(lib, W, off) as dev:
        ins = [dev.put(c) for c in polys]
        outs = [dev.empty(8 * W * n_out) for _ in polys]
        lib.additive_LDE_batch_dev(ins, n_coeffs, basis, shift, begin, count, outs, words=W)
        return [dev.get(o, n_out) for o in outs]


def run_ifft_batch(lib, W, vectors, basis, shift, off=0, in_place=False):
    n = vectors[0].shape[0]
    with C.Device(lib, W, off) as dev:
        d_in = dev.put(np.concatenate(vectors))
        d_out = d_in if in_place else dev.empty(8 * W * n * len(vectors))
        lib.additive_IFFT_batch_dev(d_in, len(vectors), basis, shift, d_out, words=W)
        got = dev.get(d_out, n * len(vectors))
        return [got[k * n:(k + 1) * n] for k in range(len(vectors))]


def same(got, want, why):
    assert len(got) == len(want), why
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (why, "vector %d" % k)


# ---- 1. the grid of dimensions: d_dim x (m - d_dim) x batch, both placements ----
def check_reextend_grid(lib, W, tiles=None):
    """every d_dim in DIMS with every m - d_dim in EXTRA and every batch in BATCHES, all cosets, at both placements; tiles=SMALLEST_TILES takes d_dim = 9
    through four upper passes and the last one in each direction"""
    with options(lib, W, tiles=tiles):
        for d in DIMS:
            for extra in EXTRA:
                m = d + extra
                basis, shift = domain(m, W)
                es = C.elem(W, 0x55 << 3)
                vectors = [seeded("grid %d %d %d" % (d, extra, k), 1 << d, W) for k in range(max(BATCHES))]
                want = expected_reextend(lib, W, vectors, basis, d, es, shift, 0, 1 << extra)
                for batch in BATCHES:
                    for off in OFFSETS:
                        got, _ = run_reextend(lib, W, vectors[:batch], basis, d, es, shift, 0, 1 << extra, off=off)
                        same(got, want[:batch], (NAME[W], d, extra, batch, off))


def check_lde_grid(lib, W, tiles=None):
    """n_coeffs in {1, 2^d - 3, 2^d} for d in {2, 5, 9} (2^2 - 3 = 1: the constant), m - d in EXTRA, every batch, both placements; for m - d = 4 also
    one coset in the middle, the last one and an odd range"""
    with options(lib, W, tiles=tiles):
        for d in (2, 5, 9):
            for n_coeffs in sorted({1, (1 << d) - 3, 1 << d}):
                dd = max(n_coeffs - 1, 0).bit_length()
                for extra in EXTRA:
                    m = d + extra
                    basis, shift = domain(m, W)
                    cosets = 1 << (m - dd)
                    polys = [seeded("lde %d %d %d %d" % (d, n_coeffs, extra, k), n_coeffs, W) for k in range(max(BATCHES))]
                    windows = [(0, cosets)] + ([(cosets // 2 - 1, 1), (cosets - 1, 1), (3, 5)] if extra == 4 else [])
                    for begin, count in windows:
                        want = expected_lde(lib, W, polys, basis, shift, begin, count)
                        for batch in BATCHES if (begin, count) == (0, cosets) else (3,):
                            for off in OFFSETS:
                                same(run_lde_batch(lib, W, polys[:batch], basis, shift, begin, count, off=off), want[:batch], (NAME[W], d, n_coeffs, extra, begin, count, batch, off))


def check_ifft_grid(lib, W, tiles=None):
    """m in DIMS, every batch, both placements, out of place and with d_out == d_evals"""
    with options(lib, W, tiles=tiles):
        for m in DIMS:
            basis, shift = domain(m, W)
            vectors = [seeded("ifft %d %d" % (m, k), 1 << m, W) for k in range(max(BATCHES))]
            want = expected_ifft(lib, W, vectors, basis, shift)
            for batch in BATCHES:
                for off in OFFSETS:
                    for in_place in (False, True):
                        same(run_ifft_batch(lib, W, vectors[:batch], basis, shift, off=off, in_place=in_place), want[:batch], (NAME[W], m, batch, off, in_place))


def check_reextend_lde_grid(lib, W, tiles=None):
    """n_polys in {1, 2} with n_coeffs in {1, 2^d - 3, 2^d} beside batches of 1 and 3, d_dim in {2, 5, 9}; a batch of none is refused as gf192 refuses it"""
    with options(lib, W, tiles=tiles):
        for d in (2, 5, 9):
            for extra in (0, 1, 4):
                m = d + extra
                basis, shift = domain(m, W)
                es = C.elem(W, C.top(W) >> 2)
                vectors = [seeded("relde v %d %d %d" % (d, extra, k), 1 << d, W) for k in range(3)]
                want_v = expected_reextend(lib, W, vectors, basis, d, es, shift, 0, 1 << extra)
                for n_coeffs in sorted({1, (1 << d) - 3, 1 << d}):
                    polys = [seeded("relde p %d %d %d" % (d, n_coeffs, k), n_coeffs, W) for k in range(2)]
                    padded = [np.concatenate([c, np.zeros(((1 << d) - n_coeffs, W), dtype=np.uint64)]) for c in polys]      # 2^d coefficients: the cosets of span(basis[:d])
                    want_p = expected_lde(lib, W, padded, basis, shift, 0, 1 << extra)
                    for batch, n_polys in ((1, 1), (3, 1), (1, 2), (3, 2)):
                        for off in OFFSETS:
                            got, _ = run_reextend(lib, W, vectors[:batch], basis, d, es, shift, 0, 1 << extra, polys=polys[:n_polys], off=off)
                            same(got, want_v[:batch] + want_p[:n_polys], (NAME[W], d, extra, n_coeffs, batch, n_polys, off))
    basis, shift = domain(3, W)
    with C.Device(lib, W) as dev:
        p = dev.put(seeded("relde none", 8, W))
        with pytest.raises(ValueError, match=r"batch size 0 \+ 1 outside 1\.\.65535"):
            lib.additive_reextend_lde_batch_dev(p, 0, [p], 8, basis, 3, shift, shift, 0, 1, [p], words=W)


# ---- 2. coset windows and the staging bound ----
def check_coset_windows(lib, W):
    """d_dim = 5 under the smallest tiles (two upper passes, so the forward passes stage), 16 cosets: all of them, one in the middle, the last one and
    [3, 8).  With the staging at 2^8 elements (8 cosets of single vectors) a batch of 3 takes groups of 2 cosets — [3, 8) ends in a group of one — and
    a batch of 5 with the staging at 2^7 (4 slots) goes in two rounds of vectors, 4 and 1, one coset at a time."""
    d, m = 5, 9
    basis, shift = domain(m, W)
    es = C.elem(W, 0x123 << 7)
    vectors = [seeded("window %d" % k, 1 << d, W) for k in range(5)]
    windows = ((0, 16), (7, 1), (15, 1), (3, 5))
    with options(lib, W, tiles=SMALLEST_TILES):
        want = {w: expected_reextend(lib, W, vectors, basis, d, es, shift, *w) for w in windows}
    for stage_bits, batch in ((None, 3), (8, 3), (7, 5), (0, 2)):
        with options(lib, W, tiles=SMALLEST_TILES, stage_bits=stage_bits):
            for w in windows:
                for off in OFFSETS:
                    got, _ = run_reextend(lib, W, vectors[:batch], basis, d, es, shift, *w, off=off)
                    same(got, want[w][:batch], (NAME[W], stage_bits, batch, w, off))


def check_default_tiles(lib, W):
    """d_dim = 13, m = 16 at the default tiles (past one tile of 2^11): a batch of 2 onto all 8 cosets, once with the default staging and once with it
    at 2^15 elements — 4 slots, so the coset range is taken in four groups of two"""
    d, m = 13, 16
    basis, shift = domain(m, W)
    es = C.elem(W, 1 << 14)
    vectors = [seeded("default %d" % k, 1 << d, W) for k in range(2)]
    want = expected_reextend(lib, W, vectors, basis, d, es, shift, 0, 8)
    got, prof = run_reextend(lib, W, vectors, basis, d, es, shift, 0, 8, profile=True)
    same(got, want, (NAME[W], "default staging"))
    assert prof[STEM[W] + "bfly_edge_batch"][0] == 1 and prof[STEM[W] + "bfly_upper_batch"][0] >= 1, prof
    with options(lib, W, stage_bits=15):
        got, prof = run_reextend(lib, W, vectors, basis, d, es, shift, 0, 8, profile=True)
    same(got, want, (NAME[W], "staging of 2^15"))
    assert prof[STEM[W] + "bfly_edge_batch"][0] == 4, prof


# ---- 3. shifts ----
def check_shifts(lib, W):
    """eval_shift zero, equal to the codeword domain's shift, in L outside H, and outside L (d_dim = 5, m = 7, three vectors, cosets [1, 4))"""
    d, m = 5, 7
    basis, shift = domain(m, W)
    shift_int = sum(int(w) << (64 * i) for i, w in enumerate(shift))
    vectors = [seeded("shift %d" % k, 1 << d, W) for k in range(3)]
    for tag, es in (("zero", C.elem(W, 0)), ("the codeword domain's", shift), ("in L outside H", C.elem(W, shift_int ^ (1 << 6))), ("outside L", C.elem(W, 1 << 20))):
        want = expected_reextend(lib, W, vectors, basis, d, es, shift, 1, 3)
        for off in OFFSETS:
            got, _ = run_reextend(lib, W, vectors, basis, d, es, shift, 1, 3, off=off)
            same(got, want, (NAME[W], tag, off))


# ---- 4. alignment: which instantiation runs ----
def check_alignment(lib, W):
    """every buffer aligned: no "_w64" row; every buffer at 8 mod 16: the launches that touch a caller's buffer (the first inverse pass, the last forward
    pass) run the 64-bit instantiations; one output of three at 8 mod 16: the launch that sees the array of outputs takes the 64-bit form, the first
    inverse pass does not, same bytes.  A one-word element has one access path."""
    d, m = 5, 7
    basis, shift = domain(m, W)
    es = C.elem(W, 0x77)
    vectors = [seeded("align %d" % k, 1 << d, W) for k in range(3)]
    with options(lib, W, tiles=SMALLEST_TILES):
        want = expected_reextend(lib, W, vectors, basis, d, es, shift, 0, 4)
        for tag, off, out_offs in (("aligned", 0, None), ("all at 8", 8, None), ("one output at 8", 0, [0, 8, 0])):
            got, prof = run_reextend(lib, W, vectors, basis, d, es, shift, 0, 4, off=off, out_offs=out_offs, profile=True)
            same(got, want, (NAME[W], tag))
            rows = {k: v[0] for k, v in prof.items() if k.startswith(STEM[W]) and "bfly" in k}
            w64 = sorted(k for k in rows if k.endswith("_w64"))
            if W == 1 or tag == "aligned":
                assert not w64, (tag, rows)
            elif tag == "all at 8":             # the upper passes run between the library's own (aligned) temporaries
                assert sorted(k for k in rows if "edge" in k) == [STEM[W] + "bfly_edge_batch_w64", STEM[W] + "bfly_edge_inv_batch_w64"], (tag, rows)
            else:
                assert STEM[W] + "bfly_edge_batch_w64" in rows and STEM[W] + "bfly_edge_batch" not in rows and STEM[W] + "bfly_edge_inv_batch" in rows, (tag, rows)


# ---- 5. aliasing ----
def check_aliased_output(lib, W):
    """one vector re-extended onto the single coset of L = H's span, its output over its input: the inverse passes write a work buffer, so the result is
    the separate call's (gf192 behaves the same way)"""
    d = 5
    basis, shift = domain(d, W)
    es = C.elem(W, 0x31)
    v = seeded("alias", 1 << d, W)
    want = expected_reextend(lib, W, [v], basis, d, es, shift, 0, 1)
    for off in OFFSETS:
        with C.Device(lib, W, off) as dev:
            p = dev.put(v)
            lib.additive_reextend_batch_dev(p, 1, basis, d, es, shift, 0, 1, [p], words=W)
            assert np.array_equal(dev.get(p, 1 << d), want[0]), (NAME[W], off)


# ---- 6. refusals: gf192's messages ----
def check_refusals(lib, W):
    d, m = 3, 5
    basis, shift = domain(m, W)
    with C.Device(lib, W) as dev:
        p = dev.put(seeded("refused", 4 << m, W))
        q = p + 8 * W * (1 << m)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_reextend_batch_dev(0, 1, basis, d, shift, shift, 0, 1, [q], words=W)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_reextend_batch_dev(p, 2, basis, d, shift, shift, 0, 1, [q, 0], words=W)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_reextend_lde_batch_dev(p, 1, [0], 4, basis, d, shift, shift, 0, 1, [q, q], words=W)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_IFFT_batch_dev(p, 1, basis, shift, 0, words=W)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_LDE_batch_dev([p, 0], 8, basis, shift, 0, 1, [q, q], words=W)
        with pytest.raises(ValueError, match="the evaluation domain must be spanned by the first basis vectors of the codeword domain"):
            lib.additive_reextend_batch_dev(p, 1, basis, m + 1, shift, shift, 0, 1, [q], words=W)
        for begin, count in ((0, 0), (4, 1), (3, 2), (0, 5)):
            with pytest.raises(ValueError, match="outside the 4 cosets of the transform"):
                lib.additive_reextend_batch_dev(p, 1, basis, d, shift, shift, begin, count, [q], words=W)
            with pytest.raises(ValueError, match="outside the 4 cosets of the transform"):
                lib.additive_LDE_batch_dev([p, p], 8, basis, shift, begin, count, [q, q], words=W)
        with pytest.raises(ValueError, match="9 coefficients exceed the 2\\^3 of the evaluation domain"):
            lib.additive_reextend_lde_batch_dev(p, 1, [p], 9, basis, d, shift, shift, 0, 1, [q, q], words=W)
        for batch in (0, 65536):
            with pytest.raises(ValueError, match="batch size %d outside 1..65535" % batch):
                lib.additive_IFFT_batch_dev(p, batch, basis[:1], shift, q, words=W)
        big = oracle.standard_basis(41, W) if W > 1 else np.arange(1, 42, dtype=np.uint64).reshape(41, 1)
        for call in (lambda: lib.additive_reextend_batch_dev(p, 1, big, d, shift, shift, 0, 1, [q], words=W),
                     lambda: lib.additive_IFFT_batch_dev(p, 1, big, shift, q, words=W),
                     lambda: lib.additive_LDE_batch_dev([p], 8, big, shift, 0, 1, [q], words=W)):
            with pytest.raises(ValueError, match="domain dimension 41 too large"):
                call()


# ---- 7. the launches of a fused re-extension ----
def field_rows(prof, W):
    return {k: v[0] for k, v in prof.items() if k.startswith(STEM[W])}


def check_structure(lib, W):
    """A fused re-extension launches no phase-1 kernel in either direction, and a batch of four takes exactly the launches of a batch of one: under the
    smallest tiles at d_dim = 9 onto two cosets that is the first inverse pass, four inverse upper passes, four forward ones and the last pass."""
    d, m = 9, 10
    basis, shift = domain(m, W)
    es = C.elem(W, 0x99)
    vectors = [seeded("structure %d" % k, 1 << d, W) for k in range(4)]
    rows = {}
    with options(lib, W, tiles=SMALLEST_TILES):
        run_reextend(lib, W, vectors, basis, d, es, shift, 0, 2)         # the plan's tables are built outside the profiles
        for batch in (1, 4):
            _, prof = run_reextend(lib, W, vectors[:batch], basis, d, es, shift, 0, 2, profile=True)
            rows[batch] = field_rows(prof, W)
    s = STEM[W]
    assert rows[1] == {s + "bfly_edge_inv_batch": 1, s + "bfly_upper_inv_batch": 4, s + "bfly_upper_batch": 4, s + "bfly_edge_batch": 1}, rows[1]
    assert rows[4] == rows[1], rows
    assert not [k for k in rows[4] if "phase1" in k]


# ---- 8. the oracle's own transforms, one case per field and entry ----
def check_against_the_oracle(lib, W):
    d, m = 5, 7
    basis, shift = domain(m, W)
    es = C.elem(W, 0xABC)
    vectors = [seeded("oracle v %d" % k, 1 << d, W) for k in range(3)]
    polys = [seeded("oracle p %d" % k, (1 << d) - 3, W) for k in range(2)]
    coeffs = [oracle.additive_ifft(v, basis[:d], es) for v in vectors]
    want_v = [oracle.additive_fft(c, basis, shift) for c in coeffs]
    want_p = [oracle.additive_fft(c, basis, shift) for c in polys]
    for tiles in (None, SMALLEST_TILES):
        with options(lib, W, tiles=tiles):
            same(run_ifft_batch(lib, W, vectors, basis[:d], es), coeffs, (NAME[W], "ifft_batch", tiles))
            same(run_lde_batch(lib, W, polys, basis, shift, 0, 4), want_p, (NAME[W], "lde_batch", tiles))
            same(run_reextend(lib, W, vectors, basis, d, es, shift, 0, 4)[0], want_v, (NAME[W], "reextend_batch", tiles))
            got, _ = run_reextend(lib, W, vectors, basis, d, es, shift, 1, 2, polys=polys)
            same(got, [w[1 << d:3 << d] for w in want_v + want_p], (NAME[W], "reextend_lde_batch", tiles))


# ---- 9. the provers ----
def native_instance(lib, W, log_n, k):
    """(instance handle, the expected transcript): the oracle's over gf64, the model's (tests/gfx_aurora_model.py) over gf128 and gf256"""
    import libiop_amd as la
    if W == 1:
        import gf64_aurora_cases as G
        n = 1 << log_n
        return lib.aurora_example_instance(la.FIELD_GF64, n, k, n - 1, G.SEED), oracle.aurora_prove(oracle.FIELD_GF64, log_n, k, G.SEED)
    want, _, inst = C.model(W, log_n, k)
    return lib.aurora_instance(C.field_code(W), inst["matrices"], inst["num_variables"], k, inst["z"]), want


def check_native_proof_profile(lib, W):
    """One native Aurora proof (2^7 constraints, 15 inputs): the expected bytes, through the batched kernels.  Every transform of this size is one
    phase-1 pass and one butterfly pass, so each plain inverse transform — a genuine coefficient form — is one bfly_edge_inv and one phase1_inv
    launch; the re-extensions bring bfly_edge_inv_batch launches and no phase-1 launch with them: the counts of phase1_inv and bfly_edge_inv agree
    and no batched phase-1 row exists in the inverse direction."""
    h, want = native_instance(lib, W, 7, 15)
    try:
        assert lib.aurora_prove(h) == want                 # plans and tables
        lib.profile_begin()
        mine = lib.aurora_prove(h)
        rows = field_rows(lib.profile_report(), W)
    finally:
        lib.aurora_instance_free(h)
    assert mine == want
    s = STEM[W]
    fused = sum(rows.get(s + "bfly_edge_inv_batch" + t, 0) for t in ("", "_w64"))
    assert fused >= 2 and sum(rows.get(s + "bfly_edge_batch" + t, 0) for t in ("", "_w64")) == fused, rows
    assert not [k for k in rows if "phase1_inv_batch" in k], rows
    assert sum(rows.get(s + "phase1_inv" + t, 0) for t in ("", "_w64")) == sum(rows.get(s + "bfly_edge_inv" + t, 0) for t in ("", "_w64")), rows
    return rows


def check_python_proof_profile(lib, torch, device, W):
    """The Python prover's transcript at (6, 3) with the field's AuroraOps, and in its profile the fused re-extension's rows"""
    if W == 1:
        import gf64_aurora_cases as G
        case = G.PYTHON_TUPLES[0]
        lib.profile_begin()
        G.check_python_prover(lib, torch, device, case)
    else:
        case = C.PYTHON_TUPLES[W][0]
        lib.profile_begin()
        C.check_python_prover(lib, torch, device, W, case)
    rows = field_rows(lib.profile_report(), W)
    assert sum(rows.get(STEM[W] + "bfly_edge_inv_batch" + t, 0) for t in ("", "_w64")) >= 2, rows
