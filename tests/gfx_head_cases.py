"""Cases for head evaluation over GF(2^64), GF(2^128) and GF(2^256) (include/libiop_amd_head.h): the pointwise division by Z_S, the host's Z_S(x),
the two-group fused re-extension, and the native Aurora prover under IOPX_GFX_HEAD_EVAL=1, parametrised by the words per element W in {1, 2, 4}.
Shared by tests/test_gfx_head_emu.py (CPU emulation) and tests/test_gpu_gfx_head.py (MI355X): every function takes the Library under test.

Every comparison is byte equality.  Expected values of the division need no division: Z_S(x_j) is the plain product of (x_j + s) over the
2^sub_dim elements s of S (oracle.gf_mul; the x_j are the subset sums in the reference's order), and the output must satisfy out * Z = in — Z != 0
makes the quotient unique.  At three words the same construction reproduces iopx_div_by_vanishing_gf192_dev and iopx_gf192_vanishing_host."""
import hashlib

import numpy as np
import pytest

import gfx_aurora_cases as C
import gfx_aurora_model as M
import gfx_batch_cases as B
import oracle

WORDS = B.WORDS
NAME = B.NAME
STEM = B.STEM
OPTION = "IOPX_GFX_HEAD_EVAL"
DIV_SHAPES = ((0, 0), (1, 0), (1, 1), (5, 0), (5, 4), (5, 5), (9, 4), (11, 4))
REEXTEND_SHAPES = ((3, 1), (5, 5), (9, 5), (9, 9), (13, 9))
REEXTEND_BATCHES = ((3, 1), (1, 1), (2, 3))


def seeded(tag, n, W):
    return C.seeded("head " + tag, n, W)


def one(W):
    return M.elem(W, 1)


def product(elems, W):
    """the product of the rows of an (n, W) array"""
    acc = one(W).reshape(1, W)
    for e in elems:
        acc = oracle.gf_mul(acc, e.reshape(1, W))
    return acc[0]


def vanishing_over(xs, S):
    """Z_S(x) = prod_{s in S} (x + s) for every row x of xs"""
    acc = np.ascontiguousarray(np.broadcast_to(one(xs.shape[1]), xs.shape))
    for s in S:
        acc = oracle.gf_mul(acc, xs ^ s)
    return acc


def div_domains(m, sub_dim, W, kind):
    """(basis, shift, sub_shift): the standard basis with shift 1 << m and S unshifted, or a seeded basis with seeded shifts"""
    if kind == "standard":
        return oracle.standard_basis(m, W), M.elem(W, 1 << m), M.elem(W, 0)
    tag = "div %d %d" % (m, sub_dim)
    return seeded(tag + " basis", m, W), seeded(tag + " shift", 1, W)[0], seeded(tag + " sub", 1, W)[0]


def div_call(lib, W):
    return lambda p_in, basis, shift, sub_dim, sub_shift, p_out: lib.div_by_vanishing(p_in, basis, shift, sub_dim, sub_shift, p_out, words=W)


def label(W, w64):
    return STEM[W] + "div_by_vanishing" + ("_w64" if w64 else "")


def run_div(lib, W, v, basis, shift, sub_dim, sub_shift, in_off=0, out_off=0, in_place=False, call=None):
    """(the output, the profile's rows of the field's division kernel)"""
    call = call or div_call(lib, W)
    n = v.shape[0]
    with C.Device(lib, W, in_off) as dev:
        p_in = dev.put(v)
        dev.off = out_off
        p_out = p_in if in_place else dev.empty(8 * W * n)
        lib.profile_begin()
        call(p_in, basis, shift, sub_dim, sub_shift, p_out)
        prof = lib.profile_report()
        return dev.get(p_out, n), {k: val for k, val in prof.items() if "div_by_vanishing" in k}


def check_div_by_vanishing(lib, W, m, sub_dim, call=None, stem=None):
    """both kinds of domain, every placement of the two vectors and in place: out * Z_S = in, the "_w64" label exactly when a pointer is off the
    16-byte boundary, 2 n E declared bytes"""
    n = 1 << m
    for kind in ("standard", "seeded"):
        basis, shift, sub_shift = div_domains(m, sub_dim, W, kind)
        xs = oracle.all_subset_sums(basis, shift)
        Z = vanishing_over(xs, oracle.all_subset_sums(basis[:sub_dim], sub_shift))
        assert Z.any(axis=1).all(), "the domain meets S"
        v = seeded("div in %d %d %s" % (m, sub_dim, kind), n, W)
        for in_off, out_off, in_place in ((0, 0, False), (8, 8, False), (0, 8, False), (8, 0, False), (0, 0, True), (8, 8, True)):
            got, rows = run_div(lib, W, v, basis, shift, sub_dim, sub_shift, in_off, out_off, in_place, call)
            assert np.array_equal(oracle.gf_mul(got, Z), v), (NAME.get(W, W), m, sub_dim, kind, in_off, out_off, in_place)
            if stem is None:
                w64 = bool(in_off or (out_off and not in_place))
                assert list(rows) == [label(W, w64)], (rows, in_off, out_off, in_place)
                assert rows[label(W, w64)][0] == 1 and rows[label(W, w64)][2] == 2 * n * 8 * W, rows


def check_div_trust(lib):
    """the trust condition: at three words the construction above accepts iopx_div_by_vanishing_gf192_dev"""
    for m, sub_dim in ((5, 4), (9, 4), (5, 0)):
        check_div_by_vanishing(lib, 3, m, sub_dim, call=div_call(lib, 3), stem="k_")


def check_div_grid_cap(lib, W):
    """the grid cap (IOPX_GFX_OPS_MAX_BLOCKS) at 2 blocks and 2^11 points: four trips of the one-element loop (two of gf64's pair loop), same outputs"""
    m, sub_dim = 11, 4
    basis, shift, sub_shift = div_domains(m, sub_dim, W, "seeded")
    v = seeded("div cap", 1 << m, W)
    Z = vanishing_over(oracle.all_subset_sums(basis, shift), oracle.all_subset_sums(basis[:sub_dim], sub_shift))
    with C.options(lib, IOPX_GFX_OPS_MAX_BLOCKS=2):
        for off in (0, 8):
            got, rows = run_div(lib, W, v, basis, shift, sub_dim, sub_shift, off, off)
            assert np.array_equal(oracle.gf_mul(got, Z), v), (NAME[W], off)
            assert list(rows) == [label(W, bool(off))], rows


def check_div_refusals(lib, W):
    m, sub_dim = 5, 2
    basis = oracle.standard_basis(m, W)
    zero, shift = M.elem(W, 0), M.elem(W, 1 << m)
    with C.Device(lib, W) as dev:
        p = dev.put(seeded("div refused", 1 << m, W))
        with pytest.raises(ValueError, match="the domain intersects the vanishing set"):
            lib.div_by_vanishing(p, basis, zero, sub_dim, zero, p, words=W)
        with pytest.raises(ValueError, match="the vanishing set must be spanned by a prefix of the domain's basis"):
            lib.div_by_vanishing(p, basis, shift, m + 1, zero, p, words=W)
        big = oracle.standard_basis(41, W) if W > 1 else np.arange(1, 42, dtype=np.uint64).reshape(41, 1)
        with pytest.raises(ValueError, match="the vanishing set must be spanned by a prefix of the domain's basis"):
            lib.div_by_vanishing(p, big, shift, 2, zero, p, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.div_by_vanishing(0, basis, shift, sub_dim, zero, p, words=W)
        with pytest.raises(ValueError, match="null argument"):
            lib.div_by_vanishing(p, basis, shift, sub_dim, zero, 0, words=W)
        fn = getattr(lib.c, "iopx_div_by_vanishing_%s_dev" % NAME[W])
        b, s = np.ascontiguousarray(basis), np.ascontiguousarray(shift)
        for args in ((C.VP(p), None, m, s.ctypes.data_as(C.U64P), sub_dim, s.ctypes.data_as(C.U64P), C.VP(p)),
                     (C.VP(p), b.ctypes.data_as(C.U64P), m, None, sub_dim, s.ctypes.data_as(C.U64P), C.VP(p)),
                     (C.VP(p), b.ctypes.data_as(C.U64P), m, s.ctypes.data_as(C.U64P), sub_dim, None, C.VP(p))):
            with pytest.raises(ValueError, match="null argument"):
                lib._check(fn(*args))
        # the rowcheck keeps its own wording for its own refusal
        with pytest.raises(ValueError, match="the codeword domain intersects the constraint domain"):
            lib.rowcheck_dev(p, p, p, basis, zero, sub_dim, zero, p, words=W)


# ---- Z_S(x) on the host ----
def check_vanishing_host(lib, W):
    """dim in {0, 1, 4, 6}: x inside S, outside S and 0; the value is the product over S of (x + s), the linear coefficient the product of the non-zero
    elements of span(basis) (1 at dim 0); either output may be NULL.  W = 3 runs the gf192 entry through the same construction."""
    zero = M.elem(W, 0)
    for dim in (0, 1, 4, 6):
        basis, shift = seeded("host basis %d" % dim, dim, W), seeded("host shift %d" % dim, 1, W)[0]
        S = oracle.all_subset_sums(basis, shift)
        span = oracle.all_subset_sums(basis, zero)
        lin_want = product(span[1:], W)
        if dim == 0:
            assert np.array_equal(lin_want, one(W))
        for tag, x in (("inside", S[len(S) // 2]), ("outside", seeded("host x %d" % dim, 1, W)[0]), ("zero", zero)):
            want = vanishing_over(x.reshape(1, W), S)[0]
            assert want.any() == (tag != "inside")
            value, lin = lib.vanishing_host(basis, shift, x, words=W)
            assert np.array_equal(value, want) and np.array_equal(lin, lin_want), (W, dim, tag)
            only_value, none = lib.vanishing_host(basis, shift, x, words=W, want_linear_coefficient=False)
            assert none is None and np.array_equal(only_value, want)
            none, only_lin = lib.vanishing_host(basis, shift, x, words=W, want_value=False)
            assert none is None and np.array_equal(only_lin, lin_want)
            if W == 3:
                v3, l3 = lib.gf192_vanishing_host(basis, shift, x)
                assert np.array_equal(v3, want) and np.array_equal(l3, lin_want)
    if W != 3:
        fn = getattr(lib.c, "iopx_%s_vanishing_host" % NAME[W])
        s = np.ascontiguousarray(zero)
        out = np.zeros(W, dtype=np.uint64)
        for args in ((None, 2, s.ctypes.data_as(C.U64P), s.ctypes.data_as(C.U64P)), (s.ctypes.data_as(C.U64P), 0, None, s.ctypes.data_as(C.U64P)),
                     (s.ctypes.data_as(C.U64P), 0, s.ctypes.data_as(C.U64P), None)):
            with pytest.raises(ValueError, match="null argument"):
                lib._check(fn(*args, out.ctypes.data_as(C.U64P), None))


# ---- the two-group fused re-extension ----
def run_reextend2(lib, W, va, vb, basis, d, shift_a, shift_b, shift, begin, count, out_offs=None, profile=False):
    n_out = count << d
    total = len(va) + len(vb)
    with C.Device(lib, W) as dev:
        pa, pb = dev.put(np.concatenate(va)), dev.put(np.concatenate(vb))
        outs = []
        for k in range(total):
            dev.off = 0 if out_offs is None else out_offs[k]
            outs.append(dev.empty(8 * W * n_out))
        if profile:
            lib.profile_begin()
        lib.additive_reextend2_batch_dev(pa, len(va), shift_a, pb, len(vb), shift_b, basis, d, shift, begin, count, outs, words=W)
        prof = lib.profile_report() if profile else None
        return [dev.get(o, n_out) for o in outs], prof


def reextend_shifts(m, W, kind):
    """(L's shift, group a's, group b's): the prover's case (a over the unshifted span, b over the first coset of L) or two seeded shifts outside L"""
    shift = M.elem(W, C.top(W) | (1 << m))
    if kind == "prover":
        return shift, M.elem(W, 0), shift
    return shift, seeded("re2 shift a %d" % m, 1, W)[0], seeded("re2 shift b %d" % m, 1, W)[0]


def windows(cosets):
    return sorted({(0, cosets), (1, cosets - 1) if cosets > 1 else (0, cosets), (cosets // 2, 1)})


def check_reextend2(lib, W, m, d, stage_bits=None, batches=REEXTEND_BATCHES):
    """under the smallest tiles: every pair of batch sizes, both kinds of shift, the coset windows; expected = the oracle's IFFT over each group's own
    coset followed by its FFT over L, and bit for bit the outputs of two one-group calls"""
    basis = oracle.standard_basis(m, W)
    nd, cosets = 1 << d, 1 << (m - d)
    va = [seeded("re2 a %d %d %d" % (m, d, k), nd, W) for k in range(3)]
    vb = [seeded("re2 b %d %d %d" % (m, d, k), nd, W) for k in range(3)]
    with B.options(lib, W, tiles=B.SMALLEST_TILES, stage_bits=stage_bits):
        for kind in ("prover", "seeded"):
            shift, sa, sb = reextend_shifts(m, W, kind)
            full_a = [oracle.additive_fft(oracle.additive_ifft(v, basis[:d], sa), basis, shift) for v in va]
            full_b = [oracle.additive_fft(oracle.additive_ifft(v, basis[:d], sb), basis, shift) for v in vb]
            for begin, count in windows(cosets):
                one_a, _ = B.run_reextend(lib, W, va, basis, d, sa, shift, begin, count)
                one_b, _ = B.run_reextend(lib, W, vb, basis, d, sb, shift, begin, count)
                for na, nb in batches:
                    got, _ = run_reextend2(lib, W, va[:na], vb[:nb], basis, d, sa, sb, shift, begin, count)
                    B.same(got, [f[begin * nd:(begin + count) * nd] for f in full_a[:na] + full_b[:nb]], (NAME[W], m, d, kind, begin, count, na, nb, "oracle"))
                    B.same(got, one_a[:na] + one_b[:nb], (NAME[W], m, d, kind, begin, count, na, nb, "one-group calls"))


def check_reextend2_staging_rounds(lib, W):
    """the staging of the forward passes lowered to two slots: a call of four vectors takes two rounds of vectors (d = 5) — and at d = 9, 2^10 elements"""
    check_reextend2(lib, W, 9, 5, stage_bits=6, batches=((3, 1), (2, 3)))
    check_reextend2(lib, W, 13, 9, stage_bits=10, batches=((3, 1),))


def check_reextend2_alignment(lib, W):
    """one output of four at 8 mod 16: the launch that sees the outputs takes the 64-bit form (one access path at one word), same bytes"""
    m, d = 7, 5
    basis = oracle.standard_basis(m, W)
    shift, sa, sb = reextend_shifts(m, W, "prover")
    va = [seeded("re2 align a %d" % k, 1 << d, W) for k in range(3)]
    vb = [seeded("re2 align b", 1 << d, W)]
    with B.options(lib, W, tiles=B.SMALLEST_TILES):
        want, _ = run_reextend2(lib, W, va, vb, basis, d, sa, sb, shift, 0, 4)
        got, prof = run_reextend2(lib, W, va, vb, basis, d, sa, sb, shift, 0, 4, out_offs=[0, 0, 8, 0], profile=True)
    B.same(got, want, (NAME[W], "one output at 8"))
    rows = B.field_rows(prof, W)
    if W > 1:
        assert STEM[W] + "bfly_edge_batch_w64" in rows and STEM[W] + "bfly_edge_batch" not in rows, rows
    assert STEM[W] + "bfly_edge_inv_batch" in rows, rows


def check_reextend2_profile(lib, W):
    """no phase-1 row; the forward launches do not depend on the batch sizes; each group has its own first inverse pass"""
    m, d = 10, 9
    basis = oracle.standard_basis(m, W)
    shift, sa, sb = reextend_shifts(m, W, "prover")
    va = [seeded("re2 prof a %d" % k, 1 << d, W) for k in range(2)]
    vb = [seeded("re2 prof b %d" % k, 1 << d, W) for k in range(3)]
    rows = {}
    with B.options(lib, W, tiles=B.SMALLEST_TILES):
        run_reextend2(lib, W, va, vb, basis, d, sa, sb, shift, 0, 2)                 # the plan's tables are built outside the profiles
        for na, nb in ((1, 1), (2, 3)):
            _, prof = run_reextend2(lib, W, va[:na], vb[:nb], basis, d, sa, sb, shift, 0, 2, profile=True)
            rows[(na, nb)] = B.field_rows(prof, W)
    s = STEM[W]
    assert rows[(1, 1)] == {s + "bfly_edge_inv_batch": 2, s + "bfly_upper_inv_batch": 8, s + "bfly_upper_batch": 4, s + "bfly_edge_batch": 1}, rows
    assert rows[(2, 3)] == rows[(1, 1)], rows
    assert not [k for r in rows.values() for k in r if "phase1" in k]


def check_reextend2_refusals(lib, W):
    m, d = 5, 3
    basis, shift = oracle.standard_basis(m, W), M.elem(W, 1 << m)
    with C.Device(lib, W) as dev:
        p = dev.put(seeded("re2 refused", 4 << m, W))
        q = p + 8 * W * (1 << m)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_reextend2_batch_dev(0, 1, shift, p, 1, shift, basis, d, shift, 0, 1, [q, q], words=W)
        with pytest.raises(ValueError, match="null buffer"):
            lib.additive_reextend2_batch_dev(p, 1, shift, p, 1, shift, basis, d, shift, 0, 1, [q, 0], words=W)
        with pytest.raises(ValueError, match=r"batch sizes 0 \+ 1 outside 1\.\.65535"):
            lib.additive_reextend2_batch_dev(p, 0, shift, p, 1, shift, basis, d, shift, 0, 1, [q], words=W)
        for bad_d in (0, m + 1):
            with pytest.raises(ValueError, match="the evaluation domains must be spanned by the first basis vectors of the codeword domain"):
                lib.additive_reextend2_batch_dev(p, 1, shift, p, 1, shift, basis, bad_d, shift, 0, 1, [q, q], words=W)
        for begin, count in ((0, 0), (4, 1), (3, 2)):
            with pytest.raises(ValueError, match="outside the 4 cosets of the transform"):
                lib.additive_reextend2_batch_dev(p, 1, shift, p, 1, shift, basis, d, shift, begin, count, [q, q], words=W)


# ---- the native prover under IOPX_GFX_HEAD_EVAL=1 ----
NATIVE_CASES = [(7, 15, C.SEED, 5, 2), (9, 15, C.SEED, 5, 2), (7, 0, C.SEED, 5, 2), (7, 3, 7, 3, 3)]      # (log_n, inputs, seed, rs_extra, localization)
INTERACTIONS = {1: 3, 2: 2, 4: 1}          # FRI's interactive repetitions at these sizes (gfx_aurora_model.parameters)


def field_code(W):
    import libiop_amd as la
    return la.FIELD_GF64 if W == 1 else C.field_code(W)


def expected_transcript(W, inst, rs_extra=5, loc=2):
    """the model's over gf128 and gf256, the oracle's own prover over gf64"""
    if W == 1:
        return oracle.aurora_prove_csr(oracle.FIELD_GF64, inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"], rs_extra=rs_extra, localization=loc)
    return M.prove(W, inst, rs_extra, loc)


def short_instance(W, log_n=7, log_v=6, k=3, seed=9):
    """2^log_n constraints over 2^log_v - 1 variables: |V| != |C|, which the seeded example instances (n constraints, n - 1 variables) never give.  The
    constraints are gfx_aurora_model.example's, z[i mod nv] * z[(i + 7) mod nv] = coef_i * z[(2 i + 1) mod nv]."""
    n, nv = 1 << log_n, (1 << log_v) - 1
    z = M.seeded(W, seed, nv)
    i = np.arange(n)
    a, b, c = i % nv, (i + 7) % nv, (2 * i + 1) % nv
    zc = z[c].copy()
    c_zero = ~zc.any(axis=1)
    zc[c_zero] = M.elem(W, 1)
    coef = oracle.gf_mul(oracle.gf_mul(z[a], z[b]), oracle.gf_inv(zc))
    ones = np.ascontiguousarray(np.broadcast_to(M.elem(W, 1), (n, W)))
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    matrices = [(row_ptr, (a + 1).astype(np.uint32), ones), (row_ptr, (b + 1).astype(np.uint32), ones), (row_ptr, np.where(c_zero, 0, c + 1).astype(np.uint32), coef)]
    return {"matrices": matrices, "z": z, "num_variables": nv, "num_inputs": k}


def prove_profiled(lib, W, inst, rs_extra=5, loc=2, head=None):
    """(transcript, the profile's launch counts, the profile) of the second of two proofs (the first builds plans and tables)"""
    h = lib.aurora_instance(field_code(W), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
    try:
        with C.options(lib, **({} if head is None else {OPTION: head})):
            first = lib.aurora_prove(h, 128, rs_extra, loc)
            lib.profile_begin()
            mine = lib.aurora_prove(h, 128, rs_extra, loc)
            prof = lib.profile_report()
        assert first == mine
        return mine, prof
    finally:
        lib.aurora_instance_free(h)


def launches(prof, stem, name):
    return sum(prof[k][0] for k in (stem + name, stem + name + "_w64") if k in prof)


def declared(prof, stem, name):
    return sum(prof[k][2] for k in (stem + name, stem + name + "_w64") if k in prof)


def assert_head_ran(W, on, off, ldt_instances, interactions):
    s = STEM[W]
    assert on["k_count_mismatch_words"][0] == ldt_instances and "k_count_mismatch_words" not in off, (on.get("k_count_mismatch_words"), ldt_instances)
    assert launches(on, s, "div_by_vanishing") == 1 and launches(off, s, "div_by_vanishing") == 0
    assert launches(on, s, "polydiv_pass") == 0, "f_w went through the division passes"
    assert declared(on, s, "ldt_combine") * 4 <= declared(off, s, "ldt_combine"), (declared(on, s, "ldt_combine"), declared(off, s, "ldt_combine"))
    return s


def check_native_head(lib, W, case, inst=None):
    """option on: the expected bytes, the option-off proof's bytes, and a profile that shows the head route"""
    log_n, k, seed, rs_extra, loc = case
    if inst is None:
        inst = M.example(W, log_n, k, seed)
    want = expected_transcript(W, inst, rs_extra, loc)
    on, on_prof = prove_profiled(lib, W, inst, rs_extra, loc, head=1)
    off, off_prof = prove_profiled(lib, W, inst, rs_extra, loc, head=0)
    assert on == want, C.first_difference(on, want)
    assert off == want, C.first_difference(off, want)
    P = M.parameters(W, (len(inst["matrices"][0][0]) - 1).bit_length() - 1, inst["num_variables"], rs_extra, loc)
    s = assert_head_ran(W, on_prof, off_prof, P["num_output_LDT_instances"], P["fri_interactive_repetitions"])
    # the first inverse passes of the fused re-extensions, one per call and group: the f_w branch brings three (f_w' onto V0, then the four-vector call's
    # two groups, or f_w and the three Mz apart when |V| != |C|), each lincheck repetition three (its p_alpha pair onto the head, and the two of the
    # sumcheck's two-coset arm), and first_round_from_head ONE per LDT instance whatever the number of interactions (3 over gf64, 2 over gf128 at these sizes)
    assert P["fri_interactive_repetitions"] == INTERACTIONS[W]
    inv = launches(on_prof, s, "bfly_edge_inv_batch")
    assert inv == 3 + 3 * P["multi_lincheck_repetitions"] + P["num_output_LDT_instances"], (inv, P["multi_lincheck_repetitions"], P["num_output_LDT_instances"])
    return on_prof, off_prof


def check_native_head_short_instance(lib, W):
    inst = short_instance(W)
    assert M.parameters(W, 7, inst["num_variables"])["variable_domain_dim"] == 6
    check_native_head(lib, W, (7, 3, 9, 5, 2), inst=inst)


def check_unsatisfied(lib, W):
    """gfx_aurora_cases.flipped: the model's bytes for that assignment with the option on and off; on, the profile shows the head, then the differing
    confirmation window, then the whole-domain LDT combination"""
    inst = M.example(W, 6, 3, 5)
    good = expected_transcript(W, inst)
    bad = C.flipped(inst)
    want = expected_transcript(W, bad)
    assert want != good
    on, on_prof = prove_profiled(lib, W, bad, head=1)
    off, off_prof = prove_profiled(lib, W, bad, head=0)
    assert on == want, C.first_difference(on, want)
    assert off == want, C.first_difference(off, want)
    s = STEM[W]
    P = M.parameters(W, 6, inst["num_variables"])
    assert on_prof["k_count_mismatch_words"][0] >= 1 and "k_count_mismatch_words" not in off_prof
    # head and confirmation window per LDT instance, then every instance over the whole domain
    n = 1 << P["codeword_domain_dim"]
    whole = [k for k in on_prof if k.startswith(s + "ldt_combine")]
    assert launches(on_prof, s, "ldt_combine") >= 3 * P["num_output_LDT_instances"], on_prof
    assert declared(on_prof, s, "ldt_combine") > declared(off_prof, s, "ldt_combine") and whole, (n, on_prof)


def check_defaults_unchanged(lib, W):
    """the option unset: no row of the head route, the expected bytes"""
    inst = M.example(W, 7, 15, C.SEED)
    mine, prof = prove_profiled(lib, W, inst)
    assert mine == expected_transcript(W, inst)
    assert "k_count_mismatch_words" not in prof and not [k for k in prof if "div_by_vanishing" in k], prof


def check_other_fields_after_head_proofs(lib, torch, device):
    """after option-on proofs over the three fields in this process: gf192, gf64 (option off), edwards Fr and alt_bn128 Fr still give their bytes"""
    for W in WORDS:
        inst = M.example(W, 6, 3, 5)
        on, _ = prove_profiled(lib, W, inst, head=1)
        assert on == expected_transcript(W, inst)
    C.check_other_fields_unchanged(lib, torch, device)


def check_warm_with_the_option(lib, W):
    """iopx_aurora_instance_warm with the option on builds the head route's tables: the proof after it uploads no table and gives the bytes"""
    inst = M.example(W, 7, 15, C.SEED)
    h = lib.aurora_instance(field_code(W), inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"])
    try:
        with C.options(lib, **{OPTION: 1}):
            lib.aurora_instance_warm(h)
            lib.profile_begin()
            mine = lib.aurora_prove(h)
            prof = lib.profile_report()
    finally:
        lib.aurora_instance_free(h)
    assert mine == expected_transcript(W, inst)
    assert launches(prof, STEM[W], "div_by_vanishing") == 1


# ---- recorded digests ----
def check_native_digest(lib, W):
    """option on: the 2^12 digests of tests/golden/gfx_aurora.json (gf128, gf256); over gf64 the oracle's recorded digest at 2^18, the largest size the
    existing gf64 GPU tests prove (tests/golden/gf64_aurora.json)"""
    with C.options(lib, **{OPTION: 1}):
        if W == 1:
            import gf64_aurora_cases as G
            lib.profile_begin()
            G.check_native_digest(lib, 18, 15)
            assert launches(lib.profile_report(), STEM[W], "div_by_vanishing") == 1
            return
        pin, inst = C.digest_instance(W)
        lib.profile_begin()
        mine = C.native_prove(lib, W, inst)
        assert launches(lib.profile_report(), STEM[W], "div_by_vanishing") == 1
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])
