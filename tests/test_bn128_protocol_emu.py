"""The alt_bn128 Fr protocol-layer kernels (k_bn_* of virtual_oracles.hip, encoded_ops.hip, fractal_ops.hip) compiled for the CPU
(tests/emu) against values computed with Python integers only (tests/bn128_protocol_cases.py): every tiny case of
tests/golden/bn128_protocol_tiny.json, the digest recipes at m = 10 and 12, the model's own check against the edwards_Fr entries,
raw (non-canonical) data words, the argument checks and the host scalars.  The GPU leg is tests/test_gpu_bn128_protocol.py."""
import ctypes

import numpy as np
import pytest

import bn128_protocol_cases as C
from emu_lib import emu

_u64p = ctypes.POINTER(ctypes.c_uint64)


def test_tiny_cases():
    want = C.load_json("bn128_protocol_tiny.json")["cases"]
    got = C.run_tiny(emu())
    assert sorted(got) == sorted(want)
    bad = sorted(k for k in want if got[k] != want[k])
    assert not bad, bad


@pytest.mark.parametrize("m", [10, 12])
def test_digest_recipes(m):
    want = C.load_json("bn128_protocol_digests_large.json")["cases"]
    for name, out in C.run_large(emu(), m):
        assert C.digest(out) == want[name]["digest"], name


def test_model_reproduces_the_edwards_entries():
    """the same model with edwards_Fr's parameters against the *_fp3_dev entries (oracle-checked elsewhere): tiny cases and m = 10"""
    lib = emu()
    bad = []
    for c in C.tiny_cases(C.ED) + C.large_cases(C.ED, 10):
        inp = C.inputs(C.ED, c)
        got, want = C.run_case(lib, C.ED, c, inp), C.model_words(C.ED, c, inp)
        if len(got) != len(want) or not all(np.array_equal(g, w) for g, w in zip(got, want)):
            bad.append(c["name"])
    assert not bad, bad


def test_raw_data_words():
    C.check_raw_words(emu())


def test_in_place_elementwise():
    """mul / sub / inv allow d_out to alias an input, as their edwards_Fr twins do"""
    lib = emu()
    F = C.BN
    for op in ("mul", "sub", "inv"):
        c = {"op": op, "name": "alias " + op, "n": 1031, "zeros": "some"}
        inp = C.inputs(F, c)
        want = C.model_words(F, c, inp)[0]
        d = lib.malloc(inp["a"].nbytes)
        db = lib.malloc(inp["a"].nbytes)
        try:
            lib.h2d(d, inp["a"])
            if op != "inv":
                lib.h2d(db, inp["b"])
                getattr(lib, "bn128_%s_dev" % op)(d, db, d, c["n"])
            else:
                lib.bn128_inv_dev(d, d, c["n"])
            out = np.empty_like(inp["a"])
            lib.d2h(out, d)
        finally:
            lib.free(d)
            lib.free(db)
        assert np.array_equal(out, want), op


def test_argument_checks():
    lib = emu()
    F = C.BN
    one, g = F.elem(1), F.elem(F.gen(4))
    p = lambda a: a.ctypes.data_as(_u64p)                                           # noqa: E731
    buf = lib.malloc(32 * 64)
    v = ctypes.c_void_p(buf)
    try:
        # log_n / log_order above the 2-adicity (28)
        for call in (lambda: lib.c.iopx_rowcheck_bn128_dev(v, v, v, 29, p(g), p(one), 2, p(one), v),
                     lambda: lib.c.iopx_fz_bn128_dev(v, v, 29, p(g), p(one), 2, p(one), v),
                     lambda: lib.c.iopx_sumcheck_g_bn128_dev(v, v, 29, p(g), p(one), 2, p(one), p(one), v),
                     lambda: lib.c.iopx_rational_sumcheck_constraint_bn128_dev(v, v, v, 29, p(g), p(one), 2, p(one), p(one), v),
                     lambda: lib.c.iopx_domain_offsets_bn128_dev(29, p(g), p(one), p(one), v),
                     lambda: lib.c.iopx_vanishing_evals_bn128_dev(29, p(g), p(one), 2, p(one), p(one), v),
                     lambda: lib.c.iopx_poly_div_vanishing_bn128_dev(v, 64, 29, p(one), v)):
            with pytest.raises(ValueError, match="2-adicity"):
                lib._check(call())
        # the twins' refusals, same error class: sub-domain larger than the domain, intersecting domains, limits, aliasing, null
        with pytest.raises(ValueError, match="sub-domain"):
            lib._check(lib.c.iopx_rowcheck_bn128_dev(v, v, v, 4, p(g), p(F.elem(5)), 5, p(one), v))
        with pytest.raises(ValueError, match="intersects"):
            lib._check(lib.c.iopx_rowcheck_bn128_dev(v, v, v, 4, p(g), p(one), 2, p(one), v))
        with pytest.raises(ValueError, match="intersects"):
            lib._check(lib.c.iopx_rational_sumcheck_constraint_bn128_dev(v, v, v, 4, p(g), p(one), 2, p(one), p(one), v))
        with pytest.raises(ValueError, match="bigger"):
            lib._check(lib.c.iopx_fz_bn128_dev(v, v, 4, p(g), p(one), 5, p(one), v))
        with pytest.raises(ValueError, match="zero coset shift"):
            lib._check(lib.c.iopx_sumcheck_g_bn128_dev(v, v, 4, p(g), p(F.elem(0)), 2, p(one), p(one), v))
        coeffs = F.to_words([F.enc(3)] * 17)
        ptrs = (ctypes.c_void_p * 17)(*[buf] * 17)
        with pytest.raises(ValueError, match="constituent"):
            lib._check(lib.c.iopx_lincheck_bn128_dev(v, ptrs, 9, p(coeffs), v, v, 16, v))
        with pytest.raises(ValueError, match="Expected same number"):
            lib._check(lib.c.iopx_lincomb_bn128_dev(ptrs, 17, p(coeffs), 16, v))
        with pytest.raises(ValueError, match="Expected same number"):
            lib._check(lib.c.iopx_lincomb_affine_bn128_dev(ptrs, 0, p(coeffs), p(one), 16, v))
        with pytest.raises(ValueError, match="null"):
            lib._check(lib.c.iopx_lincomb_affine_bn128_dev(ptrs, 2, p(coeffs), None, 16, v))
        with pytest.raises(ValueError, match="Expected same number"):
            lib._check(lib.c.iopx_rational_combine_bn128_dev(ptrs, ptrs, 5, p(coeffs), 16, v, v))
        with pytest.raises(ValueError, match="alias"):
            lib._check(lib.c.iopx_bn128_div_dev(None, v, v, 16))
        with pytest.raises(ValueError, match="alias"):
            lib._check(lib.c.iopx_bn128_div_dev(v, ctypes.c_void_p(buf + 32 * 32), v, 16))
        for call in (lambda: lib.c.iopx_bn128_mul_dev(v, None, v, 4), lambda: lib.c.iopx_bn128_sub_dev(None, v, v, 4),
                     lambda: lib.c.iopx_bn128_inv_dev(v, None, 4), lambda: lib.c.iopx_bn128_pow_table_dev(v, 4, None, p(one)),
                     lambda: lib.c.iopx_spmv_bn128_dev(None, v, v, 4, v, None, 0, v), lambda: lib.c.iopx_rowcheck_bn128_dev(v, v, v, 4, None, p(one), 2, p(one), v)):
            with pytest.raises(ValueError, match="null"):
                lib._check(call())
        # the same refusals from the edwards_Fr twins: one host implementation
        E = C.ED
        with pytest.raises(ValueError, match="intersects"):
            lib._check(lib.c.iopx_rowcheck_fp3_dev(v, v, v, 4, p(E.elem(E.gen(4))), p(E.elem(1)), 2, p(E.elem(1)), v))
        with pytest.raises(ValueError):
            lib._check(lib.c.iopx_rowcheck_fp3_dev(v, v, v, 32, p(E.elem(E.gen(4))), p(E.elem(1)), 2, p(E.elem(1)), v))
    finally:
        lib.free(buf)


def test_host_scalars():
    lib = emu()
    F = C.BN
    a, b = C.seeded_scalar("protocol host a"), C.seeded_scalar("protocol host b")
    assert F.to_ints(lib.bn128_host_add(F.elem(a), F.elem(b))) == [F.enc(a + b)]
    assert F.to_ints(lib.bn128_host_sub(F.elem(a), F.elem(b))) == [F.enc(a - b)]
    assert F.to_ints(lib.bn128_host_sub(F.elem(b), F.elem(a))) == [F.enc(b - a)]
    assert F.to_ints(lib.bn128_host_add(F.elem(F.p - 1), F.elem(1))) == [0]
    assert lib.bn128_modulus() == F.p


# ---- DeviceOps over AltBn128Fr (CPU torch tensors on the CPU build, as the other *_emu tests construct it) -------------------------
class _Csr:
    def __init__(self, ops, torch, inp, rows):
        self.rows = rows
        self.d_row_ptr, self.d_col = ops.upload_raw(inp["row_ptr"].view(np.int64), torch.int64), ops.upload_raw(inp["col"].view(np.int32), torch.int32)
        self.d_coeff = ops.upload(inp["coeff"])


def test_device_ops_over_alt_bn128():
    import torch
    from libiop_amd import domains
    F, field = C.BN, domains.AltBn128Fr()
    ops = domains.DeviceOps(emu(), torch, torch.device("cpu"), field)
    assert type(ops).__name__ == "AltBn128DeviceOps" and ops.empty(3).shape == (3, 4)
    log_n, sub = 6, 3
    L, S = field.domain(1 << log_n, shift=F.generator), field.domain(1 << sub, shift=C.seeded_scalar("ops sub shift"))
    assert F.to_ints(L.gen) == [F.enc(F.gen(log_n))] and F.to_ints(L.shift) == [F.enc(F.generator)]

    def check(case, run):
        case = dict(case, name="ops " + case["op"])
        inp = C.inputs(F, case)
        d = {k: ops.upload(v) for k, v in inp.items() if k not in ("row_ptr", "col")}
        got = run(case, inp, d)
        got = got if isinstance(got, tuple) else (got,)
        want = C.model_words(F, case, inp)
        assert all(np.array_equal(ops.download(g), w) for g, w in zip(got, want)), case["op"]

    dom = {"log_n": log_n, "shift": F.generator, "sub_log": sub, "sub_shift": S.shift_int, "mu": C.seeded_scalar("ops mu"), "constant": C.seeded_scalar("ops c")}
    cs = [C.seeded_scalar("ops coeff %d" % i) for i in range(5)]
    cw = lambda vals: np.stack([field.from_int(v) for v in vals])                   # noqa: E731
    check(dict(dom, op="rowcheck"), lambda c, i, d: ops.rowcheck(d["a"], d["b"], d["c"], L, S))
    check(dict(dom, op="fz"), lambda c, i, d: ops.fz(d["a"], d["b"], L, S))
    check(dict(dom, op="sumcheck_g"), lambda c, i, d: ops.sumcheck_g(d["a"], d["b"], L, S, field.from_int(c["mu"])))
    check(dict(dom, op="rational_sumcheck_constraint"), lambda c, i, d: ops.rational_sumcheck_constraint(d["a"], d["b"], d["c"], L, S, field.from_int(c["mu"])))
    check(dict(dom, op="vanishing_evals"), lambda c, i, d: ops.vanishing_evals(S, L, field.from_int(c["constant"])))
    check({"op": "domain_offsets", "log_n": log_n, "shift": F.generator, "point": cs[0]}, lambda c, i, d: ops.domain_offsets(L, field.from_int(cs[0])))
    check({"op": "pow_table", "n": 1 << log_n, "base": F.gen(log_n), "init": F.generator}, lambda c, i, d: ops.domain_elements(L))
    check({"op": "lincheck", "n": 64, "num": 3, "coeffs": cs[:3]}, lambda c, i, d: ops.lincheck(d["a"], [d["m0"], d["m1"], d["m2"]], cw(cs[:3]), d["b"], d["c"], 64))
    check({"op": "lincomb", "n": 64, "num": 5, "coeffs": cs}, lambda c, i, d: ops.lincomb([d["m%d" % k] for k in range(5)], cw(cs), 64))
    check({"op": "lincomb_affine", "n": 64, "num": 2, "coeffs": cs[:2], "constant": cs[4]},
          lambda c, i, d: ops.lincomb_affine([d["m0"], d["m1"]], cw(cs[:2]), field.from_int(cs[4]), 64))
    check({"op": "rational_combine", "n": 64, "num": 2, "coeffs": cs[:2]}, lambda c, i, d: ops.rational_combine([d["n0"], d["n1"]], [d["d0"], d["d1"]], cw(cs[:2]), 64))
    check({"op": "mul", "n": 70}, lambda c, i, d: ops.mul(d["a"], d["b"]))
    check({"op": "sub", "n": 70}, lambda c, i, d: ops.sub(d["a"], d["b"]))
    check({"op": "inv", "n": 70, "zeros": "some"}, lambda c, i, d: ops.inv(d["a"]))
    check({"op": "div", "n": 70, "zeros": "some", "with_num": 1}, lambda c, i, d: ops.div(d["a"], d["b"]))
    check({"op": "div", "n": 70, "zeros": "none", "with_num": 0}, lambda c, i, d: ops.div(None, d["b"]))
    check({"op": "poly_div_vanishing", "n_coeffs": 30, "sub_log": sub, "shift": S.shift_int}, lambda c, i, d: ops.poly_div_vanishing(d["a"], 30, S))
    check({"op": "spmv", "rows": 40, "cols": 33, "shape": "mixed", "scale": cs[1], "accumulate": 1},
          lambda c, i, d: ops.spmv(_Csr(ops, torch, i, 40), d["vec"], d_out=d["out"], scale=field.from_int(cs[1]), accumulate=True))
    # the operators that already had alt_bn128 entries: a round trip, a fold against the host-pointer entry, trees and queries on 32-byte elements
    lib = emu()
    coeffs = C.data_words("ops coeffs", 16)
    code = ops.FFT(ops.upload(coeffs), 16, L)
    assert np.array_equal(ops.download(code), lib.multiplicative_FFT_bn128(coeffs, log_n, L.shift))
    assert np.array_equal(ops.download(ops.IFFT(code, L))[:16], coeffs)
    assert np.array_equal(ops.download(ops.IFFT_of_known_degree(code, 16, L)), coeffs)
    assert all(np.array_equal(ops.download(t), ops.download(code)) for t in ops.FFT_batch([ops.upload(coeffs)] * 2, 16, L))
    x = field.from_int(C.seeded_scalar("ops fold x"))
    assert np.array_equal(ops.download(ops.fold(code, L, 2, x)), lib.multiplicative_evaluate_next_f_i_bn128(ops.download(code), L.shift, 2, x))
    rc = cw([C.seeded_scalar("ops ldt %d" % k) for k in range(2)])
    assert np.array_equal(ops.download(ops.ldt_combine([code], [16], rc, L)), lib.ldt_combine_bn128([ops.download(code)], [16], rc, L.shift))
    tree = ops.merkle_tree([code], L, 2)
    assert tree.num_leaves == 32 and len(tree.root()) == 32
    assert np.array_equal(ops.query_responses([code], L, [0, 5, 63])[:, 0, :], ops.download(code)[[0, 5, 63]])


def test_alt_bn128_host_scalars():
    from libiop_amd import domains
    f, p = domains.AltBn128Fr(), C.BN.p
    a, b = C.seeded_scalar("field a"), C.seeded_scalar("field b")
    A, Bw = f.from_int(a), f.from_int(b)
    assert C.BN.to_ints(A) == [C.BN.enc(a)] and f.to_int(A) == a and f.to_int(f.one()) == 1 and not f.zero().any() and f.zero().shape == (4,)
    assert f.to_int(f.mul(A, Bw)) == a * b % p and f.to_int(f.add(A, Bw)) == (a + b) % p and f.to_int(f.sub(A, Bw)) == (a - b) % p
    assert f.to_int(f.neg(A)) == -a % p and f.to_int(f.inv(A)) == pow(a, -1, p)
    S = f.domain(16, shift=b)
    assert f.to_int(f.vanishing_eval(S, A)) == (pow(a, 16, p) - pow(b, 16, p)) % p
    assert f.to_int(f.vanishing_derivative(S, A)) == 16 * pow(a, 15, p) % p
    assert f.element_in_domain(S, f.from_int(b * pow(C.BN.gen(4), 5, p))) and not f.element_in_domain(S, A)
    chain = f.fri_domains(f.domain(64, shift=5), [2, 1])
    assert [(d.dim, d.shift_int) for d in chain] == [(6, 5), (4, pow(5, 4, p)), (3, pow(5, 8, p))]
    assert S.element_outside_of_subset() == b * 5 % p
    with pytest.raises(NotImplementedError):
        f.squeeze(None, 1)
    with pytest.raises(ValueError, match="2-adicity"):
        f.domain(1 << 29)
