"""Cases for Fractal over GF(2^128) and GF(2^256) under IOPX_GFX_FRACTAL_WIDE=1 — the model tests/gfx_fractal_model.py held to the oracle at one and
three words, then the native prover, the Python prover over GF128FractalOps / GF256FractalOps and the refusals that stay held to the model at two
and four — and for the two forms of the rational combination over GF(2^128) and GF(2^256) (csrc/gfx_ops.h: kx_rational_combine, one rational after the
other with inlined products, and kx_rational_combine_lean, the same recurrence through one product site on values kept in register form), chosen
per launch by the option IOPX_GFX_RATIONAL_FORM (1 / 2; 0 is the field's measured default).  Shared by tests/test_gfx_fractal_wide_emu.py (CPU
emulation) and tests/test_gpu_gfx_fractal_wide.py (MI355X): every function takes the Library under test.

Every comparison is byte equality with gfx_fractal_cases.rational_expected (oracle.gf_mul and XOR, term by term: neither form's recurrence), and
every launch is held to the one profile row of its field and placement and to its declared bytes, (2 r + 2) n E.  The option is not something a
launch can be seen to obey from its outputs (both forms give the same bytes under the same row), so check_lean_form_is_built looks for the
kernel's name in the library that was loaded."""
import hashlib
import json
import os

import numpy as np
import pytest

import gf64_aurora_cases as G64
import gfx_aurora_cases as C
import gfx_fractal_cases as F
import gfx_fractal_model as FM
import oracle

WORDS = C.WORDS                                     # (2, 4): the lean form is instantiated for the elements of several words
NAME = C.NAME
OPTION = "IOPX_GFX_RATIONAL_FORM"
FORMS = (1, 2)
SIZES = (1, 2, 255, 256, 257, 1000)                 # one lane, two, a workgroup less one, a workgroup, one more, four ragged workgroups
COUNTS = (1, 2, 3, 4)
STRIDE_N = (1 << 11) + 3                            # under grid caps 2 and 3: a third (fifth) trip of the grid-stride loop and a ragged tail
LEAN_KERNEL = b"kx_rational_combine_lean"

_EXPECTED = {}


def instance(W, num, n, tag="wide"):
    """(numerators, denominators, coefficients, the expected pair), computed once per shape and shared by both forms and every placement"""
    key = (W, num, n, tag)
    if key not in _EXPECTED:
        Ns = [F.seeded("%s N %d %d %d" % (tag, num, n, i), n, W) for i in range(num)]
        Ds = [F.seeded("%s D %d %d %d" % (tag, num, n, i), n, W) for i in range(num)]
        coef = F.seeded("%s c %d %d" % (tag, num, n), num, W)
        _EXPECTED[key] = (Ns, Ds, coef, F.rational_expected(Ns, Ds, coef))
    return _EXPECTED[key]


def both_forms(lib, W, Ns, Ds, coef, want, placements, why):
    num, n = len(Ns), Ns[0].shape[0]
    vectors = 2 * num + 2
    for form in FORMS:
        with C.options(lib, **{OPTION: form}):
            for offs in placements:
                got, prof = F.run(lib, W, Ns + Ds, offs, [n, n], F.rational_call(lib, W, num, coef, n))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (NAME[W], form, num, n, offs, why)
                F.assert_one_row(prof, W, "rational_combine", bool(any(offs)), n * 8 * W * vectors, (form, num, n, offs, why))


def check_forms(lib, W, num, n):
    """every vector on a 16-byte boundary, every vector 8 bytes past one, and each vector of the launch alone off it"""
    Ns, Ds, coef, want = instance(W, num, n)
    both_forms(lib, W, Ns, Ds, coef, want, F.placements(2 * num + 2), "placements")


def check_strides(lib, W):
    """2^11 + 3 elements under IOPX_GFX_OPS_MAX_BLOCKS = 2 and 3 (512 and 768 lanes): five and three trips of the grid-stride loop, the last ragged"""
    for num in (2, 4):
        Ns, Ds, coef, want = instance(W, num, STRIDE_N, "wide stride")
        for cap in (2, 3):
            with C.options(lib, IOPX_GFX_OPS_MAX_BLOCKS=cap):
                both_forms(lib, W, Ns, Ds, coef, want, [(0,) * (2 * num + 2), (8,) * (2 * num + 2)], "cap %d" % cap)


def check_zeros(lib, W):
    """zero coefficients (one, and all of them), zero denominators (in one rational, in the first, in all at one position) and zero numerators: the
    products with zero operands go through the same site as every other"""
    num, n = 3, 257
    Ns, Ds, coef, _ = instance(W, num, n, "wide zeros")
    Ds = [d.copy() for d in Ds]
    Ns = [v.copy() for v in Ns]
    Ds[1][5] = 0
    Ds[0][0] = 0
    Ds[2][n - 1] = 0
    for d in Ds:
        d[100] = 0
    Ns[0][7] = 0
    Ns[2][256] = 0
    places = [(0,) * (2 * num + 2), (8,) * (2 * num + 2)]
    for tag, c in (("none", coef), ("middle", _with_zero(coef, (1,))), ("first", _with_zero(coef, (0,))), ("all", _with_zero(coef, (0, 1, 2)))):
        want = F.rational_expected(Ns, Ds, c)
        if tag == "all":
            assert not want[0].any()
        both_forms(lib, W, Ns, Ds, c, want, places, "zero coefficients: " + tag)


def _with_zero(coef, which):
    c = coef.copy()
    for i in which:
        c[i] = 0
    return c


def check_output_over_first_input(lib, W):
    """the combined numerator written over the first numerator and the combined denominator over the first denominator: a lane has read position j
    of every input before it writes position j, in either form, and the entry refuses no aliasing"""
    for num in (1, 4):
        n = 257
        Ns, Ds, coef, want = instance(W, num, n)
        for form in FORMS:
            for off in C.OFFSETS:
                with C.options(lib, **{OPTION: form}), C.Device(lib, W, off) as dev:
                    pN, pD = [dev.put(a) for a in Ns], [dev.put(a) for a in Ds]
                    lib.profile_begin()
                    lib.rational_combine_dev(pN, pD, coef, n, pN[0], pD[0], words=W)
                    prof = lib.profile_report()
                    assert np.array_equal(dev.get(pN[0], n), want[0]) and np.array_equal(dev.get(pD[0], n), want[1]), (NAME[W], form, num, off)
                    for k in range(1, num):
                        assert np.array_equal(dev.get(pN[k], n), Ns[k]) and np.array_equal(dev.get(pD[k], n), Ds[k]), (NAME[W], form, num, off, k)
                    F.assert_one_row(prof, W, "rational_combine", bool(off), n * 8 * W * (2 * num + 2), (form, num, off))


def check_form_refusals(lib, W):
    """0 and 5 rationals, a null oracle and a null output are refused in the same words under either form"""
    for form in FORMS:
        with C.options(lib, **{OPTION: form}):
            F.check_rational_refusals(lib, W)


def check_option_range(lib, W):
    """values outside 0..2 are clamped as every ranged option is: 3 is the lean form, -1 the field's choice; the bytes do not move"""
    Ns, Ds, coef, want = instance(W, 2, 255)
    for value in (0, 3, -1):
        with C.options(lib, **{OPTION: value}):
            got, prof = F.run(lib, W, Ns + Ds, (0,) * 6, [255, 255], F.rational_call(lib, W, 2, coef, 255))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (NAME[W], value)
            F.assert_one_row(prof, W, "rational_combine", False, 255 * 8 * W * 6, value)


def check_lean_form_is_built(lib):
    """the loaded library holds the lean kernel for both wide elements, in its 16-byte and 64-bit-word instantiations: the name as the compiler
    mangles it, with the element's name behind it (a host stub and the registered device name on the MI355X build, the function itself on the CPU
    build).  Without this the option would be a name nobody reads and both 'forms' of the cases above the same kernel."""
    with open(lib.path, "rb") as f:
        image = f.read()
    for elem in (b"Elem128", b"Elem256"):
        for a16 in (b"Lb1E", b"Lb0E"):
            needle = b"%d%sINS_%d%sE%s" % (len(LEAN_KERNEL), LEAN_KERNEL, len(elem), elem, a16)
            assert needle in image, needle


# ---- the Fractal model, and the provers over gf128 and gf256 under IOPX_GFX_FRACTAL_WIDE=1 ----
WIDE_OPTION = "IOPX_GFX_FRACTAL_WIDE"
SEED = F.SEED
TRUST_WORDS = (1, 3)
ORACLE_FIELD = {1: oracle.FIELD_GF64, 3: oracle.FIELD_GF192}
TRUST_TUPLES = F.NATIVE_TUPLES
NATIVE_TUPLES = [(6, 3, 3, 2), (7, 15, 2, 3)]                     # (log_n, inputs, rs_extra, localization) at SEED
PYTHON_TUPLE = (6, 3, 3, 2)
FRACTAL_OPERATORS = ("div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine", "rational_sumcheck_constraint")

_MODEL = {}


def model(W, case):
    """(transcript, index roots, instance) of the model on the seeded instance, degree check on: computed once per tuple and shared"""
    if (W, case) not in _MODEL:
        log_n, k, rs_extra, loc = case
        _MODEL[(W, case)] = FM.prove_example(W, log_n, k, SEED, rs_extra, loc, check_degrees=True)
    return _MODEL[(W, case)]


def hand_built_system(W):
    """gf64_aurora_cases.hand_built_system at W words: 64 constraints over 63 variables, (z_a + c1 z_a') * (c2 z_b or the constant c2) = coef z_c, so
    A has two entries per row and the index domain is twice the matrix domain; (system, rs_extra, localization)"""
    n, k = 64, 3
    z = C.seeded("hand-built z", n - 1, W)
    z[~z.any(axis=1)] = FM.elem(W, 1)
    full = np.concatenate([FM.elem(W, 1).reshape(1, W), z])
    i = np.arange(n)
    a1, a2, b, c = i % (n - 1) + 1, (3 * i + 5) % (n - 1) + 1, np.where(i % 5 == 0, 0, (i + 11) % (n - 1) + 1), (2 * i + 1) % (n - 1) + 1
    c1, c2 = C.seeded("hand-built c1", n, W), C.seeded("hand-built c2", n, W)
    az = full[a1] ^ oracle.gf_mul(c1, full[a2])
    bz = oracle.gf_mul(c2, full[b])
    coef = oracle.gf_mul(oracle.gf_mul(az, bz), oracle.gf_inv(full[c]))
    ones = np.ascontiguousarray(np.broadcast_to(FM.elem(W, 1), (n, W)))
    A = (2 * np.arange(n + 1, dtype=np.uint64), np.stack([a1, a2], axis=1).reshape(-1).astype(np.uint32), np.stack([ones, c1], axis=1).reshape(-1, W))
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    return {"matrices": [A, (row_ptr, b.astype(np.uint32), c2), (row_ptr, c.astype(np.uint32), coef)], "z": z, "num_variables": n - 1, "num_inputs": k}, 3, 2


def flipped_assignment(system):
    bad = system["z"].copy()
    bad[system["num_inputs"] + 17, 0] ^= np.uint64(1 << 63)        # auxiliary[17]
    return bad


def model_accepts(W, state, system, assignment):
    """the model's transcript for the assignment and whether every oracle of the LDT reducer keeps its degree bound"""
    stats = {}
    transcript = FM.prove(W, state, system, assignment, check_degrees="report", stats=stats)
    if stats["degree_failures"]:
        with pytest.raises(FM.DegreeCheckFailed):               # the asserting form of the switch
            FM.prove(W, state, system, assignment, check_degrees=True)
    return transcript, not stats["degree_failures"]


_HAND = {}


def hand_built_model(W):
    """(system, rs_extra, loc, index roots, {good, bad: (assignment, the model's transcript, whether its degrees hold)}), once per width"""
    if W not in _HAND:
        system, rs_extra, loc = hand_built_system(W)
        state, roots = FM.index(W, system, 128, rs_extra, loc)
        runs = {name: (z,) + model_accepts(W, state, system, z) for name, z in (("good", system["z"]), ("bad", flipped_assignment(system)))}
        _HAND[W] = (system, rs_extra, loc, roots, runs)
    return _HAND[W]


# -- 1. the model reproduces the oracle at one and three words --
def check_model_reproduces_the_oracle(W, case):
    log_n, k, rs_extra, loc = case
    ref, ref_roots = oracle.fractal_prove(ORACLE_FIELD[W], log_n, k, SEED, rs_extra=rs_extra, localization=loc)
    mine, roots, inst = model(W, case)
    assert roots == ref_roots, "index Merkle roots differ"
    assert mine == ref, F.first_difference(mine, ref)
    want = oracle.fractal_params(ORACLE_FIELD[W], log_n, k, rs_extra=rs_extra, localization=loc)
    P = FM.params(W, FM.cs_shape(inst), 128, rs_extra, loc)
    for name in FM.PARAM_NAMES:
        assert P[name] == want[name], (case, name, P[name], want[name])
    assert P["localization_parameters"] == want["localization_parameters"]


def check_model_hand_built(W):
    """oracle.fractal_prove_csr's roots and bytes for the satisfied and the flipped assignment, and the degree check agrees with the oracle's verifier
    on which of the two is accepted; at one word the system is gf64_aurora_cases.hand_built_system itself, at three its twin hand_built_system(3)"""
    if W == 1:
        matrices, z, k, rs_extra, loc = G64.hand_built_system()
        system = {"matrices": matrices, "z": z, "num_variables": z.shape[0], "num_inputs": k}
        state, roots = FM.index(1, system, 128, rs_extra, loc)
        systems = [(system, rs_extra, loc, roots, {name: (a,) + model_accepts(1, state, system, a) for name, a in (("good", z), ("bad", flipped_assignment(system)))})]
    else:
        systems = [hand_built_model(W)]
    for system, rs_extra, loc, roots, runs in systems:
        nv, k = system["num_variables"], system["num_inputs"]
        for name, (z, mine, degrees_hold) in runs.items():
            ref, ref_roots = oracle.fractal_prove_csr(ORACLE_FIELD[W], system["matrices"], nv, k, z, rs_extra=rs_extra, localization=loc)
            assert roots == ref_roots and mine == ref, (name,) + F.first_difference(mine, ref)
            accepted = oracle.fractal_verify_csr(ORACLE_FIELD[W], system["matrices"], nv, k, z[:k], mine, roots, rs_extra=rs_extra, localization=loc)
            assert accepted == degrees_hold == (name == "good"), (name, accepted, degrees_hold)


# -- 2. the native prover equals the model at two and four words --
class native_instance:
    def __init__(self, lib, W, system, assignment=None):
        self.lib = lib
        self.h = lib.aurora_instance(C.field_code(W), system["matrices"], system["num_variables"], system["num_inputs"],
                                     system["z"] if assignment is None else assignment)

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        self.lib.aurora_instance_free(self.h)


def native_index_and_prove(lib, W, system, rs_extra, loc, assignment=None, proofs=1, warm=False, profile=False):
    with native_instance(lib, W, system, assignment) as h, C.options(lib, **{WIDE_OPTION: 1}):
        roots = [bytes(r) for r in lib.fractal_index(h, 128, rs_extra, loc)]
        if warm:
            lib.aurora_instance_warm(h, fractal=True, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
        out = []
        for _ in range(proofs):
            if profile:
                lib.profile_begin()
            out.append(lib.fractal_prove(h, 128, rs_extra, loc))
        return roots, out, lib.profile_report() if profile else None


def check_native_prover(lib, W, case):
    want, want_roots, inst = model(W, case)
    roots, (mine,), _ = native_index_and_prove(lib, W, inst, case[2], case[3])
    assert roots == want_roots, "index Merkle roots differ"
    assert mine == want, F.first_difference(mine, want)


def hand_built_digests(W):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfx_fractal_wide.json")) as f:
        return {e["field"]: e for e in json.load(f)["hand_built"]}[NAME[W]]


def check_hand_built_digests_are_the_models(W):
    """CPU leg: the recorded digests of the hand-built system are the model's, and its degree check passes the satisfied assignment and fails the other"""
    system, rs_extra, loc, want_roots, runs = hand_built_model(W)
    pin = hand_built_digests(W)
    assert (pin["rs_extra"], pin["localization"], pin["index_roots"]) == (rs_extra, loc, [r.hex() for r in want_roots])
    assert runs["good"][2] and not runs["bad"][2] and runs["good"][1] != runs["bad"][1]
    for name, (_, want, degrees_hold) in runs.items():
        assert pin["assignments"][name] == {"bytes": len(want), "sha256": hashlib.sha256(want).hexdigest(), "degrees_hold": degrees_hold}, name


def check_native_hand_built(lib, W, through_digest=False):
    """the model's roots and bytes for the satisfied assignment and for the flipped one; the model's degree check passes the first and fails the second.
    through_digest: against the model's recorded digests (the MI355X leg: the model's four proofs take tens of seconds at four words)"""
    system, rs_extra, loc = hand_built_system(W)
    if through_digest:
        pin = hand_built_digests(W)
        assert pin["assignments"]["good"]["degrees_hold"] and not pin["assignments"]["bad"]["degrees_hold"]
        for name, z in (("good", system["z"]), ("bad", flipped_assignment(system))):
            roots, (mine,), _ = native_index_and_prove(lib, W, system, rs_extra, loc, assignment=z)
            assert [r.hex() for r in roots] == pin["index_roots"]
            assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["assignments"][name]["bytes"], pin["assignments"][name]["sha256"]), name
        return
    system, rs_extra, loc, want_roots, runs = hand_built_model(W)
    assert runs["good"][2] and not runs["bad"][2] and runs["good"][1] != runs["bad"][1]
    for name, (z, want, _) in runs.items():
        roots, (mine,), _ = native_index_and_prove(lib, W, system, rs_extra, loc, assignment=z)
        assert roots == want_roots
        assert mine == want, (name,) + F.first_difference(mine, want)


def check_native_second_proof_and_warm(lib, W):
    case = NATIVE_TUPLES[0]
    want, want_roots, inst = model(W, case)
    roots, proofs, _ = native_index_and_prove(lib, W, inst, case[2], case[3], proofs=2)
    assert roots == want_roots and proofs == [want, want]
    roots, proofs, _ = native_index_and_prove(lib, W, inst, case[2], case[3], warm=True)
    assert roots == want_roots and proofs == [want]


def check_native_flipped_bit(lib, W):
    """one bit of one auxiliary element: the same index, another transcript"""
    case = NATIVE_TUPLES[0]
    want, want_roots, inst = model(W, case)
    bad = inst["z"].copy()
    bad[inst["num_inputs"] + 11, W - 1] ^= np.uint64(1)
    roots, (mine,), _ = native_index_and_prove(lib, W, inst, case[2], case[3], assignment=bad)
    assert roots == want_roots and mine != want and len(mine) == len(want)


# -- 3. the Python prover over GF128FractalOps / GF256FractalOps --
def fractal_ops(lib, torch, device, W):
    from libiop_amd import domains
    cls, parent = {2: (domains.GF128FractalOps, domains.GF128AuroraOps), 4: (domains.GF256FractalOps, domains.GF256AuroraOps)}[W]
    ops = cls(lib, torch, device, C.domain_field(W))
    assert isinstance(ops, parent)
    return ops


def check_python_prover(lib, torch, device, W):
    from libiop_amd import fractal, r1cs
    log_n, k, rs_extra, loc = PYTHON_TUPLE
    want, want_roots, inst = model(W, PYTHON_TUPLE)
    n = 1 << log_n
    with C.options(lib, **{WIDE_OPTION: 1}):                      # the host forms of Z_S answer under the option (cpp/device.hpp)
        ops = fractal_ops(lib, torch, device, W)
        cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, k, n - 1, SEED)
        assert np.array_equal(np.concatenate([primary, auxiliary]), inst["z"])
        params = fractal.FractalParameters(ops.field, cs, RS_extra_dimensions=rs_extra, FRI_localization_parameter=loc)
        prover_index, (roots, messages) = fractal.fractal_snark_indexer(ops, cs, params)
        mine = fractal.fractal_snark_prover(ops, prover_index, cs, primary, auxiliary, params).serialize()
    assert messages == [] and [bytes(r) for r in roots] == want_roots
    assert mine == want, F.first_difference(mine, want)


# -- 4. the profile of one native proof --
def check_native_profile(lib, W):
    """one proof shows each of the five Fractal kernels under the field's stem and no kernel of another field's"""
    case = NATIVE_TUPLES[0]
    _, _, inst = model(W, case)
    _, _, prof = native_index_and_prove(lib, W, inst, case[2], case[3], profile=True)
    for kernel in F.KERNELS:
        assert F.rows_of(prof, W, kernel), (kernel, sorted(prof))
    others = tuple(stem for w, stem in F.STEM.items() if w != W)
    foreign = [k for k in prof if k.startswith(others) or k.endswith(("_gf192", "_fp3")) or k.startswith("k_bn_")]
    assert not foreign, foreign


# -- 5. the recorded digests (tools/make_gfx_fractal_wide_digests.py) --
def golden_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfx_fractal_wide.json")) as f:
        return {e["field"]: e for e in json.load(f)["fractal"]}


def check_native_digest(lib, W):
    pin = golden_digests()[NAME[W]]
    assert pin["seed"] == SEED
    inst = FM.example(W, pin["log_n"], pin["num_inputs"], SEED)
    roots, (mine,), _ = native_index_and_prove(lib, W, inst, pin["rs_extra"], pin["localization"])
    assert [r.hex() for r in roots] == pin["index_roots"]
    assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["bytes"], pin["sha256"])


# -- 6. what stays refused --
def check_refusals(lib, torch, device):
    import libiop_amd as la
    from libiop_amd import domains
    for W in WORDS:
        f = NAME[W]
        _, _, inst = model(W, NATIVE_TUPLES[0])
        comm = lib.comm_create_replay(0, 1)
        try:
            with native_instance(lib, W, inst) as h:
                with C.options(lib, **{WIDE_OPTION: 1}):
                    with pytest.raises(ValueError, match="%s has no distributed prover: pass no communicator" % f):
                        lib.fractal_index_dist(h, comm)
                    with pytest.raises(ValueError, match="%s has no distributed prover: pass no communicator" % f):
                        lib.fractal_prove_dist(h, comm)
                    for hh in (la.HASH_POSEIDON_STARKWARE, la.HASH_POSEIDON_HIGH_ALPHA):
                        with pytest.raises(ValueError, match="%s proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only" % f):
                            lib.aurora_prove(h, hash=hh)
                    with pytest.raises(ValueError, match="security_parameter 100 is not supported"):
                        lib.fractal_index(h, 100)
                    with pytest.raises(ValueError, match="codeword domain dimension 41: the %s transforms take domains of dimension up to 40" % f):
                        lib.fractal_index(h, 128, 33, 2)
                    with pytest.raises(AssertionError, match="no index for these parameters"):
                        lib.fractal_prove(h)
                # the new option unset: today's words, whatever IOPX_GFX_FRACTAL holds
                for value in (0, 1):
                    with C.options(lib, **{F.OPTION: value}):
                        with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over " + f):
                            lib.fractal_index(h)
                        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over " + f):
                            lib.fractal_prove(h)
                        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over " + f):
                            lib.aurora_instance_warm(h, fractal=True)
        finally:
            lib.comm_destroy(comm)
        # the Aurora operator sets and the plain construction refuse what they refused
        aurora_ops = C.aurora_ops(lib, torch, device, W)
        for name in FRACTAL_OPERATORS:
            with pytest.raises(NotImplementedError, match=r"%s: DeviceOps\.%s has no GF\(2\^%d\) entry" % (f, name, 64 * W)):
                getattr(aurora_ops, name)()
        plain = domains.DeviceOps(lib, torch, device, C.domain_field(W))
        with pytest.raises(NotImplementedError, match=r"%s: DeviceOps\.div has no GF\(2\^%d\) entry" % (f, 64 * W)):
            plain.div()
    # gf64 is governed by IOPX_GFX_FRACTAL alone
    g = lib.aurora_example_instance(la.FIELD_GF64, 64, 3, 63, SEED)
    try:
        with C.options(lib, **{WIDE_OPTION: 1}):
            with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over gf64"):
                lib.fractal_index(g)
            with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over gf64"):
                lib.fractal_prove(g)
    finally:
        lib.aurora_instance_free(g)


# -- 8. other fields unchanged --
def check_other_fields_unchanged(lib, torch, device):
    """gf64 (its own option), gf192 and edwards Fr Fractal transcripts after wide-field proofs in this process"""
    import fractal_cases
    for W in WORDS:
        check_native_prover(lib, W, NATIVE_TUPLES[0])
    F.check_native_prover(lib, F.NATIVE_TUPLES[0])
    fractal_cases.check_transcript_equals_oracle(lib, torch, device, "gf192", 6, 3, SEED)
    fractal_cases.check_transcript_equals_oracle(lib, torch, device, "edwards_Fr", 6, 3, SEED)
