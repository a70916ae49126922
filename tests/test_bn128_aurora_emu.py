"""Aurora over alt_bn128 Fr (BLAKE2b and both Poseidon families) on the CPU build of the kernels.

There is no oracle prover over this field; the native prover is compared with a Python-integer model (tests/bn128_aurora_model.py).  The model is
validated where the oracle can judge it (edwards_Fr + BLAKE2b against oracle.aurora_prove, its instance against oracle.r1cs_example), then used
where it cannot."""
import numpy as np
import pytest
import torch

import aurora_cases
import bn128_aurora_cases as C
import bn128_aurora_model as M
import oracle
from emu_lib import emu

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


# ---- 1. the model is right where the oracle can say so -------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", C.TUPLES)
def test_model_equals_oracle_prover_over_edwards(tup):
    log_n, inputs, rs_extra, loc = tup
    mine = M.prove_example(M.EDWARDS_FR, M.BLAKE2B, *tup, C.SEED)
    assert mine == oracle.aurora_prove(oracle.FIELD_EDWARDS, log_n, inputs, C.SEED, rs_extra=rs_extra, localization=loc)
    assert oracle.aurora_verify(oracle.FIELD_EDWARDS, log_n, inputs, C.SEED, mine, rs_extra=rs_extra, localization=loc)


@pytest.mark.parametrize("tup", C.TUPLES)
def test_model_instance_equals_oracle_example(tup):
    log_n, inputs = tup[:2]
    F = M.EDWARDS_FR
    ex = M.example(F, log_n, inputs, C.SEED)
    z, idx, coeff = oracle.r1cs_example(oracle.FIELD_EDWARDS, log_n, inputs, C.SEED)
    assert [F.from_mont_bytes(w.tobytes()) for w in z] == ex["z"]
    assert [int(v) for v in idx] == [row[0][0] for row in ex["C"]]
    assert [F.from_mont_bytes(w.tobytes()) for w in coeff] == [row[0][1] for row in ex["C"]]


# ---- 2. the feature: the native prover over alt_bn128 Fr, four schedules, one transcript ------------------------------------------------
@pytest.mark.parametrize("hash_name", list(C.HASHES))
@pytest.mark.parametrize("tup", C.TUPLES)
def test_native_prover_equals_model(fixture, tup, hash_name):
    want = M.prove_example(M.ALT_BN128_FR, C.HASHES[hash_name], *tup, C.SEED)
    assert C.digest(want) == fixture["digests"][C.key(tup, hash_name)], "the committed fixture is not what the model says today"
    for head_eval in (1, 0):
        for windows in (1, 0):
            got = C.native_prove(emu(), tup, hash_name, head_eval=head_eval, windows=windows)
            assert got == want, (head_eval, windows, "first difference at byte %d" % next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))


def test_plain_entry_means_blake2b(fixture):
    tup = C.TUPLES[0]
    assert C.digest(C.native_prove(emu(), tup, "blake2b", through_plain_entry=True)) == fixture["digests"][C.key(tup, "blake2b")]


def test_windows_leave_the_last_pass_only_when_switched_on():
    """with head evaluation the prover's transforms hand their windows out of k_bn_mfft_pass<true>; IOPX_BN128_FFT_WINDOWS=0 takes the plain transform"""
    lib, tup = emu(), C.TUPLES[2]
    for windows in (1, 0):
        lib.profile_begin()
        C.native_prove(lib, tup, "blake2b", windows=windows)
        rows = lib.profile_report()
        assert rows.get("k_bn_mfft_pass", (0,))[0] > 0
        assert (rows.get("k_bn_mfft_pass_win", (0,))[0] > 0) == bool(windows), rows.get("k_bn_mfft_pass_win")


def test_warm_then_prove(fixture):
    lib, tup = emu(), C.TUPLES[0]
    inst = lib.aurora_example_instance(C.FIELD_ALT_BN128_FR, 1 << tup[0], tup[1], (1 << tup[0]) - 1, C.SEED)
    try:
        lib.aurora_instance_warm(inst, False, 128, tup[2], tup[3])
        assert C.digest(lib.aurora_prove(inst, 128, tup[2], tup[3])) == fixture["digests"][C.key(tup, "blake2b")]
    finally:
        lib.aurora_instance_free(inst)


# ---- 3. the caller's own system, four-word coefficients; an unsatisfied witness takes the fallback schedule ----------------------------
def _csr(ex):
    mats = []
    for name in ("A", "B", "C"):
        rows = ex[name]
        row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        col = np.array([j for r in rows for j, _ in r], dtype=np.uint32)
        mats.append((row_ptr, col, C.mont_words([c for r in rows for _, c in r])))
    return mats


@pytest.mark.parametrize("hash_name", ["blake2b", "poseidon_high_alpha"])
def test_callers_own_system_and_unsatisfied_witness(fixture, hash_name):
    lib, tup = emu(), C.TUPLES[1]
    log_n, inputs, rs_extra, loc = tup
    ex = M.example(M.ALT_BN128_FR, log_n, inputs, C.SEED)
    inst = lib.aurora_instance(C.FIELD_ALT_BN128_FR, _csr(ex), ex["num_variables"], inputs, C.mont_words(ex["z"]))
    try:
        assert C.digest(lib.aurora_prove(inst, 128, rs_extra, loc, hash=C.HASHES[hash_name])) == fixture["digests"][C.key(tup, hash_name)]
    finally:
        lib.aurora_instance_free(inst)
    bad = dict(ex, z=list(ex["z"]))
    bad["z"][inputs + 11] = (bad["z"][inputs + 11] + 1) % C.BN128_R           # one auxiliary element changed
    want = M.prove(M.ALT_BN128_FR, C.HASHES[hash_name], bad, rs_extra, loc)
    inst = lib.aurora_instance(C.FIELD_ALT_BN128_FR, _csr(ex), ex["num_variables"], inputs, C.mont_words(bad["z"]))
    try:
        for head_eval in (1, 0):
            with C.options(lib, IOPX_HEAD_EVAL=head_eval):
                assert lib.aurora_prove(inst, 128, rs_extra, loc, hash=C.HASHES[hash_name]) == want, head_eval
    finally:
        lib.aurora_instance_free(inst)


# ---- 4. the absorbing hashchain reads every root at its round end ----------------------------------------------------------------------
def test_root_read_backs():
    lib, tup = emu(), C.TUPLES[2]
    stats = {}
    M.prove_example(M.ALT_BN128_FR, M.BLAKE2B, *tup, C.SEED, stats=stats)
    lib.cold_stats(reset=True)
    C.native_prove(lib, tup, "blake2b")
    assert C.roots_read_at_round_end(lib) == 0
    for h in ("poseidon_starkware", "poseidon_high_alpha"):
        lib.cold_stats(reset=True)
        C.native_prove(lib, tup, h)
        assert C.roots_read_at_round_end(lib) == stats["num_trees"] == C.num_trees(tup) == 4


# ---- 5. refusals, each by its message ---------------------------------------------------------------------------------------------------
def test_refusals():
    lib = emu()
    bn = lib.aurora_example_instance(C.FIELD_ALT_BN128_FR, 32, 3, 31, C.SEED)
    ed = lib.aurora_example_instance(1, 32, 3, 31, C.SEED)
    gf = lib.aurora_example_instance(0, 32, 3, 31, C.SEED)
    comm = lib.comm_create_replay(0, 1)
    try:
        for inst in (ed, gf):
            with pytest.raises(ValueError, match="Poseidon is wired for alt_bn128 Fr only"):
                lib.aurora_prove(inst, 128, 2, 1, hash=C.HASHES["poseidon_starkware"])
        for inst in (bn, ed):
            with pytest.raises(ValueError, match="bcs_hash_type unknown"):
                lib.aurora_prove(inst, 128, 2, 1, hash=7)
        with pytest.raises(ValueError, match="codeword domain dimension 29: alt_bn128 Fr has subgroups of order up to 2\\^28"):
            lib.aurora_prove(bn, 128, 24, 2)
        with pytest.raises(ValueError, match="alt_bn128 Fr has no distributed prover"):
            lib.aurora_prove_dist(bn, comm, 128, 2, 1)
        with pytest.raises(ValueError, match="iopx_fractal_index: there is no Fractal prover over alt_bn128 Fr"):
            lib.fractal_index(bn)
        with pytest.raises(ValueError, match="iopx_fractal_prove: there is no Fractal prover over alt_bn128 Fr"):
            lib.fractal_prove(bn)
        with pytest.raises(ValueError, match="security_parameter 100 is not supported"):
            lib.aurora_prove(bn, 100, 2, 1)
        with pytest.raises(ValueError, match="unknown field"):
            lib.aurora_example_instance(3, 32, 3, 31, C.SEED)
    finally:
        lib.comm_destroy(comm)
        for inst in (bn, ed, gf):
            lib.aurora_instance_free(inst)


# ---- 6. the fields that were there keep their bytes through the templated path --------------------------------------------------------
@pytest.mark.parametrize("field_name, code, tup", [("gf192", 0, (6, 3, 3, 2)), ("edwards_Fr", 1, (7, 7, 2, 3))])
def test_existing_fields_unchanged(field_name, code, tup):
    lib = emu()
    log_n, inputs, rs_extra, loc = tup
    transcript, _ = aurora_cases.check_transcript_equals_oracle(lib, torch, CPU, field_name, log_n, inputs, C.SEED, rs_extra=rs_extra, localization=loc)
    inst = lib.aurora_example_instance(code, 1 << log_n, inputs, (1 << log_n) - 1, C.SEED)
    try:
        assert lib.aurora_prove(inst, 128, rs_extra, loc) == lib.aurora_prove(inst, 128, rs_extra, loc, hash=C.HASHES["blake2b"]) == transcript.serialize()
    finally:
        lib.aurora_instance_free(inst)


# ---- 7. the windowed transform, directly ---------------------------------------------------------------------------------------------
def test_pass_sizes_of_the_plan():
    """one pass up to a 2^11 tile, then strided passes of up to 7 bits each (MF_TILE_BITS, MF_COLS in fft_mul.hip); the four-pass sizes (2 GB
    of output and more) are left to the prover's own limits"""
    assert C.pass_sizes(emu()) == {1: 1, 2: 12, 3: 19, 4: 26}


@pytest.mark.parametrize("log_n", [4, 11, 12, 19])          # the smallest with log_stride 1 != log_n - 2; the last one-pass size; two passes; three passes
def test_windows_equal_the_gather_of_the_output(log_n):
    lib = emu()
    sizes = C.pass_sizes(lib)
    assert lib.multiplicative_FFT_pass_count(log_n, 1 << log_n) == {4: 1, 11: 1, sizes[2]: 2, sizes[3]: 3}[log_n]
    cases = C.window_cases(log_n) if log_n < sizes[3] else C.window_cases(log_n)[1:3]       # 2^19 points on the CPU: the two-window cases only
    for n_coeffs, windows, alias in cases:
        C.check_windows(lib, log_n, n_coeffs, windows, against_integers=(log_n == 4), alias=alias)


def test_window_entry_with_the_unshifted_domain():
    C.check_windows(emu(), 6, 64, [(1, 1), (3, 4)], against_integers=True, shift=1)


def test_window_argument_refusals():
    lib = emu()
    d = lib.malloc(32 * 16)
    one = C.mont_words([1])[0]
    try:
        with pytest.raises(ValueError, match="at most two windows per transform"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 4, one, d, [(0, 1, d + 0)] * 3)
        with pytest.raises(ValueError, match="a window may not alias the output"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 4, one, d, [(0, 1, d)])
        with pytest.raises(ValueError, match="window 0: first 2, stride 2\\^1"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 4, one, d, [(2, 1, d + 256)])
        with pytest.raises(ValueError, match="window 0: first 0, stride 2\\^5"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 4, one, d, [(0, 5, d + 256)])
        with pytest.raises(ValueError, match="null window argument"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 4, one, d, [(0, 1, None)])
        with pytest.raises(ValueError, match="exceeds the 2-adicity"):
            lib.multiplicative_FFT_windows_bn128_dev(d, 0, 29, one, d, [], gen=one)
    finally:
        lib.free(d)
