"""The FRI-only SNARK over alt_bn128 Fr (BLAKE2b and both Poseidon families) on the CPU build of the kernels.

There is no oracle prover over this field; the native prover is compared with a Python-integer model (tests/bn128_fri_snark_model.py).  The
model is validated where the oracle can judge it (edwards_Fr + BLAKE2b against oracle.fri_snark_prove; its sponge against
oracle.poseidon_leafhash), then used where it cannot."""
import numpy as np
import pytest
import torch

import bn128_fri_snark_cases as C
import bn128_fri_snark_model as M
import fri_cases
import oracle
from emu_lib import emu

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


# ---- 1. the model is right where the oracle can say so -------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", C.TUPLES)
def test_model_equals_oracle_prover_over_edwards(tup):
    assert M.prove(M.EDWARDS_FR, M.BLAKE2B, *tup, seed=C.SEED) == oracle.fri_snark_prove(oracle.FIELD_EDWARDS, *tup, C.SEED)


@pytest.mark.parametrize("hash_type", [M.POSEIDON_STARKWARE, M.POSEIDON_HIGH_ALPHA])
def test_model_sponge_equals_oracle_leafhash(hash_type):
    """absorb, then squeeze one element, is algebraic_leafhash::hash: leaves of 1 .. 9 elements cross the rate (2) several times"""
    from poseidon_cases import SETS
    names = [M.POSEIDON_SETS[hash_type]] + (["high_alpha17_t4"] if hash_type == M.POSEIDON_HIGH_ALPHA else [])      # state sizes 3 and 4
    for name in names:
        params = oracle.PoseidonParams(SETS[name])
        for count in range(1, 10):
            leaf = C.seeded(40 + count, count)
            sponge = M.Sponge(params)
            sponge.absorb(leaf)
            got = sponge.squeeze(1)[0]
            assert got == oracle.bn_to_ints(oracle.poseidon_leafhash(params, oracle.bn_from_ints(leaf)))[0], (name, count)


def test_host_permutation_equals_oracle():
    """the hashchain's host permutation (iopx_poseidon_permute_bn128_host) over the shipped tables, all three sets"""
    import libiop_amd
    from poseidon_cases import SETS
    for name in ("starkware_alpha5_t3", "high_alpha17_t3", "high_alpha17_t4"):
        p, po = libiop_amd.PoseidonParams.from_dict(SETS[name]), oracle.PoseidonParams(SETS[name])
        for seed in range(3):
            st = oracle.bn_from_ints(C.seeded(70 + seed, p.state_size))
            assert np.array_equal(emu().poseidon_permute_host(p, st), oracle.poseidon_permute(po, st)), name


# ---- 2. the feature: the native prover over alt_bn128 Fr --------------------------------------------------------------------------
@pytest.mark.parametrize("hash_name", list(C.HASHES))
@pytest.mark.parametrize("tup", C.TUPLES)
def test_native_prover_equals_fixture(fixture, tup, hash_name):
    C.check_transcript(emu(), fixture, tup, hash_name)


@pytest.mark.parametrize("hash_name", list(C.HASHES))
def test_fixture_equals_model(fixture, hash_name):
    """the committed fixture is what the model says today (the dim-8 tuple; the generator writes all of it from the same function)"""
    tup = C.TUPLES[0]
    want = M.prove(M.ALT_BN128_FR, C.HASHES[hash_name], *tup, coeffs=C.seeded(C.SEED, 1 << (tup[0] - tup[1])))
    assert bytes.fromhex(fixture["transcripts"][C.key(tup, hash_name)]) == want


def test_plain_entry_means_blake2b(fixture):
    tup = C.TUPLES[0]
    assert C.native_prove(emu(), tup, "blake2b", through_plain_entry=True) == bytes.fromhex(fixture["transcripts"][C.key(tup, "blake2b")])


def test_absorbing_hashchain_reads_every_root_at_its_round_end():
    """absorbs_input = true switches deferred roots (and the side-stream trees) off: one immediate read-back per tree; none over BLAKE2b"""
    lib, tup = emu(), C.TUPLES[0]
    lib.cold_stats(reset=True)
    C.native_prove(lib, tup, "blake2b")
    assert C.roots_read_at_round_end(lib) == 0
    C.native_prove(lib, tup, "poseidon_starkware")
    assert C.roots_read_at_round_end(lib) == len(M.localization_array(tup[2], tup[0], tup[1]))
    lib.cold_stats(reset=True)


# ---- 3. fewer coefficients than the bound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_name", ["blake2b", "poseidon_starkware"])
@pytest.mark.parametrize("which", ["one", "bound_minus_one"])
def test_fewer_coefficients(fixture, which, hash_name):
    tup = C.SHORT_TUPLE
    n = 1 if which == "one" else (1 << (tup[0] - tup[1])) - 1
    C.check_transcript(emu(), fixture, tup, hash_name, n)
    if hash_name == "blake2b":
        assert bytes.fromhex(fixture["transcripts"][C.key(tup, hash_name, n)]) == M.prove(M.ALT_BN128_FR, M.BLAKE2B, *tup, coeffs=C.seeded(C.SEED, n))


# ---- 4. the 4-word BLAKE2b squeeze at a rejection ----------------------------------------------------------------------------------
def test_blake2b_squeeze_retries_over_four_words(fixture):
    """C.RETRY_TUPLE: the model's hashchain rejects a draw and retries (see the comment there); the native chain must take the same keys"""
    tup, stats = C.RETRY_TUPLE, {}
    want = M.prove(M.ALT_BN128_FR, M.BLAKE2B, *tup, coeffs=C.seeded(C.SEED, 1 << (tup[0] - tup[1])), stats=stats)
    assert stats["squeeze_retries"] >= 1
    assert C.native_prove(emu(), tup, "blake2b") == want


# ---- 5. the fields that were there before ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_name,dim,rs_extra,loc_param,interactions,queries", [
    ("gf192", 8, 2, 2, 1, 6), ("gf192", 7, 2, 1, 2, 4), ("edwards_Fr", 8, 2, 2, 1, 6), ("edwards_Fr", 10, 2, 3, 2, 10), ("edwards_Fr", 11, 2, 3, 1, 10)])
def test_existing_fields_unchanged(field_name, dim, rs_extra, loc_param, interactions, queries):
    assert fri_cases.native_prove_equals_oracle(emu(), torch, CPU, field_name, dim, rs_extra, loc_param, interactions, queries, C.SEED)


# ---- 6. argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    lib = emu()
    d = lib.malloc(64 * 32)
    try:
        lib.h2d(d, np.zeros((64, 4), dtype=np.uint64))
        for field in (0, 1):
            for h in (2, 3):
                with pytest.raises(ValueError):
                    lib.fri_snark_prove(field, d, 64, 8, 2, 2, 1, 3, hash=h)           # Poseidon is wired for alt_bn128 Fr only
        with pytest.raises(ValueError):
            lib.fri_snark_prove(2, d, 64, 29, 23, 2, 1, 3, hash=1)                      # no subgroup of order 2^29
        with pytest.raises(ValueError):
            lib.fri_snark_prove(2, d, 64, 29, 23, 2, 1, 3)
        for h in (0, 4, 7):
            with pytest.raises(ValueError):
                lib.fri_snark_prove(2, d, 64, 8, 2, 2, 1, 3, hash=h)                    # unknown hash
        comm = lib.comm_create_replay(0, 1)
        try:
            with pytest.raises(ValueError, match="distributed"):
                lib.fri_snark_prove(2, d, 64, 8, 2, 2, 1, 3, comm=comm)                 # no distributed prover over this field
        finally:
            lib.comm_destroy(comm)
        with pytest.raises(ValueError):
            lib.fri_snark_prove(2, d, 65, 8, 2, 2, 1, 3, hash=2)                        # more coefficients than the bound
        assert len(lib.fri_snark_prove(2, d, 0, 8, 2, 2, 1, 3, hash=2)) > 0             # the zero polynomial
    finally:
        lib.free(d)


# ---- 7. the fixed-shape leaf kernel for 32-byte elements ------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [2, 4, 8])
@pytest.mark.parametrize("num_oracles", [1, 2, 3, 4])
def test_leaf_kernel_sub32_equals_general(num_oracles, cs):
    for log_n in (6, 9):
        C.check_sub32_equals_general(emu(), log_n, num_oracles, cs, against_hashlib=(log_n == 6))


def test_leaf_kernel_selection():
    """inside the specialisation the fixed-shape kernel runs (and the option switches it off); outside it the general kernel does, with hashlib's roots"""
    lib, n = emu(), 1 << 6
    one = [C.rand_words(1, n)]
    assert C.sub32_launches(lib, lambda: C.leaf_nodes(lib, one, 4)) == (1, 0)
    assert C.sub32_launches(lib, lambda: C.leaf_nodes(lib, one, 4, sub32=False)) == (0, 1)
    salts = np.random.default_rng(3).integers(0, 256, size=(n // 4, 32), dtype=np.uint8)
    outside = [("five oracles", [C.rand_words(10 + k, n) for k in range(5)], 4, 1, None), ("cosets of 16", one, 16, 1, None),
               ("salted", one, 4, 1, salts), ("additive", one, 4, 0, None), ("24-byte elements", [C.rand_words(2, n, 3)], 8, 1, None)]
    for label, oracles, cs, domain_type, s in outside:
        got = []
        assert C.sub32_launches(lib, lambda: got.append(C.leaf_nodes(lib, oracles, cs, domain_type, s)))[0] == 0, label
        assert np.array_equal(got[0][0], C.hashlib_nodes(oracles, cs, domain_type, s)[0]), label
