"""FRI-only SNARK over alt_bn128 Fr: what the CPU-emulation and the GPU suites share.  The native prover (iopx_fri_snark_prove /
iopx_fri_snark_prove_hashed) against tests/golden/bn128_fri_snark.json, which tests/golden/make_bn128_fri_snark.py writes from the
Python-integer model (tests/bn128_fri_snark_model.py); and the fixed-shape BLAKE2b leaf kernel for 32-byte elements against the
general kernel.  Nothing here needs the oracle: the GPU suite reads committed fixtures only."""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bn128_fri_snark.json")

BN128_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FIELD_ALT_BN128_FR = 2
HASHES = {"blake2b": 1, "poseidon_starkware": 2, "poseidon_high_alpha": 3}
SEED = 5                                                    # as tests/test_fri_e2e_emu.py
TUPLES = [(8, 2, 2, 1, 3), (10, 3, 1, 2, 5), (11, 2, 3, 1, 10)]        # (dim, rs_extra, loc, interactions, queries)
SHORT_TUPLE = (8, 2, 2, 1, 3)                               # fewer coefficients than the bound: 1 and bound - 1
LARGE_TUPLE = (16, 2, 2, 1, 10)                             # multi-pass coset FFT, leaf grid beyond one workgroup: digests only
# The BLAKE2b hashchain ignores what it absorbs (reference quirk F8), so its challenges are a function of the round structure alone — of the
# tuple, not of the coefficient seed.  For this tuple the model's 4-word squeeze rejects a draw (at or above r after clearing the bits over
# the modulus' MSB) and retries with key += num_elements four times; (8, 2, 2, 1, 3) does so once.
RETRY_TUPLE = (10, 3, 1, 2, 5)


def key(tup, hash_name, n_coeffs=None):
    return "_".join(str(v) for v in tup) + "/" + hash_name + ("" if n_coeffs is None else "/n%d" % n_coeffs)


def seeded(seed, count):
    """tests/fri_cases.py's coefficients at four words: element i is SplitMix64 outputs 4 i .. 4 i + 3 as one integer, mod r"""
    mask = (1 << 64) - 1
    out = []
    for i in range(count):
        v = 0
        for w in range(4):
            z = (seed + (4 * i + w + 1) * 0x9E3779B97F4A7C15) & mask
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
            v |= (z ^ (z >> 31)) << (64 * w)
        out.append(v % BN128_R)
    return out


def mont_words(values):
    """canonical integers -> (count, 4) uint64 mont_repr"""
    return np.frombuffer(b"".join(((v << 256) % BN128_R).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def native_prove(lib, tup, hash_name, n_coeffs=None, through_plain_entry=False):
    dim, rs_extra, loc, interactions, queries = tup
    n = (1 << (dim - rs_extra)) if n_coeffs is None else n_coeffs
    arr = mont_words(seeded(SEED, n))
    d = lib.malloc(arr.nbytes)
    try:
        lib.h2d(d, arr)
        h = None if through_plain_entry else HASHES[hash_name]
        return lib.fri_snark_prove(FIELD_ALT_BN128_FR, d, n, dim, rs_extra, loc, interactions, queries, hash=h)
    finally:
        lib.free(d)


def first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def check_transcript(lib, fixture, tup, hash_name, n_coeffs=None):
    got = native_prove(lib, tup, hash_name, n_coeffs)
    want = bytes.fromhex(fixture["transcripts"][key(tup, hash_name, n_coeffs)])
    assert got == want, "native transcript differs from the model's at byte %d (lengths %d / %d)" % (first_difference(got, want), len(got), len(want))


def check_digest(lib, fixture, tup, hash_name):
    got = native_prove(lib, tup, hash_name)
    want = fixture["digests"][key(tup, hash_name)]
    assert len(got) == want["bytes"] and hashlib.blake2b(got, digest_size=32).hexdigest() == want["blake2b"]


def roots_read_at_round_end(lib):
    """how many roots the prover read back at their round end because the hashchain absorbs them (iopx_cold_stats counter)"""
    return lib.cold_stats().get("bcs_roots_read_at_round_end", (0, 0.0))[0]


# ---- the leaf kernels -------------------------------------------------------------------------------------------------------------
def rand_words(seed, n, words=4):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, words), dtype=np.uint64)


def leaf_nodes(lib, oracles, cs, domain_type=1, salts=None, sub32=True):
    """the node array of iopx_merkle_blake2b over host oracles; sub32=False switches the fixed-shape 32-byte kernel off"""
    if not sub32:
        lib.set_option("IOPX_LEAVES_SUB32", 0)
    try:
        return lib.merkle_tree(oracles, cs, domain_type, salts)
    finally:
        if not sub32:
            lib.clear_option("IOPX_LEAVES_SUB32")


def hashlib_nodes(oracles, cs, domain_type=1, salts=None):
    """merkle_tree.tcc:92-229 with hashlib: leaves oracle-major over positions i + j L (cosets) or i cs + j (subspaces)"""
    n = oracles[0].shape[0]
    L = n // cs
    b2 = lambda d: hashlib.blake2b(d, digest_size=32).digest()
    leaves = []
    for i in range(L):
        pos = [i + j * L for j in range(cs)] if domain_type == 1 else [i * cs + j for j in range(cs)]
        d = b2(b"".join(o[q].tobytes() for o in oracles for q in pos))
        if salts is not None:
            d = b2(d + salts[i].tobytes())
        leaves.append(d)
    nodes = [b""] * (L - 1) + leaves
    for k in range(L - 2, -1, -1):
        nodes[k] = b2(nodes[2 * k + 1] + nodes[2 * k + 2])
    return np.frombuffer(b"".join(nodes), dtype=np.uint8).reshape(2 * L - 1, 32)


def check_sub32_equals_general(lib, log_n, num_oracles, cs, against_hashlib=False):
    n = 1 << log_n
    oracles = [rand_words(1000 * num_oracles + 10 * cs + k, n) for k in range(num_oracles)]
    fixed = leaf_nodes(lib, oracles, cs)
    general = leaf_nodes(lib, oracles, cs, sub32=False)
    assert np.array_equal(fixed, general), (log_n, num_oracles, cs)
    if against_hashlib:
        assert np.array_equal(fixed, hashlib_nodes(oracles, cs)), (log_n, num_oracles, cs)


def sub32_launches(lib, fn):
    """launches of k_merkle_leaves_sub32 and of the general k_merkle_leaves while fn runs (the library's per-kernel profile)"""
    lib.profile_begin()
    fn()
    rows = lib.profile_report()
    return rows.get("k_merkle_leaves_sub32", (0,))[0], rows.get("k_merkle_leaves", (0,))[0]
