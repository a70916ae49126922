"""The FRI-only SNARK over alt_bn128 Fr on the MI355X, through the HIP library, against the committed fixture (tests/golden/bn128_fri_snark.json,
written from the Python-integer model); the fixed-shape BLAKE2b leaf kernel for 32-byte elements against the general kernel on the device; and
the first hashchain with absorbs_input = true on the GPU: no root is deferred."""
import pytest

import bn128_fri_snark_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lb = libiop_amd.lib()
    lb.init(0)
    return lb


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


@pytest.mark.parametrize("hash_name", list(C.HASHES))
@pytest.mark.parametrize("tup", C.TUPLES)
def test_transcripts(lib, fixture, tup, hash_name):
    C.check_transcript(lib, fixture, tup, hash_name)


@pytest.mark.parametrize("hash_name", ["blake2b", "poseidon_starkware"])
@pytest.mark.parametrize("which", ["one", "bound_minus_one"])
def test_fewer_coefficients(lib, fixture, which, hash_name):
    tup = C.SHORT_TUPLE
    C.check_transcript(lib, fixture, tup, hash_name, 1 if which == "one" else (1 << (tup[0] - tup[1])) - 1)


@pytest.mark.parametrize("hash_name", list(C.HASHES))
def test_dim16_digest(lib, fixture, hash_name):
    """dim 16: the coset FFT takes several passes and the leaf grid more than one workgroup"""
    C.check_digest(lib, fixture, C.LARGE_TUPLE, hash_name)


def test_absorbing_hashchain_defers_no_root(lib, fixture):
    """the Poseidon chain absorbs every root: each of the tuple's trees is read back at its round end, with the default schedule options
    (IOPX_DEFER_ROOTS, IOPX_MERKLE_STREAM) in force; the BLAKE2b chain over the same field reads none there"""
    tup = C.LARGE_TUPLE
    trees = 1 + (tup[0] - tup[1] - 1) // tup[2]
    lib.cold_stats(reset=True)
    C.native_prove(lib, tup, "blake2b")
    assert C.roots_read_at_round_end(lib) == 0
    C.check_digest(lib, fixture, tup, "poseidon_starkware")
    assert C.roots_read_at_round_end(lib) == trees
    lib.cold_stats(reset=True)


@pytest.mark.parametrize("cs", [2, 4, 8])
@pytest.mark.parametrize("num_oracles", [1, 2, 3, 4])
def test_leaf_kernel_sub32_equals_general(lib, num_oracles, cs):
    C.check_sub32_equals_general(lib, 9, num_oracles, cs, against_hashlib=True)
    C.check_sub32_equals_general(lib, 14, num_oracles, cs)


def test_leaf_kernel_selection(lib):
    one = [C.rand_words(1, 1 << 9)]
    assert C.sub32_launches(lib, lambda: C.leaf_nodes(lib, one, 4)) == (1, 0)
    assert C.sub32_launches(lib, lambda: C.leaf_nodes(lib, one, 4, sub32=False)) == (0, 1)
    assert C.sub32_launches(lib, lambda: C.leaf_nodes(lib, one, 16)) == (0, 1)
