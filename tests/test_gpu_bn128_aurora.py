"""Aurora over alt_bn128 Fr on the MI355X: the windowed last pass of the forward transform at the one-, two- and three-pass sizes, the native
prover against the committed digests of the Python-integer model (tests/golden/bn128_aurora.json), and the absorbing hashchain's root read-backs."""
import pytest

import bn128_aurora_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    l = libiop_amd.lib()
    l.init(0)
    return l


@pytest.fixture(scope="module")
def fixture():
    return C.load_fixture()


def test_pass_sizes_of_the_plan(lib):
    assert C.pass_sizes(lib) == {1: 1, 2: 12, 3: 19, 4: 26}


@pytest.mark.parametrize("log_n", [4, 11, 12, 19])
def test_windows_equal_the_gather_of_the_output(lib, log_n):
    sizes = C.pass_sizes(lib)
    assert lib.multiplicative_FFT_pass_count(log_n, 1 << log_n) == {4: 1, 11: 1, sizes[2]: 2, sizes[3]: 3}[log_n]
    for n_coeffs, windows, alias in C.window_cases(log_n):
        C.check_windows(lib, log_n, n_coeffs, windows, against_integers=(log_n == 4), alias=alias)


@pytest.mark.parametrize("hash_name", list(C.HASHES))
def test_native_prover_equals_fixture_small(lib, fixture, hash_name):
    tup = C.TUPLES[1]
    first = C.check_digest(lib, fixture, tup, hash_name)
    for head_eval, windows in ((1, 0), (0, 1), (0, 0)):
        assert C.native_prove(lib, tup, hash_name, head_eval=head_eval, windows=windows) == first, (head_eval, windows)


@pytest.mark.parametrize("hash_name", C.GPU_HASHES)
def test_native_prover_equals_fixture_two_pass_codewords(lib, fixture, hash_name):
    first = C.check_digest(lib, fixture, C.GPU_TUPLE, hash_name)
    assert C.native_prove(lib, C.GPU_TUPLE, hash_name, windows=0) == first
    assert C.native_prove(lib, C.GPU_TUPLE, hash_name, head_eval=0) == first


def test_windowed_pass_runs_in_the_prover(lib):
    for windows in (1, 0):
        lib.profile_begin()
        C.native_prove(lib, C.GPU_TUPLE, "blake2b", windows=windows)
        rows = lib.profile_report()
        assert rows.get("k_bn_mfft_pass", (0,))[0] > 0
        assert (rows.get("k_bn_mfft_pass_win", (0,))[0] > 0) == bool(windows)


def test_root_read_backs(lib):
    tup = C.TUPLES[1]
    lib.cold_stats(reset=True)
    C.native_prove(lib, tup, "blake2b")
    assert C.roots_read_at_round_end(lib) == 0
    lib.cold_stats(reset=True)
    C.native_prove(lib, tup, "poseidon_starkware")
    assert C.roots_read_at_round_end(lib) == C.num_trees(tup) == 4
