"""The prime-field kernels at their limb and range bounds on the MI355X: the cases of tests/limb_bound_cases.py (inputs chosen in the stored
form, expected values from Python integers, exact equality of canonical words) against the HIP library.  The CPU-build leg is
tests/test_limb_bounds_emu.py."""
import pytest

import limb_bound_cases as C

pytestmark = pytest.mark.gpu

FIELD_NAMES = sorted(C.FIELDS)


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_every_ordered_pair_of_patterns_in_one_butterfly(lib, field):
    C.check_all_pairs(lib, C.FIELDS[field])


@pytest.mark.parametrize("log_n", range(1, 12))
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_single_pass_transforms(lib, field, log_n):
    C.check_transforms(lib, C.FIELDS[field], log_n)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_targeted_butterflies(lib, field):
    C.check_targeted_transforms(lib, C.FIELDS[field])


@pytest.mark.parametrize("log_n", [12, 13, C.PAIR_SWEEP_LOG, 19])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_multi_pass_transforms(lib, field, log_n):
    C.check_large_transforms(lib, C.FIELDS[field], log_n)


@pytest.mark.parametrize("log_n", [1, 3, 4, 6, 8])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_folds(lib, field, log_n):
    C.check_folds(lib, C.FIELDS[field], log_n)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_folds_of_every_ordered_pair_and_targeted_products(lib, field):
    C.check_fold_pair_sweep_and_targets(lib, C.FIELDS[field])


@pytest.mark.parametrize("log_n", [5, 8])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_ldt_combination(lib, field, log_n):
    C.check_ldt(lib, C.FIELDS[field], log_n)


def test_edwards_sums_of_products_with_stored_extremes(lib):
    C.check_lincomb(lib)


def test_edwards_elementwise_on_every_ordered_pair(lib):
    C.check_elementwise(lib)


def test_edwards_virtual_oracles_on_stored_patterns(lib):
    C.check_virtual_oracles(lib)


def test_edwards_sparse_products_and_division_on_stored_patterns(lib):
    C.check_sparse_and_division(lib)


def test_edwards_rationals_on_stored_patterns(lib):
    C.check_rationals(lib)


def test_bn128_to_montgomery_at_and_above_r(lib):
    C.check_to_montgomery(lib)


@pytest.mark.parametrize("name", ["test_params", "starkware_alpha5_t3", "high_alpha17_t3", "high_alpha17_t4"])
def test_bn128_poseidon_on_stored_extremes(lib, name):
    C.check_poseidon(lib, name)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_raw_words_up_to_the_documented_limit(lib, field):
    import noncanonical_cases
    noncanonical_cases.check_raw_limit(lib, field)
