"""The prime-field kernels at their limb and range bounds, on the CPU build of the kernel sources (tests/emu): inputs chosen in the stored
form (tests/limb_bound_cases.py), expected values from Python integers, exact equality of canonical words.  The GPU leg is
tests/test_gpu_limb_bounds.py."""
import pytest

import limb_bound_cases as C
from emu_lib import emu

FIELD_NAMES = sorted(C.FIELDS)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_the_two_references_agree(field):
    C.check_references_agree(C.FIELDS[field])


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_patterns_are_what_they_say(field):
    """the stored limbs themselves: all-ones runs, alternating limbs, and for alt_bn128 the top of the canonical range"""
    F = C.FIELDS[field]
    pats = C.patterns(F)
    limbs = lambda v: [(v >> (29 * i)) & C.MASK29 for i in range(F.limbs)]
    for i in range(F.limbs - 1):
        v = pats["ones_%d" % i]
        assert limbs(v)[:i + 1] == [C.MASK29] * (i + 1) and v < F.P <= v + (1 << (29 * (i + 1)))
    assert limbs(pats["alt_0"])[0::2][:3] == [C.MASK29] * 3 and not any(limbs(pats["alt_0"])[1::2])
    assert limbs(pats["alt_1"])[1::2][:3] == [C.MASK29] * 3 and not any(limbs(pats["alt_1"])[0::2])
    if F is C.BN:
        assert sum(1 for v in pats.values() if v >= 1 << 253) >= 12 and pats["p-1"] == F.P - 1
    full = F.random_canonical("range", 4096)
    assert max(full) > F.P - (F.P >> 8) and all(v < F.P for v in full)
    if F is C.BN:
        assert sum(1 for v in full if v >= 1 << 253) > 1000          # more than a third of the field lies there


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_every_ordered_pair_of_patterns_in_one_butterfly(field):
    C.check_all_pairs(emu(), C.FIELDS[field])


@pytest.mark.parametrize("log_n", range(1, 12))
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_single_pass_transforms(field, log_n):
    C.check_transforms(emu(), C.FIELDS[field], log_n)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_targeted_butterflies(field):
    C.check_targeted_transforms(emu(), C.FIELDS[field])


@pytest.mark.parametrize("log_n", [12, 13, C.PAIR_SWEEP_LOG, 19])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_multi_pass_transforms(field, log_n):
    C.check_large_transforms(emu(), C.FIELDS[field], log_n)


@pytest.mark.parametrize("log_n", [1, 3, 4, 6, 8])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_folds(field, log_n):
    C.check_folds(emu(), C.FIELDS[field], log_n)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_folds_of_every_ordered_pair_and_targeted_products(field):
    C.check_fold_pair_sweep_and_targets(emu(), C.FIELDS[field])


@pytest.mark.parametrize("log_n", [5, 8])
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_ldt_combination(field, log_n):
    C.check_ldt(emu(), C.FIELDS[field], log_n)


def test_edwards_sums_of_products_with_stored_extremes():
    C.check_lincomb(emu())


def test_edwards_elementwise_on_every_ordered_pair():
    C.check_elementwise(emu())


def test_edwards_virtual_oracles_on_stored_patterns():
    C.check_virtual_oracles(emu())


def test_edwards_sparse_products_and_division_on_stored_patterns():
    C.check_sparse_and_division(emu())


def test_edwards_rationals_on_stored_patterns():
    C.check_rationals(emu())


def test_bn128_to_montgomery_at_and_above_r():
    C.check_to_montgomery(emu())


@pytest.mark.parametrize("name", ["test_params", "starkware_alpha5_t3", "high_alpha17_t3", "high_alpha17_t4"])
def test_bn128_poseidon_on_stored_extremes(name):
    C.check_poseidon(emu(), name)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_raw_words_up_to_the_documented_limit(field):
    """outside the contract (canonical words in): what is still promised for raw words, per field — tests/noncanonical_cases.py"""
    import noncanonical_cases
    noncanonical_cases.check_raw_limit(emu(), field)
