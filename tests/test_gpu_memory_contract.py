"""The memory contract (tests/memory_contract_cases.py) on a real MI355X: every device entry inside 4096-byte frames under the library's
memory-check mode (guards around every block the library allocates, poisoned payloads, two poison bytes), at the shapes where the launch
geometry changes, and the provers under the same mode with a warm second proof.  The checker's own self-check writes outside a payload on
purpose (inside its block's guards) and therefore runs on the CPU build only: tests/test_memory_contract_emu.py."""
import pytest

import memory_contract_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()          # raises if the HIP library is missing: no fallback
    lib.init(0)
    return lib


@pytest.mark.parametrize("group", sorted(mc.GROUPS))
def test_direct_entries(gpu, group):
    mc.run_group(gpu, group)


@pytest.mark.parametrize("tag", ["fp3", "bn128"])
def test_three_pass_transform(gpu, tag):
    mc.check_three_pass_fft(gpu, tag)


@pytest.mark.parametrize("case", sorted(mc.PROVER_CASES))
def test_provers(gpu, case):
    mc.check_prover(gpu, case, on_gpu=True)


def test_option_off_allocates_as_before(gpu):
    mc.check_mode_off_and_mixing(gpu, align=256)
