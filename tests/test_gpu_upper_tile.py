"""The comb upper butterfly pass on the GPU: the shapes of tests/upper_tile_cases.py (every dimension there has comb upper passes, see that
module's table of the schedule), byte for byte against the oracle; at d = 17 against the oracle's pinned digests, which
tests/test_upper_tile_emu.py::test_pins_are_the_oracles keeps equal to the oracle's outputs.  Here a tile is eight wavefronts running at once:
a barrier missing where the rows change hands, or a row owned by two wavefronts, is a race over 2048 elements per tile."""
import pytest

import upper_tile_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import libiop_amd
    lib = libiop_amd.lib()          # raises if the HIP library is missing: no fallback
    lib.init(0)
    return lib


@pytest.mark.parametrize("d,kind", [(d, "standard") for d in uc.DIMS] + [(12, "random")])
def test_forward_and_inverse(gpu, d, kind):
    uc.check_fft_ifft(gpu, d, kind, pinned=(d == 17))


@pytest.mark.parametrize("cb,cc", uc.LDE_COSETS)
@pytest.mark.parametrize("d,kind", [(11, "standard"), (12, "standard"), (17, "standard"), (12, "random"), (14, "random")])
def test_coset_lde(gpu, d, kind, cb, cc):
    uc.check_lde(gpu, True, d, kind, cb, cc, pinned=(d == 17))


def test_reextension_batch(gpu):
    uc.check_reextend(gpu, True)
