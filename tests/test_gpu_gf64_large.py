"""The GF(2^64) arm past its launch caps on the MI355X (tests/gf64_large_cases.py): every protocol-layer entry (libiop_amd/csrc/gfx_ops.h over gf64) at the smallest
size where its grid-stride loop takes a second trip (2^23 + 3 elements, 2^22 + 3 rows, m = 24), whole-vector against a host-side reference
that tests/test_gf64_large_emu.py holds to the oracle at m = 12; and the LDE of libiop_amd/csrc/gf64.hip over two staging groups (2^13
coefficients, 4101 cosets of an m = 26 domain).  The wall time of each test is the host-side reference's: the kernels take milliseconds."""
import pytest

import gf64_large_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    return lib


def test_add(lib):
    L.check_add(lib)


def test_lincomb_and_affine(lib):
    L.check_lincomb(lib)


def test_lincheck(lib):
    L.check_lincheck(lib)


def test_pow_table(lib):
    L.check_pow_table(lib)


def test_spmv(lib):
    L.check_spmv(lib)


def test_poly_div_vanishing(lib):
    L.check_poly_div_vanishing(lib)


def test_rowcheck(lib):
    L.check_rowcheck(lib)


def test_fz(lib):
    L.check_fz(lib)


@pytest.mark.parametrize("arm", L.SUMCHECK_ARMS)
def test_sumcheck_g(lib, arm):
    L.check_sumcheck_g(lib, arm)


def test_lde_over_two_staging_groups(lib):
    L.check_lde_groups(lib)
