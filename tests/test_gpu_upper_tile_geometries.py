"""The comb upper butterfly pass (k_bfly_upper_comb) on the MI355X at the tile geometries the defaults never reach, byte for byte against the
oracle: three level pairs in a 96 KiB tile with two wave tasks per wavefront, column chunks (256 columns), two column widths in one transform,
one wavefront per workgroup, workgroups of 256 threads.  tests/upper_tile_cases.py (GEOMETRIES, check_geometry) holds the options of each row,
its dimensions, the tiles they give and the cases; the CPU leg, under hostile thread orders too, is
tests/test_kernel_schedules_emu.py::test_upper_tile_geometries.

The geometry is read once per process, so each row runs in a CHILD process with its options in the environment; the child fails, not skips,
when the library does not see them (upper_tile_cases.assert_comb_schedule)."""
import os
import subprocess
import sys

import pytest

import upper_tile_cases as uc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os
import libiop_amd
import upper_tile_cases as uc
lib = libiop_amd.lib()
lib.init(0)
uc.check_geometry(lib, True, os.environ["IOPX_UPPER_GEOMETRY"])
print("ok")
"""


def _run(script, extra_env, timeout=300):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **extra_env)
    out = subprocess.run([sys.executable, "-c", script], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (extra_env, out.stdout[-2000:], out.stderr[-4000:])


@pytest.mark.parametrize("name", sorted(uc.GEOMETRIES))
def test_geometry_equals_the_oracle(name):
    _run(CHILD, dict(uc.geometry_env(name), IOPX_P1_COLS="3"))
