"""The C++ seam of Fractal over the subspace-only binary fields: tests/cpp/test_gfx_fractal.cpp compiled against libiop_amd/cpp/fractal.hpp with the
gf64, gf128 and gf256 types of cpp/fields.hpp, run on the CPU build of the kernels and (-m gpu) against the HIP library.  The program holds the five
device operators over all three types to the host's products itself; it proves gf64_aurora_cases.hand_built_system() with
fractal_snark_prover<gf64> under IOPX_GFX_FRACTAL=1, and its index roots and bytes must equal the C ABI's on the same library and the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import gf64_aurora_cases as C
import gfx_fractal_cases as F
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, lib, lib_dir, lib_file):
    import libiop_amd
    matrices, z, num_inputs, rs_extra, loc = C.hand_built_system()
    n, num_variables = len(matrices[0][0]) - 1, z.shape[0]
    words = [np.array([n, num_variables, num_inputs, rs_extra, loc], dtype=np.uint64)]
    for row_ptr, col, coeff in matrices:
        words += [row_ptr.astype(np.uint64), col.astype(np.uint64), coeff.reshape(-1)]
    np.concatenate(words + [z.reshape(-1)]).astype(np.uint64).tofile(str(tmp_path / "in_system.bin"))
    exe = str(tmp_path / "gfx_fractal")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + ROOT,
                           os.path.join(ROOT, "tests", "cpp", "test_gfx_fractal.cpp"), "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gfx fractal ok" in r.stdout, r.stdout + r.stderr
    with open(str(tmp_path / "out_transcript.bin"), "rb") as f:
        mine = f.read()
    with open(str(tmp_path / "out_roots.bin"), "rb") as f:
        raw = f.read()
    roots = [raw[i:i + 32] for i in range(0, len(raw), 32)]
    inst = lib.aurora_instance(libiop_amd.FIELD_GF64, matrices, num_variables, num_inputs, z)
    try:
        with F.C.options(lib, **{F.OPTION: 1}):
            assert roots == [bytes(x) for x in lib.fractal_index(inst, 128, rs_extra, loc)]
            assert mine == lib.fractal_prove(inst, 128, rs_extra, loc)
    finally:
        lib.aurora_instance_free(inst)
    ref, ref_roots = oracle.fractal_prove_csr(oracle.FIELD_GF64, matrices, num_variables, num_inputs, z, rs_extra=rs_extra, localization=loc)
    assert roots == ref_roots and mine == ref, F.first_difference(mine, ref)


def test_gfx_fractal_seam_on_the_cpu_build(tmp_path):
    from emu_lib import emu
    _run(tmp_path, emu(), os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so")


@pytest.mark.gpu
def test_gfx_fractal_seam_on_the_gpu(tmp_path):
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    _run(tmp_path, lib, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH))
