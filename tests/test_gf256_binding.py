"""The C++ seam over GF(2^256): tests/cpp/test_gf256_binding.cpp compiled against libiop_amd/cpp/libiop_amd.hpp with the 32-byte gf256 type of
cpp/fields.hpp, run on the CPU build of the kernels and (-m gpu) against the HIP library.  The program checks the round trips, the dispatchers
and the fold template against the C entry, refuses multiplicative_coset<gf256>, keeps the 32-byte prime type on alt_bn128 Fr's arm and runs
FRI_snark_prover<gf256>; its outputs must equal the oracle's and the prover model's."""
import os
import subprocess

import numpy as np
import pytest

import gf256_cases as C
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, lib_dir, lib_file):
    exe = str(tmp_path / "gf256_binding")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + ROOT,
                           os.path.join(ROOT, "tests", "cpp", "test_gf256_binding.cpp"), "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    shift, x = C.elem((1 << 255) | 0x99), C.seeded("binding x", 1)[0]
    basis, dshift = oracle.fri_domains_additive(C.std_basis(9), C.elem((0x1234 << 200) | 0x77), [2])[0]
    np.concatenate([shift, x, basis.reshape(-1), dshift.reshape(-1)]).astype(np.uint64).tofile(str(tmp_path / "in_scalars.bin"))
    coeffs, f = C.seeded("binding fft", 100), C.seeded("binding fold", 128)
    coeffs.tofile(str(tmp_path / "in_fft.bin"))
    f.tofile(str(tmp_path / "in_fold.bin"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gf256 binding ok" in r.stdout, r.stdout + r.stderr

    def out(name):
        return np.fromfile(str(tmp_path / ("out_%s.bin" % name)), dtype=np.uint64).reshape(-1, 4)
    assert np.array_equal(out("fft"), oracle.additive_fft(coeffs, C.std_basis(9), shift))
    assert np.array_equal(out("fold"), oracle.fri_fold_additive(f, basis, dshift, 4, x))
    with open(str(tmp_path / "out_fri.bin"), "rb") as fh:
        assert fh.read() == C.model_bytes(4, C.FRI_SNARK_TUPLES[0])


def test_gf256_binding_on_the_cpu_build(tmp_path):
    from emu_lib import emu
    emu()
    _run(tmp_path, os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so")


@pytest.mark.gpu
def test_gf256_binding_on_the_gpu(tmp_path):
    import libiop_amd
    _run(tmp_path, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH))
