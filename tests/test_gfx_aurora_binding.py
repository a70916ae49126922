"""The C++ seam of Aurora over GF(2^128) and GF(2^256): tests/cpp/test_gfx_aurora.cpp compiled against libiop_amd/cpp/aurora.hpp with the 16- and
32-byte types of cpp/fields.hpp, run on the CPU build of the kernels and (-m gpu) against the HIP library.  It proves a hand-built constraint
system (two-term rows, a constant column); its bytes must equal the C ABI's on the same library and the model's (tests/gfx_aurora_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import gfx_aurora_cases as C
import gfx_aurora_model as M
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = pytest.mark.parametrize("words", C.WORDS, ids=lambda w: C.NAME[w])


def hand_built_system(W):
    """(instance, rs_extra, localization): 64 constraints over 63 variables, (z_a + c1 z_a') * (c2 z_b or the constant c2) = coef z_c with coef
    chosen so that the seeded assignment satisfies it"""
    n, num_inputs = 64, 3
    z = C.seeded("hand-built z", n - 1, W)
    full = np.concatenate([C.elem(W, 1).reshape(1, W), z])
    i = np.arange(n)
    a1, a2, b, c = i % (n - 1) + 1, (3 * i + 5) % (n - 1) + 1, np.where(i % 5 == 0, 0, (i + 11) % (n - 1) + 1), (2 * i + 1) % (n - 1) + 1
    c1, c2 = C.seeded("hand-built c1", n, W), C.seeded("hand-built c2", n, W)
    az = full[a1] ^ oracle.gf_mul(c1, full[a2])
    bz = oracle.gf_mul(c2, full[b])
    coef = oracle.gf_mul(oracle.gf_mul(az, bz), oracle.gf_inv(full[c]))
    ones = np.ascontiguousarray(np.broadcast_to(C.elem(W, 1), (n, W)))
    A = (2 * np.arange(n + 1, dtype=np.uint64), np.stack([a1, a2], axis=1).reshape(-1).astype(np.uint32), np.stack([ones, c1], axis=1).reshape(-1, W))
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    matrices = [A, (row_ptr, b.astype(np.uint32), c2), (row_ptr, c.astype(np.uint32), coef)]
    return {"matrices": matrices, "z": z, "num_variables": n - 1, "num_inputs": num_inputs}, 3, 2


def _run(tmp_path, lib, lib_dir, lib_file, W):
    inst, rs_extra, loc = hand_built_system(W)
    matrices, z = inst["matrices"], inst["z"]
    n = len(matrices[0][0]) - 1
    words = [np.array([n, inst["num_variables"], inst["num_inputs"], rs_extra, loc], dtype=np.uint64)]
    for row_ptr, col, coeff in matrices:
        words += [row_ptr.astype(np.uint64), col.astype(np.uint64), coeff.reshape(-1)]
    np.concatenate(words + [z.reshape(-1)]).astype(np.uint64).tofile(str(tmp_path / "in_system.bin"))
    exe = str(tmp_path / "gfx_aurora")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-DGFX_WORDS=%d" % W, "-I" + ROOT,
                           os.path.join(ROOT, "tests", "cpp", "test_gfx_aurora.cpp"), "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gfx aurora ok" in r.stdout, r.stdout + r.stderr
    with open(str(tmp_path / "out_transcript.bin"), "rb") as f:
        mine = f.read()
    assert mine == C.native_prove(lib, W, inst, rs_extra, loc)
    want = M.prove(W, inst, rs_extra, loc)
    assert mine == want, C.first_difference(mine, want)


@pytest.mark.parametrize("words, ofield", [(1, oracle.FIELD_GF64), (3, oracle.FIELD_GF192)], ids=["gf64", "gf192"])
def test_model_reproduces_the_oracle_on_the_hand_built_system(words, ofield):
    """the trust condition on this file's own instance: two-term rows and a constant column, rate 3"""
    inst, rs_extra, loc = hand_built_system(words)
    want = oracle.aurora_prove_csr(ofield, inst["matrices"], inst["num_variables"], inst["num_inputs"], inst["z"], rs_extra=rs_extra, localization=loc)
    assert M.prove(words, inst, rs_extra, loc) == want


@WORDS
def test_gfx_aurora_seam_on_the_cpu_build(tmp_path, words):
    from emu_lib import emu
    _run(tmp_path, emu(), os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so", words)


@pytest.mark.gpu
@WORDS
def test_gfx_aurora_seam_on_the_gpu(tmp_path, words):
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    _run(tmp_path, lib, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH), words)
