"""The C++ seam of Fractal over gf128 and gf256: tests/cpp/test_gfx_fractal_wide.cpp compiled against libiop_amd/cpp/fractal.hpp with the gf128 and
gf256 types of cpp/fields.hpp, run on the CPU build of the kernels and (-m gpu) against the HIP library.  It proves
gfx_fractal_wide_cases.hand_built_system(W) with fractal_snark_prover<gf128> / <gf256> under IOPX_GFX_FRACTAL_WIDE=1; its index roots and bytes must
equal the C ABI's on the same library and the model's (tests/gfx_fractal_model.py, which tests/test_gfx_fractal_wide_emu.py holds to the oracle; on
the MI355X through the model's recorded digests, tests/golden/gfx_fractal_wide.json)."""
import os
import subprocess

import numpy as np
import pytest

import gfx_fractal_cases as F
import gfx_fractal_wide_cases as FW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = pytest.mark.parametrize("words", FW.WORDS, ids=lambda w: FW.NAME[w])


def _run(tmp_path, lib, lib_dir, lib_file, words, through_digest=False):
    """through_digest: the model's recorded digests stand for the model (the MI355X leg; the CPU leg holds the digests to the model)"""
    import hashlib
    if through_digest:
        system, rs_extra, loc = FW.hand_built_system(words)
        pin = FW.hand_built_digests(words)
        z, want_roots, want = system["z"], [bytes.fromhex(r) for r in pin["index_roots"]], None
        assert pin["assignments"]["good"]["degrees_hold"]
    else:
        system, rs_extra, loc, want_roots, runs = FW.hand_built_model(words)
        z, want, degrees_hold = runs["good"]
        assert degrees_hold
    matrices, num_variables, num_inputs = system["matrices"], system["num_variables"], system["num_inputs"]
    n = len(matrices[0][0]) - 1
    parts = [np.array([n, num_variables, num_inputs, rs_extra, loc], dtype=np.uint64)]
    for row_ptr, col, coeff in matrices:
        parts += [row_ptr.astype(np.uint64), col.astype(np.uint64), coeff.reshape(-1)]
    np.concatenate(parts + [z.reshape(-1)]).astype(np.uint64).tofile(str(tmp_path / "in_system.bin"))
    exe = str(tmp_path / "gfx_fractal_wide")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + ROOT,
                           os.path.join(ROOT, "tests", "cpp", "test_gfx_fractal_wide.cpp"), "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, str(tmp_path), str(words)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gfx fractal wide ok" in r.stdout, r.stdout + r.stderr
    with open(str(tmp_path / "out_transcript.bin"), "rb") as f:
        mine = f.read()
    with open(str(tmp_path / "out_roots.bin"), "rb") as f:
        raw = f.read()
    roots = [raw[i:i + 32] for i in range(0, len(raw), 32)]
    abi_roots, (abi,), _ = FW.native_index_and_prove(lib, words, system, rs_extra, loc)
    assert roots == abi_roots and mine == abi, F.first_difference(mine, abi)
    assert roots == want_roots
    if through_digest:
        assert (len(mine), hashlib.sha256(mine).hexdigest()) == (pin["assignments"]["good"]["bytes"], pin["assignments"]["good"]["sha256"])
    else:
        assert mine == want, F.first_difference(mine, want)


@W
def test_gfx_fractal_wide_seam_on_the_cpu_build(tmp_path, words):
    from emu_lib import emu
    _run(tmp_path, emu(), os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so", words)


@pytest.mark.gpu
@W
def test_gfx_fractal_wide_seam_on_the_gpu(tmp_path, words):
    import libiop_amd
    lib = libiop_amd.lib()
    lib.init(0)
    _run(tmp_path, lib, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH), words, through_digest=True)
