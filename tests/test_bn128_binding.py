"""The alt_bn128 Fr stubs of INTEGRATION.md (the blocks marked `bn128:def`), compiled VERBATIM into tests/cpp/test_bn128_binding.cpp against the mirror
classes with the 32-byte stand-in field of libiop_amd/cpp/fields.hpp, run on the CPU build of the kernels and (-m gpu) against the HIP library; the
stubs' outputs must equal the integer-only vectors of tests/golden/bn128_tiny.json, and the mirror's own dispatchers must agree with the stubs."""
import os
import re
import subprocess

import numpy as np
import pytest

import bn128_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_blocks():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    blocks = re.findall(r"<!-- bn128:def -->\s*```cpp\n(.*?)```", text, re.S)
    assert len(blocks) == 2
    return "\n".join(blocks)


def _inputs(d):
    fold_shift = C.seeded_scalar("fold shift")
    scalars = [C.seeded_scalar("fft shift"), fold_shift, C.fold_x(6, False, fold_shift)] + \
              [C.seeded_scalar("ldt coefficient %d" % i) for i in range(6)]
    np.concatenate([C.elem(v).reshape(1, 4) for v in scalars]).tofile(os.path.join(d, "in_scalars.bin"))
    C.data_words("fft 6", 64)[:33].tofile(os.path.join(d, "in_fft.bin"))
    C.data_words("fold 6 2", 64).tofile(os.path.join(d, "in_fold.bin"))
    np.concatenate([C.data_words("ldt %d" % k, 32) for k in range(3)]).tofile(os.path.join(d, "in_ldt.bin"))


def _run(tmp_path, lib_dir, lib_file):
    (tmp_path / "bn128_stubs.inc").write_text(_stub_blocks())
    exe = str(tmp_path / "bn128_binding")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror=return-type", "-I" + ROOT, "-I" + str(tmp_path),
                           os.path.join(ROOT, "tests", "cpp", "test_bn128_binding.cpp"), "-o", exe, os.path.join(lib_dir, lib_file), "-Wl,-rpath," + lib_dir])
    _inputs(str(tmp_path))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bn128 stubs ok" in r.stdout, r.stdout + r.stderr
    want = C.load_json("bn128_tiny.json")["cases"]

    def out(name):
        return np.fromfile(str(tmp_path / ("out_%s.bin" % name)), dtype=np.uint64).reshape(-1, 4)
    assert C.digest(out("fft")) == want["fft"]["fft_6_seeded_33"]
    assert C.digest(out("fold")) == want["fold"]["fold_6_2_seeded"]
    assert C.digest(out("ldt")) == want["ldt"]["ldt_5"]


def test_bn128_stubs_on_the_cpu_build(tmp_path):
    from emu_lib import emu
    emu()
    _run(tmp_path, os.path.join(ROOT, "tests", "emu"), "libiopx_emu.so")


@pytest.mark.gpu
def test_bn128_stubs_on_the_gpu(tmp_path):
    import libiop_amd
    _run(tmp_path, os.path.dirname(libiop_amd.LIB_PATH), os.path.basename(libiop_amd.LIB_PATH))
