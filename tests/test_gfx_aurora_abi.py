"""The second public header: include/libiop_amd_gfx.h (included by libiop_amd.h) declares the protocol-layer entries of Aurora over gf128 and
gf256 from one parameterised text.  Its expansion and libiop_amd.GFX_OPS_SYMBOLS agree, the product library exports every one of them, and
a C translation unit that includes libiop_amd.h alone sees them."""
import os
import re
import subprocess

import libiop_amd
from libiop_amd import build as iopx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "libiop_amd_gfx.h")).read()
    body = text[text.index("#define IOPX_DECLARE_GFX_OPS(FIELD)"):]
    patterns = re.findall(r"\b(iopx_[a-z0-9_#FIELD]+)\s*\(", body)
    fields = re.findall(r"^IOPX_DECLARE_GFX_OPS\((\w+)\)", text, re.M)
    return sorted(p.replace("##FIELD##", f) for f in fields for p in patterns)


def test_header_and_binding_agree():
    assert len(_declared()) == 18 and _declared() == sorted(libiop_amd.GFX_OPS_SYMBOLS)
    assert not set(libiop_amd.GFX_OPS_SYMBOLS) & set(libiop_amd.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol():
    iopx_build.build()
    lib = libiop_amd.Library()
    for name in _declared():
        assert hasattr(lib.c, name), name


def test_the_main_header_brings_the_declarations(tmp_path):
    src = tmp_path / "uses.c"
    src.write_text('#include "include/libiop_amd.h"\nint (*const probe[])(uint64_t *, size_t, const uint64_t *, const uint64_t *) = { iopx_gf128_pow_table_dev, iopx_gf256_pow_table_dev, iopx_gf64_pow_table_dev };\n'
                   'int (*const probe2)(const uint64_t *, size_t, const uint64_t *, size_t, const uint64_t *, uint64_t *) = iopx_poly_div_vanishing_gf256_dev;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "uses.o")])
