"""The third public header: include/libiop_amd_batch.h (included by libiop_amd.h) declares the batched transforms and the fused re-extension over
gf64, gf128 and gf256 from one parameterised text.  Its expansion and libiop_amd.BATCH_SYMBOLS agree, the list is disjoint from the other two, the
product library exports every name, the C++ dispatch table fills the four slots for every binary field, and a C99 translation unit that includes
libiop_amd.h alone sees the declarations."""
import os
import re
import subprocess

import libiop_amd
from libiop_amd import build as iopx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "libiop_amd_batch.h")).read()
    body = text[text.index("#define IOPX_DECLARE_ADD_BATCH(FIELD)"):]
    patterns = re.findall(r"\b(iopx_[a-z0-9_#FIELD]+)\s*\(", body)
    fields = re.findall(r"^IOPX_DECLARE_ADD_BATCH\((\w+)\)", text, re.M)
    return sorted(p.replace("##FIELD##", f) for f in fields for p in patterns)


def test_header_and_binding_agree():
    assert len(_declared()) == 12 and _declared() == sorted(libiop_amd.BATCH_SYMBOLS)
    assert not set(libiop_amd.BATCH_SYMBOLS) & (set(libiop_amd.EXPORTED_SYMBOLS) | set(libiop_amd.GFX_OPS_SYMBOLS))


def test_library_exports_every_declared_symbol():
    iopx_build.build()
    lib = libiop_amd.Library()
    for name in _declared():
        assert hasattr(lib.c, name), name


def test_the_field_tables_name_every_entry():
    """libiop_amd/cpp/field_ops.hpp: each of the twelve names, and gf192's four, in a subspace_ops table; domains.py: the three keys per field"""
    text = open(os.path.join(ROOT, "libiop_amd", "cpp", "field_ops.hpp")).read()
    for name in libiop_amd.BATCH_SYMBOLS + ["iopx_add_%s_gf192_batch_dev" % k for k in ("ifft", "lde", "reextend", "reextend_lde")]:
        assert re.search(r"^    .*\b%s\b" % name, text, re.M), name
    from libiop_amd import domains
    for field in (domains.GF64, domains.GF128, domains.GF256):
        for key in ("IFFT_batch", "LDE_batch", "reextend_batch"):
            assert field.entries[key][1] == {"words": field.words}, (field.name, key)


def test_the_main_header_brings_the_declarations(tmp_path):
    src = tmp_path / "uses.c"
    src.write_text('#include "include/libiop_amd.h"\n'
                   'int (*const ifft[])(const uint64_t *, size_t, const uint64_t *, size_t, const uint64_t *, uint64_t *) = { iopx_add_ifft_gf64_batch_dev, iopx_add_ifft_gf192_batch_dev };\n'
                   'int (*const lde)(const uint64_t *const *, size_t, size_t, const uint64_t *, size_t, const uint64_t *, size_t, size_t, uint64_t *const *) = iopx_add_lde_gf128_batch_dev;\n'
                   'int (*const re[])(const uint64_t *, size_t, const uint64_t *, size_t, size_t, const uint64_t *, const uint64_t *, size_t, size_t, uint64_t *const *) = '
                   '{ iopx_add_reextend_gf256_batch_dev, iopx_add_reextend_gf192_batch_dev };\n'
                   'int (*const relde)(const uint64_t *, size_t, const uint64_t *const *, size_t, size_t, const uint64_t *, size_t, size_t, const uint64_t *, const uint64_t *, size_t, size_t, '
                   'uint64_t *const *) = iopx_add_reextend_lde_gf64_batch_dev;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "uses.o")])
