"""The fourth public header: include/libiop_amd_head.h (included by libiop_amd.h) declares what head evaluation needs over gf64, gf128 and gf256 from
one parameterised text.  Its expansion and libiop_amd.HEAD_SYMBOLS agree, the list is disjoint from the other three, the product library exports
every name, the C++ dispatch table fills the three slots for every binary field, and a C99 translation unit that includes libiop_amd.h alone sees
the declarations."""
import os
import re
import subprocess

import libiop_amd
from libiop_amd import build as iopx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "libiop_amd_head.h")).read()
    body = text[text.index("#define IOPX_DECLARE_HEAD(FIELD)"):]
    patterns = re.findall(r"\b(iopx_[a-z0-9_#FIELD]+)\s*\(", body)
    fields = re.findall(r"^IOPX_DECLARE_HEAD\((\w+)\)", text, re.M)
    return sorted(p.replace("##FIELD##", f) for f in fields for p in patterns)


def test_header_and_binding_agree():
    assert len(_declared()) == 9 and _declared() == sorted(libiop_amd.HEAD_SYMBOLS)
    others = set(libiop_amd.EXPORTED_SYMBOLS) | set(libiop_amd.GFX_OPS_SYMBOLS) | set(libiop_amd.BATCH_SYMBOLS)
    assert not set(libiop_amd.HEAD_SYMBOLS) & others
    text = open(os.path.join(ROOT, "include", "libiop_amd_head.h")).read()
    assert "#undef IOPX_DECLARE_HEAD" in text


def test_library_exports_every_declared_symbol():
    iopx_build.build()
    lib = libiop_amd.Library()
    for name in _declared():
        assert hasattr(lib.c, name), name


def test_the_field_table_names_every_entry():
    """libiop_amd/cpp/field_ops.hpp: each of the nine names, and gf192's three, in a subspace_ops table; aurora.hpp names none of them"""
    text = open(os.path.join(ROOT, "libiop_amd", "cpp", "field_ops.hpp")).read()
    for name in libiop_amd.HEAD_SYMBOLS + ["iopx_div_by_vanishing_gf192_dev", "iopx_gf192_vanishing_host", "iopx_add_reextend2_gf192_batch_dev"]:
        assert re.search(r"^    .*\b%s\b" % name, text, re.M), name
    for header in ("aurora.hpp", "device.hpp"):
        code = open(os.path.join(ROOT, "libiop_amd", "cpp", header)).read()
        assert not re.search(r"iopx_div_by_vanishing_\w+_dev|iopx_add_reextend2_\w+_batch_dev|iopx_\w+_vanishing_host", code), header


def test_the_main_header_brings_the_declarations(tmp_path):
    src = tmp_path / "uses.c"
    src.write_text('#include "include/libiop_amd.h"\n'
                   'int (*const div[])(const uint64_t *, const uint64_t *, size_t, const uint64_t *, size_t, const uint64_t *, uint64_t *) = '
                   '{ iopx_div_by_vanishing_gf64_dev, iopx_div_by_vanishing_gf128_dev, iopx_div_by_vanishing_gf256_dev, iopx_div_by_vanishing_gf192_dev };\n'
                   'int (*const host[])(const uint64_t *, size_t, const uint64_t *, const uint64_t *, uint64_t *, uint64_t *) = '
                   '{ iopx_gf64_vanishing_host, iopx_gf128_vanishing_host, iopx_gf256_vanishing_host, iopx_gf192_vanishing_host };\n'
                   'int (*const re2[])(const uint64_t *, size_t, const uint64_t *, const uint64_t *, size_t, const uint64_t *, const uint64_t *, size_t, size_t, const uint64_t *, '
                   'size_t, size_t, uint64_t *const *) = { iopx_add_reextend2_gf64_batch_dev, iopx_add_reextend2_gf128_batch_dev, iopx_add_reextend2_gf256_batch_dev, '
                   'iopx_add_reextend2_gf192_batch_dev };\n'
                   '#ifdef IOPX_DECLARE_HEAD\n#error "the declaring macro leaked"\n#endif\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "uses.o")])
