"""The fifth public header: include/libiop_amd_fractal.h (included by libiop_amd.h) declares what the Fractal prover needs over gf64, gf128 and gf256 from
one parameterised text.  Its expansion and libiop_amd.FRACTAL_SYMBOLS agree, the list is disjoint from the other four, the product library exports
every name, the C++ dispatch table fills the five slots for every binary field, and a C99 translation unit that includes libiop_amd.h alone sees the
declarations."""
import os
import re
import subprocess

import libiop_amd
from libiop_amd import build as iopx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GF192 = ["iopx_gf192_div_dev", "iopx_domain_offsets_gf192_dev", "iopx_vanishing_evals_gf192_dev", "iopx_rational_combine_gf192_dev",
         "iopx_rational_sumcheck_constraint_gf192_dev"]


def _declared():
    text = open(os.path.join(ROOT, "include", "libiop_amd_fractal.h")).read()
    body = text[text.index("#define IOPX_DECLARE_FRACTAL(FIELD)"):]
    patterns = re.findall(r"\b(iopx_[a-z0-9_#FIELD]+)\s*\(", body)
    fields = re.findall(r"^IOPX_DECLARE_FRACTAL\((\w+)\)", text, re.M)
    return sorted(p.replace("##FIELD##", f) for f in fields for p in patterns)


def test_header_and_binding_agree():
    assert len(_declared()) == 15 and _declared() == sorted(libiop_amd.FRACTAL_SYMBOLS)
    others = set(libiop_amd.EXPORTED_SYMBOLS) | set(libiop_amd.GFX_OPS_SYMBOLS) | set(libiop_amd.BATCH_SYMBOLS) | set(libiop_amd.HEAD_SYMBOLS)
    assert not set(libiop_amd.FRACTAL_SYMBOLS) & others
    text = open(os.path.join(ROOT, "include", "libiop_amd_fractal.h")).read()
    assert "#undef IOPX_DECLARE_FRACTAL" in text
    assert '#include "libiop_amd_fractal.h"' in open(os.path.join(ROOT, "include", "libiop_amd.h")).read()


def test_library_exports_every_declared_symbol():
    iopx_build.build()
    lib = libiop_amd.Library()
    for name in _declared():
        assert hasattr(lib.c, name), name


def test_the_field_table_names_every_entry():
    """libiop_amd/cpp/field_ops.hpp: each of the fifteen names, and gf192's five, in a table; no slot of a binary field is null; fractal.hpp names none"""
    text = open(os.path.join(ROOT, "libiop_amd", "cpp", "field_ops.hpp")).read()
    for name in libiop_amd.FRACTAL_SYMBOLS + GF192:
        assert re.search(r"^    .*\b%s\b" % name, text, re.M), name
    tables = text[text.index("inline constexpr vector_ops gf192"):text.index("inline constexpr prime_field_ops edwards_Fr")]
    assert "nullptr" not in tables
    code = open(os.path.join(ROOT, "libiop_amd", "cpp", "fractal.hpp")).read()
    assert not re.search(r"iopx_\w+_div_dev|iopx_domain_offsets_\w+_dev|iopx_vanishing_evals_\w+_dev|iopx_rational_\w+_dev", code)


def test_the_python_tables_name_the_entries():
    from libiop_amd import domains
    for field in (domains.GF64, domains.GF128, domains.GF256):
        for op in ("div", "domain_offsets", "vanishing_evals", "rational_combine", "rational_sumcheck_constraint"):
            assert field.entries[op][1] == {"words": field.words}, (field.name, op)
            assert field.entries[op][0] == domains.GF192.entries[op][0], (field.name, op)
    allowed = {n for n in domains._OPERATORS if getattr(domains.GF64FractalOps, n) is getattr(domains.DeviceOps, n)}
    assert allowed == domains._GF64_AURORA | {"div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine",
                                              "rational_sumcheck_constraint"}


def test_the_main_header_brings_the_declarations(tmp_path):
    src = tmp_path / "uses.c"
    src.write_text('#include "include/libiop_amd.h"\n'
                   'int (*const div[])(const uint64_t *, const uint64_t *, uint64_t *, size_t) = '
                   '{ iopx_gf64_div_dev, iopx_gf128_div_dev, iopx_gf256_div_dev, iopx_gf192_div_dev };\n'
                   'int (*const offsets[])(const uint64_t *, size_t, const uint64_t *, const uint64_t *, uint64_t *) = '
                   '{ iopx_domain_offsets_gf64_dev, iopx_domain_offsets_gf128_dev, iopx_domain_offsets_gf256_dev, iopx_domain_offsets_gf192_dev };\n'
                   'int (*const evals[])(const uint64_t *, size_t, const uint64_t *, const uint64_t *, size_t, const uint64_t *, const uint64_t *, uint64_t *) = '
                   '{ iopx_vanishing_evals_gf64_dev, iopx_vanishing_evals_gf128_dev, iopx_vanishing_evals_gf256_dev, iopx_vanishing_evals_gf192_dev };\n'
                   'int (*const combine[])(const void *const *, const void *const *, size_t, const uint64_t *, size_t, uint64_t *, uint64_t *) = '
                   '{ iopx_rational_combine_gf64_dev, iopx_rational_combine_gf128_dev, iopx_rational_combine_gf256_dev, iopx_rational_combine_gf192_dev };\n'
                   'int (*const constraint[])(const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, size_t, const uint64_t *, size_t, '
                   'const uint64_t *, const uint64_t *, uint64_t *) = { iopx_rational_sumcheck_constraint_gf64_dev, iopx_rational_sumcheck_constraint_gf128_dev, '
                   'iopx_rational_sumcheck_constraint_gf256_dev, iopx_rational_sumcheck_constraint_gf192_dev };\n'
                   '#ifdef IOPX_DECLARE_FRACTAL\n#error "the declaring macro leaked"\n#endif\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "uses.o")])
