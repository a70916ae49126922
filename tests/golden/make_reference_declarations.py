"""Generates tests/golden/reference_declarations.json (run where the reference tree is present): the declarations of the reference headers that
tests/test_reference_signatures.py compares with the mirror, as that test's parser extracts them — return type, parameter types, constness.

    python tests/golden/make_reference_declarations.py [/path/to/reference/libiop]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_reference_signatures as sig  # noqa: E402


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/libiop"
    decls = sig.reference_declarations(ref_root)
    with open(os.path.join(HERE, "reference_declarations.json"), "w") as f:
        json.dump({"generated_by": "tests/golden/make_reference_declarations.py",
                   "what": "declarations in the reference's libiop/ headers, normalised by tests/test_reference_signatures.py: "
                           "[return type, [parameter types], const] per member or function, [parameter types] for a constructor",
                   "declarations": decls}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(decls), "declarations")


if __name__ == "__main__":
    main()
