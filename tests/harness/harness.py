"""TEST INFRASTRUCTURE ONLY — container-only: build and run the reference-over-shim programs of tests/harness.

`reference_plain`    the reference's own Aurora / Fractal prover and verifier, compiled straight from /root/reference over the stand-in libff /
                     libfqfft of tests/harness/shim (field arithmetic = this repository's host code);
`reference_stubbed`  the same program with the stubs of INTEGRATION.md compiled in verbatim (tests/harness/make_shadow.py), forwarding to the CPU build
                     of the kernel sources (tests/emu) through the C ABI.
Nothing of the reference is copied; build() compiles the programs into oracle/_ref/build (git-ignored) by the recipe oracle/reference.mk, and the
tests run what it left there."""
import hashlib
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
CONDA = "/opt/conda"
RECIPE = os.path.join(ROOT, "oracle", "reference.mk")
BUILD = os.path.join(ROOT, "oracle", "_ref", "build")

# (protocol, field, log_n, num_inputs, seed, rs_extra): the instrument programs' settings (instrument_aurora_snark.cpp:95-122: RS_extra_dimensions 5 non-zk,
# k = 15; instrument_fractal_snark.cpp:93-110: 3, k = 15 over subspaces and 0 over cosets), localization parameter 2
CASES = [("aurora", "gf192", 6, 15, 0x2204, 5), ("aurora", "gf192", 8, 15, 0x2204, 5), ("aurora", "gf192", 10, 15, 0x2204, 5), ("aurora", "gf192", 12, 15, 0x2204, 5),
         ("aurora", "edwards_Fr", 8, 15, 0x2204, 5), ("aurora", "edwards_Fr", 10, 15, 0x2204, 5), ("aurora", "edwards_Fr", 12, 15, 0x2204, 5),
         ("fractal", "gf192", 7, 15, 0x2205, 3), ("fractal", "gf192", 9, 15, 0x2205, 3),
         ("fractal", "edwards_Fr", 8, 0, 0x2205, 3), ("fractal", "edwards_Fr", 11, 0, 0x2205, 3)]


def buildable():
    """None when the programs can be compiled here, else the reason they cannot."""
    if not os.path.isdir(os.path.join(REFERENCE, "libiop")):
        return "no /root/reference (the reference tree exists in the build container only)"
    for f in ("include/sodium.h", "include/gmp.h", "lib/libsodium.so.23", "lib/libgmp.so.10"):
        if not os.path.exists(os.path.join(CONDA, f)):
            return "no %s/%s (libiop needs libsodium and GMP)" % (CONDA, f)
    return None


# libiop's own test files run as programs (oracle/reference.mk REFTESTS); the default subset (three programs, seconds each, built by build()) keeps the CPU suite
# short, IOPX_REFTESTS=all runs the 34
REFTESTS_DEFAULT = ["protocols/test_fri_aux", "protocols/test_aurora_protocol", "protocols/test_direct_ldt"]
# what build() leaves in oracle/_ref/build for the CPU suite (oracle/reference.mk, target `all`)
PROGRAMS = ["stubs.inc", "reference_plain", "reference_stubbed", "reference_vectors"]


def available():
    """None when the programs build() compiles from the reference tree are present, else the reason they are not."""
    for name in PROGRAMS + ["reftests/stubbed/" + t for t in REFTESTS_DEFAULT]:
        if not os.path.exists(os.path.join(BUILD, name)):
            why = buildable()
            return "oracle/_ref/build/%s was not built (build() compiles it where the reference tree is present%s)" % (name, "" if why is None else ": " + why)
    return None


def _make(targets):
    """xdist workers start together: one make at a time; targets are paths under oracle/_ref/build (or recipe targets such as `all`)"""
    import fcntl
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-j8", "-f", RECIPE, "-C", ROOT] +
                              [t if t in ("all", "hip") or t.startswith("reftests_") else os.path.join(BUILD, t) for t in targets])


def build(stubbed=True):
    _make(["reference_plain"] + (["reference_stubbed"] if stubbed else []))


def run(variant, protocol, field, log_n, num_inputs, seed, rs_extra, localization=2):
    """-> {"transcript": bytes, "verifier_accepts": bool, "index_roots": [bytes], "kernel_launches_in_prover": {name: count}}"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "t.bin")
        r = subprocess.run([os.path.join(BUILD, "reference_" + variant), protocol, field, str(log_n), str(num_inputs), hex(seed), str(rs_extra),
                            str(localization), out], capture_output=True, text=True, timeout=1800)
        assert r.returncode in (0, 1), (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
        info = json.loads(r.stdout.strip().splitlines()[-1])
        with open(out, "rb") as f:
            info["transcript"] = f.read()
    info["index_roots"] = [bytes.fromhex(x) for x in info["index_roots"]]
    return info


def digest(b):
    return hashlib.blake2b(b, digest_size=32).hexdigest()


def reftests():
    if os.environ.get("IOPX_REFTESTS") == "all":
        out = subprocess.run(["make", "-s", "-f", RECIPE, "-C", ROOT, "-pn"], capture_output=True, text=True).stdout
        for line in out.splitlines():
            if line.startswith("REFTESTS :="):
                return line.split(":=")[1].split()
    return list(REFTESTS_DEFAULT)


def build_reftest(name, variant="stubbed"):
    """the default programs come from build(); any other is compiled on first use (needs the reference tree)"""
    if not os.path.exists(os.path.join(BUILD, "reftests", variant, name)):
        _make(["reftests/%s/%s" % (variant, name)])


# the two tests that feed raw random bytes as edwards_Fr elements (tests/harness/run_reftests.py FILTER)
REFTEST_FILTER = {"protocols/test_ligero_interleaved_lincheck_et": "--gtest_filter=-InterleavedLincheckETTrueMultiplicativeTest.*",
                  "protocols/test_ligero_interleaved_lincheck_ot": "--gtest_filter=-InterleavedLincheckOTTrueMultiplicativeTest.*"}


def run_reftest(name, variant="stubbed"):
    """-> (tests run, tests passed, {kernel: launches}, tail of the output)"""
    r = subprocess.run([os.path.join(BUILD, "reftests", variant, name)] + ([REFTEST_FILTER[name]] if name in REFTEST_FILTER and variant != "plain" else []),
                       capture_output=True, text=True, timeout=1800)
    lines = r.stdout.splitlines()
    ran = sum(1 for l in lines if l.startswith("[ RUN "))
    ok = sum(1 for l in lines if l.startswith("[       OK ]"))
    kernels = {}
    if "[ KERNELS  ]" in r.stdout:
        for l in r.stdout.split("[ KERNELS  ]")[1].split("[ /KERNELS ]")[0].splitlines():
            parts = l.split()
            if len(parts) >= 2 and parts[0].startswith("k_"):
                kernels[parts[0]] = int(parts[1])
    return ran, ok, kernels, (r.stdout[-600:] + r.stderr[-600:]) if r.returncode else ""
