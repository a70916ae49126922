"""Whole-output pins for BASELINE configs 2 and 3 at their own sizes: the additive FFT / IFFT on a 2^22-point subspace (standard and general
bases), the FRI fold chains of the config-3 codeword (fused and unfused folds), and the FRI SNARKs of dimension 22.  One module holds the input
recipes, the call sequences and the digest function, shared by the fixture's generator (tests/golden/make_oracle_function_digests_large.py, which
runs the oracle), the GPU tests (tests/test_gpu_fullsize.py, full size) and the CPU-build tests (tests/test_fullsize_recipes_emu.py, the fixture's
"small" sizes).  Every recipe is a function of the size, so that the CPU build proves the GPU tests build the generator's inputs.

Digests are BLAKE2b-256 of the (n, 3) uint64 array's bytes, little-endian, row-major; chunk digests cover 2^log_chunk consecutive elements each, so
that a mismatch says which region of the output is wrong."""
import hashlib
import json
import os

import numpy as np

import oracle
from helpers import rand_elems

W = 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_function_digests_large.json")

LARGE_M = 22                                 # config 2's subspace, config 3's codeword domain
SMALL_MS, SMALL_DIM = (10, 12), 12
LARGE_LOG_CHUNK, SMALL_LOG_CHUNK = 16, 6
RS_EXTRA = 2                                 # config 3: degree 2^(m - 2) on the 2^m-point domain

# Fixture keys; "{m}" is the size the recipe runs at (the subspace / codeword domain dimension)
TRANSFORMS = ("add_fft/std0/shift0", "add_fft/std0/shift_x{m}", "add_fft/general", "add_ifft/std0/shift0", "add_ifft/general")
FOLD_CHAINS = {"fold_chain/cfg3": 2, "fold_chain/loc4": 4}          # FRI localization parameter
INTERACTIONS, QUERIES, SNARK_SEED = 1, 10, 0x2203
SNARKS = tuple("fri_snark/%s/{m}/%d/%d/%d/%d" % (f, RS_EXTRA, loc, INTERACTIONS, QUERIES) for f, loc in (("gf192", 2), ("gf192", 4), ("edwards_Fr", 2)))


def keys(m):
    return [k.format(m=m) for k in TRANSFORMS + tuple(FOLD_CHAINS) + SNARKS]


def digest(arr):
    return hashlib.blake2b(np.ascontiguousarray(arr, dtype=np.uint64).tobytes(), digest_size=32).hexdigest()


def chunk_digests(arr, log_chunk):
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    c = 1 << log_chunk
    return [digest(a[i:i + c]) for i in range(0, a.shape[0], c)]


def record(arr, log_chunk):
    return {"n": int(arr.shape[0]), "digest": digest(arr), "chunks": chunk_digests(arr, log_chunk)}


def mismatch(arr, entry, log_chunk):
    """None when arr hashes to the entry, otherwise a message naming the first differing chunks."""
    if arr.shape[0] == entry["n"] and digest(arr) == entry["digest"]:
        return None
    got = chunk_digests(arr, log_chunk)
    bad = [i for i, (a, b) in enumerate(zip(got, entry["chunks"])) if a != b]
    return "%d of %d chunks of 2^%d elements differ (n %d, expected %d), first %s" % (
        len(bad), len(entry["chunks"]), log_chunk, arr.shape[0], entry["n"], bad[:16])


def load():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- input recipes ----
def std_domain(m):
    return oracle.standard_basis(m, W), np.zeros(W, dtype=np.uint64)


def general_domain(m):
    """A random m-vector basis and a random shift with all three words nonzero (multi-word subspace elements throughout)."""
    basis, shift = rand_elems(0x2212, m, W), rand_elems(0x2213, 1, W)[0]
    assert shift.all() and basis.all()
    return basis, shift


def transform_input(key, m):
    """(input vector, basis, shift) of a transform case; the IFFT cases take seeded evaluations of their own, not an FFT's output, so that
    a mistake the two transforms share cannot cancel."""
    if key == "add_fft/std0/shift0":                       # config 2 exactly (test_cfg2_full_size_properties's input)
        return (rand_elems(0x2201, 1 << m, W),) + std_domain(m)
    if key == "add_fft/std0/shift_x%d" % m:              # one-word shift x^m past the basis: Aurora's codeword coset
        return rand_elems(0x2202, 1 << m, W), oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)
    if key == "add_fft/general":
        return (rand_elems(0x2211, 1 << m, W),) + general_domain(m)
    if key == "add_ifft/std0/shift0":
        return (rand_elems(0x2221, 1 << m, W),) + std_domain(m)
    if key == "add_ifft/general":
        return (rand_elems(0x2222, 1 << m, W),) + general_domain(m)
    raise KeyError(key)


def fold_chain_input(key, m):
    """(coefficients of degree 2^(m - 2), basis, shift, localization, challenges): config 3's codeword domain and its FRI rounds."""
    basis, shift = std_domain(m)
    loc = oracle.localization_array(FOLD_CHAINS[key], m, RS_EXTRA)
    xs = [rand_elems(0x2230 + i, 1, W)[0] for i in range(len(loc))]
    return rand_elems(0x2203, 1 << (m - RS_EXTRA), W), basis, shift, loc, xs


def snark_args(key):
    """(field name, codeword domain dim, RS extra dimensions, localization, interactive repetitions, query repetitions) from the key."""
    _, field, *nums = key.split("/")
    return (field,) + tuple(int(v) for v in nums)


# ---- the oracle's side (generator only) ----
def oracle_transform(key, m):
    v, basis, shift = transform_input(key, m)
    return oracle.additive_fft(v, basis, shift) if key.startswith("add_fft") else oracle.additive_ifft(v, basis, shift)


def oracle_fold_chain(key, m):
    """The LDE codeword, then the word after every fold."""
    coeffs, basis, shift, loc, xs = fold_chain_input(key, m)
    doms = oracle.fri_domains_additive(basis, shift, loc)
    words = [oracle.additive_fft(coeffs, basis, shift)]
    cb, cs = basis, shift
    for i, eta in enumerate(loc):
        words.append(oracle.fri_fold_additive(words[-1], cb, cs, 1 << eta, xs[i]))
        cb, cs = doms[i]
    return words


def oracle_snark(key):
    import fri_cases
    field, *rest = snark_args(key)
    return oracle.fri_snark_prove(fri_cases.FIELDS[field][0], *rest, SNARK_SEED)


# ---- the library's side (GPU and CPU build) ----
def device_transform(lib, key, m):
    v, basis, shift = transform_input(key, m)
    return lib.additive_FFT(v, basis, shift) if key.startswith("add_fft") else lib.additive_IFFT(v, basis, shift)


def device_fold_chain(ops, key, m, check):
    """The device LDE (DeviceOps.FFT), then DeviceOps.fold round by round; check(step, device word) sees every word."""
    from libiop_amd import domains
    coeffs, basis, shift, loc, xs = fold_chain_input(key, m)
    field = ops.field
    dom = domains.Domain(field, domains.ADDITIVE, basis=basis, shift=shift)
    cw = ops.FFT(ops.upload(coeffs), coeffs.shape[0], dom)
    check(0, cw)
    for i, (eta, (nb, ns)) in enumerate(zip(loc, oracle.fri_domains_additive(basis, shift, loc))):
        cw = ops.fold(cw, dom, 1 << eta, xs[i])
        dom = domains.Domain(field, domains.ADDITIVE, basis=nb, shift=ns)
        check(i + 1, cw)


def device_snarks(lib, torch, device, key):
    """(Python device prover's transcript, native prover's transcript) of the seeded polynomial."""
    import fri_cases
    from libiop_amd import domains, fri, r1cs
    field, *rest = snark_args(key)
    ops = domains.DeviceOps(lib, torch, device, fri_cases.FIELDS[field][1]())
    params = fri.FRISnarkParameters(*rest)
    d_coeffs = ops.upload(r1cs.seeded_elements(ops.field, SNARK_SEED, params.poly_degree_bound))
    mine = fri.fri_snark_prover(ops, params, d_poly_coeffs=d_coeffs).serialize()
    native = lib.fri_snark_prove(0 if field == "gf192" else 1, d_coeffs.data_ptr(), params.poly_degree_bound, *rest)
    return mine, native


def snark_mismatch(data, entry):
    if len(data) == entry["argument_bytes"] and hashlib.blake2b(data, digest_size=32).hexdigest() == entry["transcript_blake2b"]:
        return None
    return "transcript of %d bytes, expected %d, digest differs" % (len(data), entry["argument_bytes"])
