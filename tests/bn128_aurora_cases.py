"""Aurora over alt_bn128 Fr: what the CPU-emulation and the GPU suites share.  The native prover (iopx_aurora_prove / iopx_aurora_prove_hashed on
an instance of field 2) against tests/golden/bn128_aurora.json, which tests/golden/make_bn128_aurora.py writes from the Python-integer model
(tests/bn128_aurora_model.py); and the windowed forward transform (iopx_mul_fft_bn128_windows_dev) against the plain entry, the strided
gather of its own output and, at the smallest size, the integer NTT.  Nothing here needs the oracle: the GPU suite reads committed fixtures only."""
import hashlib
import json
import os

import numpy as np

from bn128_fri_snark_cases import BN128_R, FIELD_ALT_BN128_FR, HASHES, mont_words, rand_words, roots_read_at_round_end      # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bn128_aurora.json")

SEED = 0x2204                                               # as tests/test_aurora_emu.py
TUPLES = [(5, 3, 2, 1), (6, 0, 3, 2), (7, 7, 2, 3)]         # (log_n, inputs, rs_extra, loc)
GPU_TUPLE = (10, 3, 2, 2)                                   # codeword domain 2^12: two-pass transforms, leaf grids beyond one workgroup
GPU_HASHES = ("blake2b", "poseidon_starkware")


def key(tup, hash_name):
    return "_".join(str(v) for v in tup) + "/" + hash_name


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def num_trees(tup):
    """the witness round, the sumcheck round, one per FRI round after the first (localization array [1, loc, loc, ...], fri_ldt.tcc:132-146)"""
    return 2 + (tup[0] - 1) // tup[3]


def digest(transcript):
    return {"bytes": len(transcript), "blake2b": hashlib.blake2b(transcript, digest_size=32).hexdigest()}


class options:
    """iopx_set_option for the duration of a block"""

    def __init__(self, lib, **values):
        self.lib, self.values = lib, values

    def __enter__(self):
        for k, v in self.values.items():
            self.lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.lib.clear_option(k)


def native_prove(lib, tup, hash_name, head_eval=1, windows=1, through_plain_entry=False):
    log_n, inputs, rs_extra, loc = tup
    inst = lib.aurora_example_instance(FIELD_ALT_BN128_FR, 1 << log_n, inputs, (1 << log_n) - 1, SEED)
    try:
        with options(lib, IOPX_HEAD_EVAL=head_eval, IOPX_BN128_FFT_WINDOWS=windows):
            return lib.aurora_prove(inst, 128, rs_extra, loc, hash=None if through_plain_entry else HASHES[hash_name])
    finally:
        lib.aurora_instance_free(inst)


def check_digest(lib, fixture, tup, hash_name, **schedule):
    got = native_prove(lib, tup, hash_name, **schedule)
    assert digest(got) == fixture["digests"][key(tup, hash_name)], (tup, hash_name, schedule)
    return got


# ---- the windowed transform -------------------------------------------------------------------------------------------------------
def pass_sizes(lib):
    """the smallest log_n at which the forward transform of 2^log_n coefficients takes one, two and three passes, read from the plan"""
    out = {}
    for log_n in range(1, 29):
        out.setdefault(lib.multiplicative_FFT_pass_count(log_n, 1 << log_n), log_n)
    return out


def integer_fft(coeffs, log_n, shift):
    """the coset transform over Python integers: evaluations at shift * g^i"""
    from bn128_fri_snark_model import ALT_BN128_FR, ntt
    p, a, s = BN128_R, [], 1
    for c in coeffs:
        a.append(c * s % p)
        s = s * shift % p
    return ntt(a + [0] * ((1 << log_n) - len(a)), ALT_BN128_FR.subgroup_generator(log_n), p)


def run_windows(lib, log_n, n_coeffs, windows, shift=5, alias=False, seed=1):
    """(d_out, [window, ...], plain entry's output) as host arrays; windows = [(first, log_stride), ...]; alias: coefficients in the output buffer"""
    n = 1 << log_n
    ints = [int.from_bytes(w.tobytes(), "little") % BN128_R for w in rand_words(seed, n_coeffs)]
    coeffs, sh = mont_words(ints) if n_coeffs else np.zeros((0, 4), dtype=np.uint64), mont_words([shift])[0]
    d_out, d_plain = lib.malloc(32 * n), lib.malloc(32 * n)
    d_coeffs = d_out if alias else lib.malloc(max(32 * n_coeffs, 8))
    d_wins = [lib.malloc(32 * (n >> ls)) for _, ls in windows]
    try:
        for d, (_, ls) in zip(d_wins, windows):                       # poison: a window the call does not fill shows
            lib.h2d(d, np.full((n >> ls, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
        if n_coeffs:
            lib.h2d(d_coeffs, coeffs)
            d_plain_in = lib.malloc(32 * n_coeffs)
            lib.h2d(d_plain_in, coeffs)
            import ctypes
            gen = lib.bn128_subgroup_generator(log_n)
            lib._check(lib.c.iopx_mul_fft_bn128_dev(ctypes.c_void_p(d_plain_in), n_coeffs, log_n, gen.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                    sh.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.c_void_p(d_plain)))
            lib.free(d_plain_in)
        lib.multiplicative_FFT_windows_bn128_dev(d_coeffs, n_coeffs, log_n, sh, d_out, [(f, ls, d) for (f, ls), d in zip(windows, d_wins)])
        out, plain = np.empty((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        lib.d2h(out, d_out)
        if n_coeffs:
            lib.d2h(plain, d_plain)
        wins = []
        for d, (_, ls) in zip(d_wins, windows):
            wins.append(np.empty((n >> ls, 4), dtype=np.uint64))
            lib.d2h(wins[-1], d)
        return out, wins, plain, ints
    finally:
        for d in d_wins + [d_out, d_plain] + ([] if alias else [d_coeffs]):
            lib.free(d)


def check_windows(lib, log_n, n_coeffs, windows, against_integers=False, **kw):
    out, wins, plain, ints = run_windows(lib, log_n, n_coeffs, windows, **kw)
    assert np.array_equal(out, plain), ("output differs from the plain entry's", log_n, n_coeffs, windows)
    for (first, ls), w in zip(windows, wins):
        assert np.array_equal(w, out[first::1 << ls]), ("window is not the strided gather of the output", log_n, n_coeffs, first, ls)
    if against_integers:
        want = integer_fft(ints, log_n, kw.get("shift", 5))
        assert np.array_equal(out, mont_words(want)), ("output differs from the integer transform", log_n, n_coeffs)


def window_cases(log_n):
    """(n_coeffs, windows, alias) at one size: one and two windows, first != 0, log_stride 1 and log_n - 2, n_coeffs in {0, 1, n/4, n}, aliasing"""
    n, far = 1 << log_n, log_n - 2
    return [(n, [(0, 1)], False), (n, [(1, 1), (3, far)], False), (n // 4, [((1 << far) - 1, far), (0, 1)], False), (1, [(1, 1), (0, far)], False),
            (0, [(0, 1), (2, far)], False), (n, [(1, far), (1, 1)], True), (n // 4, [(0, far)], True)]
