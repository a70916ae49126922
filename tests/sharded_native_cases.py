"""The native multi-rank paths behind the C ABI (libiop_amd/cpp/dist.hpp, libiop_amd/csrc/fft_add_dist.hip, run_phase1 of fft_add.hip), as
functions of (lib, comm, rank, world, ...) that return plain results: transcript bytes, index roots, communicator statistics, digests of
transform outputs.  Shared by tests/test_distributed_gloo.py (kernels compiled for the CPU, gloo group, host-pointer callbacks) and
tests/gpu_ranks_worker.py (N ranks on ONE MI355X, gloo group, staged callbacks).  The functions that run inside a rank never call the
oracle: the *_expected / *_verdicts functions do, once per shape (cached), wherever the caller wants the comparison made."""
import ctypes
import functools
import hashlib

import numpy as np

W = 3

# (m, kind): "std" standard basis with zero shift, "general" random basis with random shift, "aurora" standard basis with shift 1 << m
FFT_SHAPES = ((6, "std"), (8, "general"), (11, "aurora"))


def digest(arr):
    return hashlib.blake2b(np.ascontiguousarray(arr).tobytes(), digest_size=32).digest()


def _rand_elems(seed, count, words):
    from helpers import rand_elems
    return rand_elems(seed, count, words)


def fft_inputs(m, kind):
    import oracle
    if kind == "std":
        basis, shift = oracle.standard_basis(m, W), np.zeros(W, dtype=np.uint64)
    elif kind == "aurora":
        basis, shift = oracle.standard_basis(m, W), np.array([1 << m, 0, 0], dtype=np.uint64)
    else:
        basis, shift = _rand_elems(70 + m, m, W), _rand_elems(71 + m, 1, W)[0]
    return basis, shift, _rand_elems(72 + m, 1 << m, W), _rand_elems(73 + m, 1 << m, W)


@functools.lru_cache(maxsize=None)
def fft_expected(m, kind):
    """(forward transform of the coefficients, the coefficients, inverse transform of the independent evaluations): whole vectors, from the oracle."""
    import oracle
    basis, shift, coeffs, evals = fft_inputs(m, kind)
    return oracle.additive_fft(coeffs, basis, shift), coeffs, oracle.additive_ifft(evals, basis, shift)


# ---- ONE transform as long as its domain across the ranks (iopx_add_[i]fft_gf192_dist_dev) ----
def native_fft(lib, comm, rank, world, shapes=FFT_SHAPES):
    """{"digests": per shape [forward, inverse of its own output, inverse of independent evaluations] of this rank's block,
    "collectives": issued by those, "refused": for world > 2 [forward refused, inverse refused, comm_stats unchanged] at m = 2 log2(world) - 1}."""
    digests = []
    for m, kind in shapes:
        basis, shift, coeffs, evals = fft_inputs(m, kind)
        per = (1 << m) // world
        lo = rank * per
        d_in, d_out, d_back = lib.malloc(per * 24), lib.malloc(per * 24), lib.malloc(per * 24)
        try:
            one = []
            lib.h2d(d_in, np.ascontiguousarray(coeffs[lo:lo + per]))
            lib.additive_FFT_dist_dev(comm, d_in, basis, shift, d_out)
            got = np.empty((per, W), dtype=np.uint64)
            lib.d2h(got, d_out)
            one.append(digest(got))
            lib.additive_FFT_dist_dev(comm, d_out, basis, shift, d_back, inverse=True)           # back to the coefficients
            lib.d2h(got, d_back)
            one.append(digest(got))
            lib.h2d(d_in, np.ascontiguousarray(evals[lo:lo + per]))                             # independent evaluations against the oracle's IFFT
            lib.additive_FFT_dist_dev(comm, d_in, basis, shift, d_out, inverse=True)
            lib.d2h(got, d_out)
            one.append(digest(got))
            digests.append(one)
        finally:
            for d in (d_in, d_out, d_back):
                lib.free(d)
    before = lib.comm_stats()[0]
    refused = []
    if world > 2:                                        # m = 2 log2(world) - 1: nothing to put in a transpose chunk — refused, no collective issued
        import oracle
        m = 2 * (world.bit_length() - 1) - 1
        per = max(1, (1 << m) // world)
        d_a, d_b = lib.malloc(per * 24), lib.malloc(per * 24)
        for inverse in (False, True):
            try:
                lib.additive_FFT_dist_dev(comm, d_a, oracle.standard_basis(m, W), np.zeros(W, dtype=np.uint64), d_b, inverse=inverse)
                refused.append(False)
            except ValueError:
                refused.append(True)
        lib.free(d_a)
        lib.free(d_b)
        refused.append(lib.comm_stats()[0] == before)
    return {"digests": digests, "collectives": before, "refused": refused}


def native_fft_verdicts(result, rank, world, shapes=FFT_SHAPES):
    """One boolean per check of native_fft, in its order: three per shape (bit-exact with the oracle's slice), then the refusals."""
    ok = []
    for (m, kind), got in zip(shapes, result["digests"]):
        per = (1 << m) // world
        ok += [bytes(g) == digest(full[rank * per:(rank + 1) * per]) for g, full in zip(got, fft_expected(m, kind))]
    assert len(result["digests"]) == len(shapes)
    return ok + [bool(v) for v in result["refused"]]


# ---- the provers distributed over the ranks (iopx_aurora_prove_dist / iopx_fractal_*_dist / iopx_fri_snark_prove with comm=) ----
def native_prove(lib, comm, protocol, field_code, log_n, num_inputs, seed, rs_extra):
    """(transcript bytes, index roots, (collectives, bytes sent) of this proof).  protocol "fri": log_n is the codeword domain's dimension,
    num_inputs the query repetitions, the polynomial the seeded one of degree 2^(log_n - rs_extra)."""
    n = 1 << log_n
    inst = lib.aurora_example_instance(field_code, n, num_inputs, n - 1, seed)
    try:
        lib.comm_stats(reset=True)
        if protocol == "fri":
            from libiop_amd import domains, r1cs
            f = domains.GF192() if field_code == 0 else domains.EdwardsFr()
            coeffs = np.ascontiguousarray(r1cs.seeded_elements(f, seed, 1 << (log_n - rs_extra)), dtype=np.uint64)
            d = lib.malloc(coeffs.nbytes)
            lib.h2d(d, coeffs)
            t = lib.fri_snark_prove(field_code, d, coeffs.shape[0], log_n, rs_extra, 2, 1, num_inputs, comm=comm)
            lib.free(d)
            roots = []
        elif protocol == "aurora":
            t = lib.aurora_prove_dist(inst, comm, 128, rs_extra, 2)
            roots = []
        else:
            roots = lib.fractal_index_dist(inst, comm, 128, rs_extra, 2)
            t = lib.fractal_prove_dist(inst, comm, 128, rs_extra, 2)
        return t, roots, lib.comm_stats()
    finally:
        lib.aurora_instance_free(inst)


@functools.lru_cache(maxsize=None)
def prove_expected(protocol, field_code, log_n, num_inputs, seed, rs_extra):
    """(transcript, index roots) of the oracle's single-process prover."""
    import oracle
    field = oracle.FIELD_GF192 if field_code == 0 else oracle.FIELD_EDWARDS
    if protocol == "fri":
        return oracle.fri_snark_prove(field, log_n, rs_extra, 2, 1, num_inputs, seed), []
    if protocol == "aurora":
        return oracle.aurora_prove(field, log_n, num_inputs, seed, rs_extra=rs_extra), []
    return oracle.fractal_prove(field, log_n, num_inputs, seed)


def bad_witness_instance(lib, field_code, log_n, k, seed, device=None):
    """The seeded constraint system with one auxiliary variable changed (Az * Bz != Cz): an instance handle built through iopx_aurora_instance_create."""
    import torch
    import head_cases as hc
    from libiop_amd import domains, r1cs
    field = domains.GF192() if field_code == 0 else domains.EdwardsFr()
    ops = domains.DeviceOps(lib, torch, device if device is not None else torch.device("cpu"), field)
    n = 1 << log_n
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, k, n - 1, seed)
    z = np.concatenate([np.asarray(primary, dtype=np.uint64).reshape(-1, 3), np.asarray(auxiliary, dtype=np.uint64).reshape(-1, 3)])
    z[k + 5] = z[k + 6]
    return lib.aurora_instance(field_code, [hc.csr(ops, M) for M in (cs.A, cs.B, cs.C)], n - 1, k, z)


def bad_witness_prove(lib, comm, field_code, log_n, device=None):
    """(transcript, launches of the whole-domain LDT combination on this rank) of the distributed Aurora prover on the unsatisfied instance."""
    inst = bad_witness_instance(lib, field_code, log_n, 15, 0x2204, device)
    try:
        lib.profile_begin()
        t = lib.aurora_prove_dist(inst, comm, 128, 5, 2)
        prof = lib.profile_report()
        return t, sum(v[0] for k, v in prof.items() if k.startswith("k_ldt_combine"))
    finally:
        lib.aurora_instance_free(inst)


def bad_witness_expected(lib, field_code, log_n, set_option, clear_option, device=None):
    """The single-process prover's bytes by the reference's schedule (IOPX_HEAD_EVAL=0, switched by the caller's two functions)."""
    set_option("IOPX_HEAD_EVAL", "0")
    inst = bad_witness_instance(lib, field_code, log_n, 15, 0x2204, device)
    try:
        return lib.aurora_prove(inst)
    finally:
        lib.aurora_instance_free(inst)
        clear_option("IOPX_HEAD_EVAL")


# ---- phase 1 of the replicated transforms split over the ranks (iopx_comm_bind_transforms; fft_add.hip run_phase1) ----
def phase1_inputs(m, kind):
    import oracle
    basis = oracle.standard_basis(m, W) if kind == "std" else _rand_elems(70 + m, m, W)
    coeffs = _rand_elems(72 + m, 1 << m, W)
    return basis, _rand_elems(71 + m, 1, W)[0], coeffs, coeffs[: (1 << (m - 2)) - 3]          # the short input: phase 1 on 2^(m-2) coefficients


@functools.lru_cache(maxsize=None)
def phase1_expected(m, kind):
    """Digests of (forward transform, coefficients recovered from it, low-degree extension of the short input) from the oracle."""
    import oracle
    basis, shift, coeffs, short = phase1_inputs(m, kind)
    return [digest(oracle.additive_fft(coeffs, basis, shift)), digest(coeffs), digest(oracle.additive_fft(short, basis, shift))]


def _bind(lib, comm):
    lib.c.iopx_comm_bind_transforms.argtypes = [ctypes.c_void_p]
    lib._check(lib.c.iopx_comm_bind_transforms(comm))


def phase1_split(lib, comm, shapes, against_unbound=False):
    """additive_FFT, additive_IFFT and a short-input extension with the communicator bound for transforms, per shape (m, kind):
    {"digests": [forward, inverse, extension], "collectives": [issued by each of the three]}.  The inverse's input is the forward
    result of the UNBOUND transform of the same library; against_unbound: the expected digests are the unbound transforms' own
    (sizes at which the single-GPU transform is pinned elsewhere), returned under "unbound"."""
    out = []
    for m, kind in shapes:
        basis, shift, coeffs, short = phase1_inputs(m, kind)
        full = lib.additive_FFT(coeffs, basis, shift)
        one = {"digests": [], "collectives": []}
        if against_unbound:
            one["unbound"] = [digest(full), digest(lib.additive_IFFT(full, basis, shift)), digest(lib.additive_FFT(short, basis, shift))]
        _bind(lib, comm)
        try:
            for fn, arg in ((lib.additive_FFT, coeffs), (lib.additive_IFFT, full), (lib.additive_FFT, short)):
                lib.comm_stats(reset=True)
                one["digests"].append(digest(fn(arg, basis, shift)))
                one["collectives"].append(lib.comm_stats()[0])
        finally:
            _bind(lib, None)
        out.append(one)
    return out


def phase1_min_m(world):
    """The smallest m at which, with the default tile geometry and IOPX_P1_SHARD_MIN_D lowered to it or below, the three transforms of
    phase1_split all split.  run_phase1 splits a 2^d-coefficient phase 1 over 2^r ranks when every level below r has passes of its own in
    phase1_schedule(d): with 2^10-element tiles and a 2^11-element last tile the last pass starts at level d - 11, so d >= 11 + r; the short
    input has d = m - 2."""
    return 13 + (world.bit_length() - 1)
