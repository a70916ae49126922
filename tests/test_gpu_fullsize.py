"""Correctness at BASELINE.json's full sizes (configs 4 and 5: 2^20-constraint instances, 2^25-point codeword domains) on the
MI355X, through the C ABI: what the stage timings and bench.py run is checked here at the size they run it — sampled values
against the oracle's point formulas (Horner evaluation, single-coset fold, hashlib digests, the LDT combination at a point),
whole-vector identities computed on the device (interpolate o evaluate, re-extension of a folded codeword), and the complete
2^20 Aurora proof accepted by the oracle's independent verifier.  Configs 2 and 3 (the 2^22-point additive FFT, the FRI SNARK of dimension 22)
are pinned whole against digests of the oracle's outputs (tests/fullsize_cases.py)."""
import hashlib

import numpy as np
import pytest

import fullsize_cases as fc
import oracle
from helpers import rand_elems

pytestmark = pytest.mark.gpu
W = 3
M, D = 25, 20                       # codeword domain 2^25, polynomials of 2^20 coefficients (rate 1/32)


@pytest.fixture(scope="module")
def env():
    import torch
    import libiop_amd
    from libiop_amd import domains
    lib = libiop_amd.lib()
    lib.init(0)
    lib.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda:0")
    return lib, torch, dev, domains.DeviceOps(lib, torch, dev, domains.GF192()), domains.DeviceOps(lib, torch, dev, domains.EdwardsFr())


def _sample_positions(n, coset, seed):
    """First / last element of several cosets, the two ends of the vector, positions >= n/2, plus random ones."""
    rng = np.random.default_rng(seed)
    pos = {0, 1, coset - 1, coset, n // 2 - 1, n // 2, n - coset, n - 1, (n // 2) + coset * 5, n - 2 * coset - 1}
    pos.update(int(p) for p in rng.integers(0, n, size=12))
    pos.update(int(c) * coset for c in rng.integers(0, n // coset, size=4))
    return sorted(pos)


def test_lde_2p20_to_2p25_horner(env):
    """additive LDE with Aurora's shift x^25: sampled evaluations equal Horner evaluation of the polynomial at the domain point."""
    lib, torch, dev, ops, _ = env
    field = ops.field
    L = field.domain(1 << M, np.array([1 << M, 0, 0], dtype=np.uint64))
    coeffs = rand_elems(0x2504, 1 << D, W)
    cw = ops.FFT(ops.upload(coeffs), 1 << D, L)
    pos = _sample_positions(1 << M, 1 << D, 1)
    assert max(pos) >= (1 << 24)
    vals = lib.query_responses_dev([cw.data_ptr()], 24, 1 << M, pos)[:, 0, :]
    for p, v in zip(pos, vals):
        point = np.array([p ^ (1 << M), 0, 0], dtype=np.uint64)            # shift + sum of basis bits: all in word 0
        assert np.array_equal(v, oracle.poly_eval(coeffs, point)), p
    # batched extension of four polynomials: equal to four single extensions
    polys = [ops.upload(rand_elems(0x2510 + k, 1 << D, W)) for k in range(3)] + [ops.upload(coeffs)]
    batch = ops.FFT_batch(polys, 1 << D, L)
    assert torch.equal(batch[3], cw)
    single = ops.FFT(polys[1], 1 << D, L)
    assert torch.equal(batch[1], single)
    # interpolation of the systematic part returns the coefficients (IFFT_of_known_degree on the first 2^20 evaluations)
    back = ops.IFFT_of_known_degree(cw, 1 << D, L)
    assert np.array_equal(ops.download(back), coeffs)


def _check_tree(lib, torch, nodes, oracles_host_getter, num_oracles, n, coset, additive, sample_leaves):
    """Sampled leaf digests against hashlib over the reference's serialisation (merkle_tree.tcc:127-134), the root against a
    recomputation from the device's level-8 nodes, sampled inner nodes against their children."""
    L = n // coset
    nodes_h = nodes.cpu().numpy()
    for leaf in sample_leaves:
        cols = []
        for j in range(coset):
            p = leaf * coset + j if additive else leaf + j * L
            cols.append(oracles_host_getter(p))                      # (num_oracles, 3)
        cols = np.stack(cols)                                        # [j][k]
        msg = b"".join(cols[j, k].tobytes() for k in range(num_oracles) for j in range(coset))      # slice[j + k * coset]
        assert hashlib.blake2b(msg, digest_size=32).digest() == bytes(nodes_h[L - 1 + leaf]), leaf
    level = [bytes(nodes_h[(1 << 8) - 1 + i]) for i in range(1 << 8)]
    while len(level) > 1:
        level = [hashlib.blake2b(level[2 * i] + level[2 * i + 1], digest_size=32).digest() for i in range(len(level) // 2)]
    assert level[0] == bytes(nodes_h[0])
    rng = np.random.default_rng(9)
    for j in [0, 1, L - 2, (L - 1) // 2] + [int(v) for v in rng.integers(0, L - 1, size=16)]:
        assert hashlib.blake2b(bytes(nodes_h[2 * j + 1]) + bytes(nodes_h[2 * j + 2]), digest_size=32).digest() == bytes(nodes_h[j]), j


def test_merkle_2p24_leaves_four_oracles(env):
    """cfg4 round 0: 4 oracles x 2^25 elements, cosets of 2 -> 2^24 leaves of 192 bytes."""
    lib, torch, dev, ops, _ = env
    n = 1 << M
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    oracles = [torch.randint(-2**62, 2**62, (n, 3), dtype=torch.int64, device=dev, generator=gen) for _ in range(4)]
    torch.cuda.synchronize()
    tree = ops.merkle_tree(oracles, ops.field.domain(n), 2)
    lib.synchronize()
    get = lambda p: np.stack([o[p].cpu().numpy().view(np.uint64) for o in oracles])
    L = n // 2
    _check_tree(lib, torch, tree.nodes, get, 4, n, 2, True, [0, 1, L // 2, L - 1, 12345678, (1 << 23) + 77])


def test_merkle_2p24_leaves_twelve_oracles_multiplicative(env):
    """cfg5 index round: 12 oracles, multiplicative position map, cosets of 2 -> 2^24 leaves of 576 bytes."""
    lib, torch, dev, _, ops = env
    n = 1 << M
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    oracles = [torch.randint(0, 2**62, (n, 3), dtype=torch.int64, device=dev, generator=gen) for _ in range(12)]
    torch.cuda.synchronize()
    tree = ops.merkle_tree(oracles, ops.field.domain(n), 2)
    lib.synchronize()
    get = lambda p: np.stack([o[p].cpu().numpy().view(np.uint64) for o in oracles])
    L = n // 2
    _check_tree(lib, torch, tree.nodes, get, 12, n, 2, False, [0, 1, L // 2, L - 1, 7654321, (1 << 23) + 5])


def test_fold_chain_2p25(env):
    """FRI folds 2^25 -> 2^24 -> 2^22 of an LDE codeword: sampled cosets against the oracle's single-coset fold
    (fri_aux.tcc:270-303), and the twice-folded codeword is again a codeword of degree < 2^17 over the derived domain
    (interpolating its first 2^17 evaluations and re-extending reproduces all 2^22)."""
    lib, torch, dev, ops, _ = env
    field = ops.field
    L0 = field.domain(1 << M, np.array([1 << M, 0, 0], dtype=np.uint64))
    doms = field.fri_domains(L0, [1, 2], lib)
    f0 = ops.FFT(ops.upload(rand_elems(0x2511, 1 << D, W)), 1 << D, L0)
    x0, x1 = rand_elems(0x2512, 1, W)[0], rand_elems(0x2513, 1, W)[0]
    f1 = ops.fold(f0, doms[0], 2, x0)
    f2 = ops.fold(f1, doms[1], 4, x1)
    for f, g, dom, cs, x in ((f0, f1, doms[0], 2, x0), (f1, f2, doms[1], 4, x1)):
        ncos = dom.size // cs
        for c in [0, 1, ncos // 2, ncos - 1, 3333333 % ncos, (ncos // 2) + 12345]:
            evals = lib.query_responses_dev([f.data_ptr()], 24, dom.size, [c * cs + k for k in range(cs)])[:, 0, :]
            # the coset's first element: shift + sum of the high basis vectors selected by c
            first = np.array(dom.shift, dtype=np.uint64).copy()
            eta = cs.bit_length() - 1
            for k in range(dom.dim - eta):
                if (c >> k) & 1:
                    first ^= dom.basis[eta + k]
            want = oracle.fri_fold_at_coset(evals, dom.basis[:eta], first, x)
            got = lib.query_responses_dev([g.data_ptr()], 24, ncos, [c])[0, 0]
            assert np.array_equal(got, want), (cs, c)
    coeffs = ops.IFFT_of_known_degree(f2, 1 << (D - 3), doms[2])
    again = ops.FFT(coeffs, 1 << (D - 3), doms[2])
    assert torch.equal(again, f2)


def test_multiplicative_fft_2p22_to_2p25_round_trip(env):
    """cfg5's prover transforms: 2^22 coefficients onto the 2^25 coset with shift = the field's generator, back through the strided
    known-degree IFFT (fft.tcc:435-456); sampled evaluations against Horner."""
    lib, torch, dev, _, ops = env
    import libiop_amd as la
    field = ops.field
    L = field.domain(1 << M, la.EDWARDS_FR_GENERATOR)
    ncoef = 1 << 22
    rng = np.random.default_rng(0x2505)
    raw = rng.integers(0, 2**63, size=(ncoef, 3), dtype=np.uint64)
    raw[:, 2] &= np.uint64((1 << 50) - 1)                                   # below p: valid Montgomery representatives
    d_coeffs = ops.upload(raw)
    cw = ops.FFT(d_coeffs, ncoef, L)
    back = ops.IFFT_of_known_degree(cw, ncoef, L)
    assert torch.equal(back, d_coeffs)
    pos = [0, 1, (1 << 24) + 3, (1 << M) - 1, 23456789]
    vals = lib.query_responses_dev([cw.data_ptr()], 24, 1 << M, pos)[:, 0, :]
    g = field.to_int(L.gen)
    for p, v in zip(pos, vals):
        x = field.from_int(L.shift_int * pow(g, p, field.P))
        assert np.array_equal(v, oracle.fp_poly_eval(raw, x)), p


def test_ldt_combination_2p25_sampled(env):
    """combined_LDT_virtual_oracle over 7 oracles of 2^25 elements with Aurora's degrees: sampled positions against the point
    formula sum_i c_i f_i(x) + sum_submaximal c'_i x^(max - deg_i) f_i(x) (ldt_reducer_aux.tcc:133-170)."""
    from libiop_amd import host
    lib, torch, dev, ops, _ = env
    n = 1 << M
    L = ops.field.domain(n, np.array([n, 0, 0], dtype=np.uint64))
    gen = torch.Generator(device=dev)
    gen.manual_seed(6)
    oracles = [torch.randint(-2**62, 2**62, (n, 3), dtype=torch.int64, device=dev, generator=gen) for _ in range(7)]
    degrees = [(1 << D) - 1, (1 << D) - 1, (1 << D) - 16, 1 << D, 1 << D, 1 << D, (1 << D) - 1]       # h, g, fw, fAz, fBz, fCz, rowcheck
    coeffs = rand_elems(0x2514, 14, W)
    out = ops.ldt_combine(oracles, degrees, coeffs, L)
    pos = _sample_positions(n, 1 << D, 2)
    got = lib.query_responses_dev([out.data_ptr()], 24, n, pos)[:, 0, :]
    vals = lib.query_responses_dev([o.data_ptr() for o in oracles], 24, n, pos)
    c = [1] + [host.gf_from_words(w) for w in coeffs]                       # coefficients_ = {1, r...} (ldt_reducer_aux.tcc:34-36)
    submax = [i for i, d in enumerate(degrees) if d < max(degrees)]
    for q, p in enumerate(pos):
        x = p ^ n
        acc = 0
        for i in range(7):
            acc ^= host.gf_mul(c[i], host.gf_from_words(vals[q, i]))
        for s, i in enumerate(submax):
            e, xp, r = max(degrees) - degrees[i], x, 1
            while e:
                if e & 1:
                    r = host.gf_mul(r, xp)
                xp = host.gf_sq(xp)
                e >>= 1
            acc ^= host.gf_mul(host.gf_mul(c[7 + s], r), host.gf_from_words(vals[q, i]))
        assert host.gf_from_words(got[q]) == acc, p


# The 2^20 Aurora proof is pinned by digest equality with the oracle prover's transcript (test_aurora_transcript_equals_the_oracle_provers_at_large_sizes[20],
# native and Python provers); the oracle VERIFIER's run on it (two minutes of one host core for bytes whose equality is already asserted) is made at 2^14
# (test_aurora_2p14_transcript_byte_equal_to_the_oracle_prover: byte equality, acceptance) and with every tampered component at 2^8 - 2^12 (tests/aurora_cases.py).


def test_fractal_2p20_proof_accepted_by_the_oracle_verifier(env):
    """BASELINE config 5 at full size: the Fractal index (twelve 2^25-point oracles, one Merkle tree) and proof of the 2^20-constraint
    instance over the 181-bit field are accepted by the oracle's independent verifier, which holds only the index tree's root; a
    flipped index-oracle answer and a wrong root are rejected."""
    from libiop_amd import fractal, r1cs
    lib, torch, dev, _, ops = env
    n = 1 << D
    cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, 0, n - 1, 0x2205)
    params = fractal.FractalParameters(ops.field, cs)
    assert params.codeword_domain_dim == 25 and params.index_domain_dim == 20 and params.localization_parameters == [1] + [2] * 10
    prover_index, (roots, _) = fractal.fractal_snark_indexer(ops, cs, params)
    roots = [bytes(r) for r in roots]
    transcript = fractal.fractal_snark_prover(ops, prover_index, cs, primary, auxiliary, params)
    data = transcript.serialize()
    assert len(transcript.MT_roots) == 13 and len(transcript.query_positions) == 14
    assert oracle.fractal_verify(oracle.FIELD_EDWARDS, D, 0, 0x2205, data, roots)
    bad_root = bytearray(roots[0]); bad_root[9] ^= 2
    assert not oracle.fractal_verify(oracle.FIELD_EDWARDS, D, 0, 0x2205, data, [bytes(bad_root)])
    transcript.query_responses[0] = transcript.query_responses[0].copy()
    transcript.query_responses[0][3, 6, 1] ^= np.uint64(4)
    assert not oracle.fractal_verify(oracle.FIELD_EDWARDS, D, 0, 0x2205, transcript.serialize(), roots)


def test_fri_snark_cfg3_full_size_accepted_by_the_oracle_verifier(env):
    """BASELINE config 3 at its own size: the FRI-only SNARK for a degree-2^20 polynomial on the 2^22-point
    codeword domain (RS_extra_dimensions 2, localization 2 -> [1, 2 x 9], 10 Merkle trees, 1 interactive and 10 query repetitions:
    profiling/instrument_fri_snark.cpp:84-86,144-148; protocols/fri_iop.tcc:3-101; fri_ldt.tcc:475-548) is proved on the device
    and accepted by the oracle's verifier; a flipped answer, a flipped final-polynomial coefficient and a wrong root are rejected."""
    import copy
    from libiop_amd import fri, r1cs
    lib, torch, dev, ops, _ = env
    dim, rs_extra, loc, interactions, queries, seed = 22, 2, 2, 1, 10, 0x2203
    params = fri.FRISnarkParameters(dim, rs_extra, loc, interactions, queries)
    assert params.poly_degree_bound == 1 << 20 and params.localization_parameters == [1] + [2] * 9
    coeffs = r1cs.seeded_elements(ops.field, seed, params.poly_degree_bound)
    d_coeffs = ops.upload(coeffs)
    transcript = fri.fri_snark_prover(ops, params, d_poly_coeffs=d_coeffs)
    assert len(transcript.MT_roots) == 10
    args = (oracle.FIELD_GF192, dim, rs_extra, loc, interactions, queries)
    assert oracle.fri_snark_verify(*args, transcript.serialize())
    # the native prover (libiop_amd/cpp/fri.hpp behind iopx_fri_snark_prove) at the same size: the same bytes.  Both provers call the same
    # kernels, so this pins nothing against the oracle: test_fri_snark_2p22_equals_the_oracle_prover does (the oracle prover's transcript digest)
    assert lib.fri_snark_prove(0, d_coeffs.data_ptr(), params.poly_degree_bound, dim, rs_extra, loc, interactions, queries) == transcript.serialize()
    t = copy.deepcopy(transcript)
    t.query_responses[1] = t.query_responses[1].copy(); t.query_responses[1][0, 0, 1] ^= np.uint64(1)
    assert not oracle.fri_snark_verify(*args, t.serialize())
    t = copy.deepcopy(transcript)
    t.prover_messages[0] = t.prover_messages[0].copy(); t.prover_messages[0][0, 0] ^= np.uint64(1)
    assert not oracle.fri_snark_verify(*args, t.serialize())
    t = copy.deepcopy(transcript)
    r = bytearray(t.MT_roots[0]); r[5] ^= 1; t.MT_roots[0] = bytes(r)
    assert not oracle.fri_snark_verify(*args, t.serialize())


def _reference_own_entry(protocol, field, log_n):
    import reference_digest_cases as rc
    import json
    import os
    with open(os.path.join(rc.ROOT, "tests", "golden", "reference_over_shim.json")) as f:
        doc = json.load(f)
    return next(e for e in doc["large_entries"] + doc["entries"] if (e["protocol"], e["field"], e["log_n"]) == (protocol, field, log_n))


def test_aurora_2p14_transcript_byte_equal_to_the_references_own_prover(env):
    """the largest case whose verifier run stays in the suite.  The Python device prover's transcript against the digest of what libiop's OWN
    prover produced for the instance (tests/golden/reference_over_shim.json, 49 s of one core in the build container; until round 6 the oracle prover was run here
    instead: 25 s of this test), and the oracle's verifier accepts it."""
    import hashlib
    import aurora_cases
    lib, torch, dev, _, _ = env
    e = _reference_own_entry("aurora", "gf192", 14)
    transcript, _, _ = aurora_cases.device_prove(lib, torch, dev, "gf192", 14, 15, 0x2204, 5, 2)
    mine = transcript.serialize()
    assert len(mine) == e["transcript_bytes"] and hashlib.blake2b(mine, digest_size=32).hexdigest() == e["transcript_blake2b"]
    assert oracle.aurora_verify(oracle.FIELD_GF192, 14, 15, 0x2204, mine, rs_extra=5, localization=2)


def test_fractal_2p14_transcript_byte_equal_to_the_references_own_prover(env):
    import hashlib
    import fractal_cases
    lib, torch, dev, _, _ = env
    e = _reference_own_entry("fractal", "edwards_Fr", 14)
    transcript, (roots, messages), _, _, _ = fractal_cases.device_index_and_prove(lib, torch, dev, "edwards_Fr", 14, 0, 0x2205, 3, 2)
    assert messages == [] and [bytes(r).hex() for r in roots] == e["index_roots"]
    mine = transcript.serialize()
    assert len(mine) == e["transcript_bytes"] and hashlib.blake2b(mine, digest_size=32).hexdigest() == e["transcript_blake2b"]
    assert oracle.fractal_verify(oracle.FIELD_EDWARDS, 14, 0, 0x2205, mine, [bytes(r) for r in roots], rs_extra=3, localization=2)


def test_cpp_prover_transcripts_equal_the_python_provers_at_2p20(env):
    """The C++ prover surface (libiop_amd/cpp/aurora.hpp, tools/cpp/aurora_bench.cpp) derives the same 2^20-constraint instance from
    the seed and must produce the Python prover's transcript (whose acceptance by the oracle verifier is tested above): compared
    through BLAKE2b-256 of the canonical transcript bytes, both fields."""
    import json
    import os
    import subprocess
    from libiop_amd import aurora, build as iopx_build, r1cs
    lib, torch, dev, ops_gf, ops_fr = env
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "cpp", "aurora_bench")
    libpath = iopx_build.build()
    src = os.path.join(root, "tools", "cpp", "aurora_bench.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe, "-L" + os.path.dirname(libpath), "-liop_amd", "-Wl,-rpath," + os.path.dirname(libpath),
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    n = 1 << D
    for ops, flag in ((ops_gf, "gf192"), (ops_fr, "edwards")):
        cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, 15, n - 1, 0x2204)
        params = aurora.AuroraParameters(ops.field, n, n - 1, 15)
        mine = aurora.aurora_snark_prover(ops, cs, primary, auxiliary, params).serialize()
        del cs
        torch.cuda.synchronize()
        r = subprocess.run([exe, "--log-n", str(D), "--steps", "1", "--warmup", "1", "--field", flag], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["argument_bytes"] == len(mine)
        assert out["transcript_blake2b"] == hashlib.blake2b(mine, digest_size=32).hexdigest(), flag
        assert out["pcie_h2d_bytes_per_proof"] + out["pcie_d2h_bytes_per_proof"] < (1 << 20)      # a codeword is 768 MiB


@pytest.mark.parametrize("log_n", [16, 18, 20])
def test_aurora_transcript_equals_the_oracle_provers_at_large_sizes(env, log_n):
    """Byte-equality with the oracle prover AT BASELINE's full size: tests/golden/oracle_aurora_transcript_digests_large.json holds BLAKE2b-256 of
    the oracle prover's transcript for 2^16, 2^18 and 2^20 constraints (42 minutes of one host core for 2^20, tools/cpu_baseline_sizes.py on the GPU
    box); the native device prover's transcript of the same seeded instance must hash to it — and so must the Python prover's at 2^20."""
    import json
    import os
    from libiop_amd import aurora, r1cs
    lib, torch, dev, ops, _ = env
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_aurora_transcript_digests_large.json")) as f:
        want = json.load(f)["digests"][str(log_n)]
    n = 1 << log_n
    inst = lib.aurora_example_instance(0, n, 15, n - 1, 0x2204)
    try:
        t = lib.aurora_prove(inst)
    finally:
        lib.aurora_instance_free(inst)
    assert len(t) == want["argument_bytes"]
    assert hashlib.blake2b(t, digest_size=32).hexdigest() == want["transcript_blake2b"], "native device transcript differs from the oracle prover's"
    if log_n == 20:
        cs, primary, auxiliary = r1cs.generate_r1cs_example(ops, n, 15, n - 1, 0x2204)
        params = aurora.AuroraParameters(ops.field, n, n - 1, 15)
        py = aurora.aurora_snark_prover(ops, cs, primary, auxiliary, params).serialize()
        assert hashlib.blake2b(py, digest_size=32).hexdigest() == want["transcript_blake2b"], "Python device prover's transcript differs from the oracle prover's"


@pytest.mark.parametrize("log_n", [16, 18, 20])
def test_fractal_transcript_equals_the_oracle_provers_at_large_sizes(env, log_n):
    """The native Fractal indexer and prover over the 181-bit field against the oracle's recorded index root and transcript digest
    (tests/golden/oracle_fractal_transcript_digests_large.json: 2^18 costs the oracle 7 minutes and 13 GB, 2^20 — BASELINE configs[4]'s own
    size, what bench.py times as secondary_fractal — 15 minutes and 47 GB)."""
    import json
    import os
    lib, torch, dev, _, _ = env
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_fractal_transcript_digests_large.json")) as f:
        want = json.load(f)["digests"][str(log_n)]
    n = 1 << log_n
    inst = lib.aurora_example_instance(1, n, 0, n - 1, 0x2205)
    try:
        roots = lib.fractal_index(inst)
        t = lib.fractal_prove(inst)
    finally:
        lib.aurora_instance_free(inst)
    assert [r.hex() for r in roots] == want["index_roots"]
    assert len(t) == want["argument_bytes"]
    assert hashlib.blake2b(t, digest_size=32).hexdigest() == want["transcript_blake2b"], "native device transcript differs from the oracle prover's"


# ---- whole-output pins for configs 2 and 3 (tests/fullsize_cases.py; digests of the oracle's outputs in tests/golden/oracle_function_digests_large.json) ----
def _large(key):
    return fc.load()["large"]["entries"][key]


@pytest.mark.parametrize("key", [k.format(m=fc.LARGE_M) for k in fc.TRANSFORMS])
def test_additive_transform_2p22_equals_the_oracle(env, key):
    """Config 2 and its neighbours at 2^22: every output of the device FFT / IFFT (Library.additive_FFT / additive_IFFT, as in
    test_cfg2_full_size_properties) hashes to the oracle's, chunk by chunk."""
    lib = env[0]
    err = fc.mismatch(fc.device_transform(lib, key, fc.LARGE_M), _large(key), fc.LARGE_LOG_CHUNK)
    assert err is None, err


@pytest.mark.parametrize("key", sorted(fc.FOLD_CHAINS))
def test_fri_fold_chain_2p22_equals_the_oracle(env, key):
    """Config 3's codeword (the device LDE of 2^20 coefficients onto 2^22 points), then every FRI round's fold over the derived domains
    (localization 2: fused folds [1, 2 x 9]; localization 4: unfused folds over cosets of 16): every word hashes to the oracle's."""
    lib, torch, dev, ops, _ = env
    want = _large(key)
    steps = [want] + want["folds"]
    seen = []

    def check(i, d_word):
        err = fc.mismatch(ops.download(d_word), steps[i], fc.LARGE_LOG_CHUNK)
        assert err is None, "step %d: %s" % (i, err)
        seen.append(i)

    fc.device_fold_chain(ops, key, fc.LARGE_M, check)
    assert seen == list(range(len(steps)))


@pytest.mark.parametrize("key", [k.format(m=fc.LARGE_M) for k in fc.SNARKS])
def test_fri_snark_2p22_equals_the_oracle_prover(env, key):
    """The FRI SNARK at config 3's size, both fields and localization 4: the Python device prover's and the native prover's transcripts
    both hash to the oracle prover's."""
    lib, torch, dev, _, _ = env
    mine, native = fc.device_snarks(lib, torch, dev, key)
    want = _large(key)
    err = fc.snark_mismatch(mine, want)
    assert err is None, "Python device prover: " + err
    err = fc.snark_mismatch(native, want)
    assert err is None, "native prover: " + err
