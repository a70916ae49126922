"""The Aurora SNARK prover (non-zk, BLAKE2b) for the additive arm in the reference's own schedule, written once over the oracle's
word-dispatching building blocks and parametrised by the word count of a binary field.

There is no oracle prover over gf128 or gf256 (oracle.aurora_prove knows fields 0, 1 and 3), so this model is what the provers over those
fields are compared with.  It is trusted because the same text, run at one and at three words, reproduces oracle.aurora_prove byte for
byte, oracle.aurora_params field by field and oracle.r1cs_example (tests/test_gfx_aurora_emu.py checks that first); at two and four words
every field operation below is an oracle call that dispatches on the word count.  Nothing in this file calls libiop_amd or the emulation
library.

Steps (every virtual oracle over the WHOLE codeword domain: the only schedule of a subspace-only field):
  generate_r1cs_example (r1cs_examples.tcc:23-78, seeded)        example()
  f_w, f_Az, f_Bz, f_Cz (r1cs_rs_iop.tcc:481-615)                 round 0, one tree
  multi_lincheck + sumcheck h (basic_lincheck_aux.tcc:29-144,
  sumcheck.tcc:343-388), row check (rowcheck.tcc:5-88)            round 1, one tree
  LDT instance reducer over all oracles (ldt_reducer_aux.tcc)     virtual, FRI's f_0
  FRI (fri_ldt.tcc:474-548), final polynomials                    rounds 2.., one tree each
  proof of work, query positions, pruned paths, serialize()       the canonical byte form of libiop_amd/cpp/iop.hpp

Oracle calls: additive_fft / additive_ifft, merkle_build, Hashchain, rowcheck_additive, fz_additive, sumcheck_g_additive, lincheck_combine,
ldt_combine_additive, fri_fold_additive, fri_domains_additive, gf_mul, gf_inv, pow_bitlen / pow_solve_blake2b, membership_proof_indices.
The division by a vanishing polynomial and the CSR products are restated here over gf_mul and XOR."""
import math
import struct

import numpy as np

import oracle
from gf128_fri_snark_model import ZERO_DIGEST, localization_array, seeded

PARAM_NAMES = ("codeword_domain_dim", "pow_bits", "query_soundness_error_bits", "interactive_soundness_error_bits", "max_tested_degree_bound",
               "max_constraint_degree_bound", "absolute_proximity_parameter", "multi_lincheck_repetitions", "num_output_LDT_instances",
               "fri_interactive_repetitions", "fri_query_repetitions")


# ---- field helpers over (count, words) uint64 arrays -----------------------------------------------------------------------------
def elem(words, v):
    return np.array([(v >> (64 * k)) & ((1 << 64) - 1) for k in range(words)], dtype=np.uint64)


def scaled(v, c):
    """v[i] * c for one element c"""
    v = np.ascontiguousarray(v, dtype=np.uint64)
    return oracle.gf_mul(v, np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.uint64).reshape(1, -1), v.shape)))


def _mul1(a, b):
    return oracle.gf_mul(a.reshape(1, -1), b.reshape(1, -1))[0]


def subspace_poly(basis):
    """coefficients c_i of prod_{v in span(basis)} (X - v) = sum_i c_i X^(2^i) (vanishing_polynomial.tcc:373-395), and its evaluation"""
    words = basis.shape[1]

    def ev(c, x):
        r = np.zeros(words, dtype=np.uint64)
        for ci in c:
            r = r ^ _mul1(ci, x)
            x = _mul1(x, x)
        return r
    c = [elem(words, 1)]
    for b in basis:
        zb = ev(c, b)
        nxt = [np.zeros(words, dtype=np.uint64) for _ in range(len(c) + 1)]
        for i, ci in enumerate(c):
            nxt[i + 1] = nxt[i + 1] ^ _mul1(ci, ci)
            nxt[i] = nxt[i] ^ _mul1(ci, zb)
        c = nxt
    return c, ev


def div_vanishing(poly, n_coeffs, basis, shift):
    """polynomial_over_vanishing_polynomial(P, Z_S).first for S = span(basis) + shift (vanishing_polynomial.tcc:314-371): with
    Z = X^N + sum_t Z_t X^t, Q_j = P_(j + N) + sum_t Z_t Q_(j + N - t), from the top down in blocks no term reaches into"""
    words, dim = basis.shape[1], basis.shape[0]
    N = 1 << dim
    M = max(n_coeffs - N, 0)
    Q = np.zeros((M, words), dtype=np.uint64)
    if M == 0:
        return Q
    c, ev = subspace_poly(basis)
    assert np.array_equal(c[dim], elem(words, 1))
    terms = [(N - (1 << i), c[i]) for i in range(dim) if c[i].any()]
    const = ev(c, np.asarray(shift, dtype=np.uint64))
    if const.any():
        terms.append((N, const))
    block = min([off for off, _ in terms] + [M])
    hi = M
    while hi > 0:
        lo = max(hi - block, 0)
        blk = poly[N + lo:N + hi].copy()
        for off, coef in terms:
            end = min(hi + off, M)
            if lo + off < end:
                blk[:end - lo - off] ^= scaled(Q[lo + off:end], coef)
        Q[lo:hi] = blk
        hi = lo
    return Q


def powers(base, count):
    """base^i for i < count"""
    words = base.shape[0]
    out = elem(words, 1).reshape(1, words)
    step = base
    while out.shape[0] < count:
        out = np.concatenate([out, scaled(out, step)])
        step = _mul1(step, step)
    return np.ascontiguousarray(out[:count])


def _rows_of(row_ptr):
    rp = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))


def _xor_into(out, index, values):
    """out[index[t]] ^= values[t], repeated indices included"""
    for w in range(out.shape[1]):
        np.bitwise_xor.at(out[:, w], index, values[:, w])


# ---- the instance ------------------------------------------------------------------------------------------------------------------
def example(words, log_n, num_inputs, seed):
    """constraint i: z[i mod m] * z[(i + 7) mod m] = coef_i * z[(2 i + 1) mod m] (r1cs_examples.tcc:23-78) as three CSR triples (row_ptr, col, coeff;
    column 0 is the constant 1) and the assignment z = primary || auxiliary"""
    n = 1 << log_n
    nv = n - 1
    z = seeded(words, seed, nv)
    i = np.arange(n)
    a, b, c = i % nv, (i + 7) % nv, (2 * i + 1) % nv
    ab = oracle.gf_mul(z[a], z[b])
    zc = z[c].copy()
    c_zero = ~zc.any(axis=1)
    zc[c_zero] = elem(words, 1)
    coef = oracle.gf_mul(ab, oracle.gf_inv(zc))              # the constant term carries A B where C's variable is zero
    ones = np.ascontiguousarray(np.broadcast_to(elem(words, 1), (n, words)))
    row_ptr = np.arange(n + 1, dtype=np.uint64)
    matrices = [(row_ptr, (a + 1).astype(np.uint32), ones), (row_ptr, (b + 1).astype(np.uint32), ones),
                (row_ptr, np.where(c_zero, 0, c + 1).astype(np.uint32), coef)]
    return {"matrices": matrices, "z": z, "num_variables": nv, "num_inputs": num_inputs}


# ---- parameters (aurora_snark.tcc:38-101, aurora_iop.tcc:3-186; non-zk, heuristic FRI and LDT-reducer soundness) --------------------
def _repetitions(bits, per):
    return max(1, math.ceil(-bits / per))


def parameters(words, log_constraints, num_variables, rs_extra=5, loc=2, security=128):
    fbits = 64 * words                                            # libff::soundness_log_of_field_size_helper: the extension degree
    cdim, vdim = log_constraints, (num_variables + 1).bit_length() - 1
    sdim = max(cdim, vdim)
    dim = sdim + rs_extra
    pow_bits = cdim + 3
    query_bits, interactive_bits = security + 1 - pow_bits, security + 3
    size = 1 << dim
    max_tested, max_constraint = 1 << sdim, max(2 * (1 << sdim) - 1, 2 * (1 << cdim) - 1)
    assert max_constraint + 1 < size
    proximity = min(size - max_constraint, size - max_tested) - 1
    locs = localization_array(loc, dim, rs_extra)
    return {"codeword_domain_dim": dim, "pow_bits": pow_bits, "query_soundness_error_bits": query_bits, "interactive_soundness_error_bits": interactive_bits,
            "max_tested_degree_bound": max_tested, "max_constraint_degree_bound": max_constraint, "absolute_proximity_parameter": proximity,
            "multi_lincheck_repetitions": _repetitions(interactive_bits, cdim - fbits),
            "num_output_LDT_instances": _repetitions(interactive_bits, dim - fbits),
            "fri_interactive_repetitions": _repetitions(interactive_bits, math.log2((1 << locs[0]) - 1) - fbits),
            "fri_query_repetitions": _repetitions(query_bits, math.log2(1 - proximity / size)),
            "localization_parameters": locs, "constraint_domain_dim": cdim, "variable_domain_dim": vdim, "summation_domain_dim": sdim}


# ---- the prover ------------------------------------------------------------------------------------------------------------------
def prove(words, inst, rs_extra=5, loc=2, stats=None):
    """The serialised transcript over the binary field of `words` words for inst = {"matrices", "z", "num_variables", "num_inputs"}; any
    assignment is proved as it stands."""
    W = words
    matrices, nv, k = inst["matrices"], inst["num_variables"], inst["num_inputs"]
    z = np.ascontiguousarray(inst["z"], dtype=np.uint64).reshape(-1, W)
    assert z.shape[0] == nv
    m = len(matrices[0][0]) - 1
    P = parameters(W, m.bit_length() - 1, nv, rs_extra, loc)
    cdim, vdim, sdim, dim, locs = P["constraint_domain_dim"], P["variable_domain_dim"], P["summation_domain_dim"], P["codeword_domain_dim"], P["localization_parameters"]
    idim = (k + 1).bit_length() - 1
    nC, nV, nS, nI = 1 << cdim, 1 << vdim, 1 << sdim, 1 << idim
    assert m == nC and nv + 1 == nV and k + 1 == nI
    zero = np.zeros(W, dtype=np.uint64)
    basis = oracle.standard_basis(dim, W)
    Lshift = elem(W, 1 << dim)                                    # element_outside_of_subset of the unshifted domain (subspace.tcc:219-227)
    bC, bV, bS, bI = basis[:cdim], basis[:vdim], basis[:sdim], basis[:idim]
    fft_L = lambda coeffs: oracle.additive_fft(coeffs, basis, Lshift)     # noqa: E731
    chain = oracle.Hashchain()
    bitlen = oracle.pow_bitlen(P["pow_bits"], 1)

    roots, trees, tree_oracles = [], [], []

    def commit(oracles, cs):
        nodes = oracle.merkle_build(oracles, cs)
        trees.append(nodes); tree_oracles.append(oracles); roots.append(nodes[0].tobytes())
        chain.absorb(nodes[0].tobytes())
        chain.absorb(ZERO_DIGEST)                                 # the round's prover messages: none

    # ---- round 0: the witness oracles (r1cs_rs_iop.tcc:481-615) ----
    zfull = np.concatenate([elem(W, 1).reshape(1, W), z])
    f1v = oracle.additive_ifft(zfull[:nI], bI, zero)              # interpolates (1, primary) over I
    f1v_V = oracle.additive_fft(f1v, bV, zero)
    fw_prime = oracle.additive_ifft(zfull ^ f1v_V, bV, zero)
    fw = div_vanishing(fw_prime, nV, bI, zero)
    Mz = []
    for row_ptr, col, coeff in matrices:
        v = np.zeros((nC, W), dtype=np.uint64)
        col = np.asarray(col, dtype=np.int64)
        if col.shape[0]:
            _xor_into(v, _rows_of(row_ptr), oracle.gf_mul(np.ascontiguousarray(coeff, dtype=np.uint64).reshape(-1, W), zfull[col]))
        Mz.append(v)
    cw_fw = fft_L(fw)
    cw_Mz = [fft_L(oracle.additive_ifft(v, bC, zero)) for v in Mz]
    commit([cw_fw] + cw_Mz, 1 << locs[0])
    reps = P["multi_lincheck_repetitions"]
    alphas = [chain.squeeze(1, W)[0] for _ in range(reps)]
    r_Mzs = [chain.squeeze(3, W) for _ in range(reps)]
    sum_challenges = [chain.squeeze(1, W)[0] for _ in range(reps)]

    # ---- round 1: lincheck, sumcheck (one h per repetition); the row check is virtual ----
    fz = oracle.fz_additive(cw_fw, fft_L(f1v), basis, Lshift, bI, zero)
    hs, gs = [], []
    lincheck_degree = nS + max(nV, nC) - 1                        # basic_lincheck.tcc:151-154 (the degrees as registered, r1cs_rs_iop.tcc:285-375)
    for rep in range(reps):
        pw = powers(alphas[rep], nC)
        prime, abc = np.zeros((nS, W), dtype=np.uint64), np.zeros((nS, W), dtype=np.uint64)
        prime[:nC] = pw
        for q, (row_ptr, col, coeff) in enumerate(matrices):      # p_alpha_ABC: column c of M_q lands at summation index c (basic_lincheck_aux.tcc:64-88)
            col = np.asarray(col, dtype=np.int64)
            if col.shape[0]:
                t = oracle.gf_mul(np.ascontiguousarray(coeff, dtype=np.uint64).reshape(-1, W), pw[_rows_of(row_ptr)])
                _xor_into(abc, col, scaled(t, r_Mzs[rep][q]))
        p1 = fft_L(oracle.additive_ifft(prime, bS, zero))
        p2 = fft_L(oracle.additive_ifft(abc, bS, zero))
        lin = oracle.lincheck_combine(fz, cw_Mz, r_Mzs[rep], p1, p2)
        combined_f = scaled(lin, sum_challenges[rep])
        kd = (lincheck_degree - 1).bit_length()                   # IFFT_of_known_degree (fft.tcc:435-456): the head of the domain
        poly = oracle.additive_ifft(combined_f[:1 << kd], basis[:kd], Lshift)
        h = div_vanishing(poly, lincheck_degree, bS, zero)
        cw_h = fft_L(h)
        hs.append(cw_h)
        gs.append(oracle.sumcheck_g_additive(combined_f, cw_h, basis, Lshift, bS, zero, zero))      # claimed sum 0
    rowcheck = oracle.rowcheck_additive(cw_Mz[0], cw_Mz[1], cw_Mz[2], basis, Lshift, cdim, zero)
    commit(hs, 1 << locs[0])

    # ---- the LDT instance reducer over (h, g per repetition; f_w, f_Az, f_Bz, f_Cz, row check) ----
    ldt_oracles, degrees = [], []
    for rep in range(reps):
        ldt_oracles += [hs[rep], gs[rep]]
        degrees += [lincheck_degree - nS, nS - 1]
    ldt_oracles += [cw_fw] + cw_Mz + [rowcheck]
    degrees += [nV - (k + 1), nC, nC, nC, nC - 1]
    assert max(degrees) <= P["max_tested_degree_bound"]
    num = len(ldt_oracles)
    ldt_coefficients = [chain.squeeze(2 * num, W) for _ in range(P["num_output_LDT_instances"])]
    interactions = P["fri_interactive_repetitions"]
    xs = [chain.squeeze(1, W)[0] for _ in range(interactions)]
    combined = [oracle.ldt_combine_additive(ldt_oracles, degrees, c, basis, Lshift) for c in ldt_coefficients]

    # ---- FRI (fri_ldt.tcc:474-548): [interaction][ldt] ----
    nr = len(locs)
    domains = [(basis, Lshift)] + [(b, s) for b, s in oracle.fri_domains_additive(basis, Lshift, locs)]
    cur = [list(combined) for _ in range(interactions)]
    for i in range(nr):
        if i > 0:
            commit([cur[j][l] for j in range(interactions) for l in range(len(combined))], 1 << locs[i])
            xs = [chain.squeeze(1, W)[0] for _ in range(interactions)]
        b, s = domains[i]
        cur = [[oracle.fri_fold_additive(cur[j][l], b, s, 1 << locs[i], xs[j]) for l in range(len(combined))] for j in range(interactions)]
    final_bound = P["max_tested_degree_bound"] >> sum(locs)
    b, s = domains[nr]
    messages = [oracle.additive_ifft(cur[j][l], b, s)[:final_bound] for j in range(interactions) for l in range(len(combined))]
    chain.absorb(ZERO_DIGEST)                                     # the last round: messages only, no tree
    challenge = oracle.blake2b(chain.squeeze(1, W).tobytes())     # squeeze_root_type (blake2b.tcc:105-110)
    pow_answer = oracle.pow_solve_blake2b(challenge, bitlen)[0]

    # ---- queries (fri_ldt.tcc:400-472): round 0's positions reach the trees of rounds 0 and 1 through the virtual f_0.  Over an affine
    # subspace a coset is contiguous (subspace.tcc:73-91) and its index is the position in the next domain ----
    sizes = [1 << (dim - sum(locs[:i])) for i in range(nr)]
    qpos = [set() for _ in range(nr)]
    for _ in range(P["fri_query_repetitions"]):
        pos = chain.squeeze_query_positions(1, sizes[0])[0]
        for r in range(nr):
            pos >>= locs[r]
            qpos[r].update((pos << locs[r]) + t for t in range(1 << locs[r]))
    tree_positions = [qpos[0], qpos[0]] + qpos[1:]
    tree_round = [0, 0] + list(range(1, nr))

    out = bytearray()
    u64 = lambda v: out.extend(struct.pack("<Q", v))      # noqa: E731
    u64(len(messages))
    for msg in messages:
        u64(len(msg))
        out.extend(np.ascontiguousarray(msg, dtype=np.uint64).tobytes())
    u64(len(roots))
    for r in roots:
        out.extend(r)
    for t in range(len(trees)):
        r = tree_round[t]
        positions = sorted(tree_positions[t])
        num_leaves = sizes[r] >> locs[r]
        leaves = sorted(set(q >> locs[r] for q in positions))
        u64(len(positions))
        for q in positions:
            u64(q)
        u64(len(leaves))
        for q in leaves:
            u64(q)
        u64(len(tree_oracles[t]) if positions else 0)
        for q in positions:
            for o in tree_oracles[t]:
                out.extend(o[q].tobytes())
        aux = oracle.membership_proof_indices(num_leaves, leaves)
        u64(len(aux))
        for a in aux:
            out.extend(trees[t][a].tobytes())
    out.extend(pow_answer)
    if stats is not None:
        stats["num_trees"] = len(trees)
        stats["parameters"] = P
    return bytes(out)


def prove_example(words, log_n, num_inputs, seed, rs_extra=5, loc=2, stats=None):
    """(transcript, parameters, instance) of the seeded instance"""
    inst = example(words, log_n, num_inputs, seed)
    st = {} if stats is None else stats
    t = prove(words, inst, rs_extra, loc, st)
    return t, st["parameters"], inst
