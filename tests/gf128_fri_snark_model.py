"""The FRI-only SNARK prover (BASELINE config 3's shape, quirk F14 read as the oracle reads it: the LDT reducer takes the submitted
codeword itself) for the additive arm, written over the oracle's building blocks and parametrised by the word count of a binary field.

There is no oracle prover over gf128 (oracle.fri_snark_prove knows fields 0, 1 and 3), so this model is what the provers over that field
are compared with.  It is trusted because the same text, run at one and at three words, reproduces oracle.fri_snark_prove byte for byte
(tests/test_gf128_emu.py checks that first); at two words every step below is an oracle call that dispatches on the word count.

Steps, as tests/bn128_fri_snark_model.py takes them over a prime field: coefficients -> oracle.additive_fft onto the unshifted domain of 2^dim
points; round-0 tree (oracle.merkle_build) over cosets of 2^loc[0]; LDT reducer with one instance (one input of maximal degree: the combined
oracle is 1 * f, ldt_reducer_aux.tcc:35-36, 52-66); folds (oracle.fri_fold_additive) over the chain oracle.fri_domains_additive; final
polynomial (oracle.additive_ifft); proof of work; query positions; pruned membership proofs (oracle.membership_proof_indices); serialize()
in the canonical byte form of libiop_amd/cpp/iop.hpp.  Challenges come from oracle.Hashchain."""
import struct

import numpy as np

import oracle

MASK64 = (1 << 64) - 1
ZERO_DIGEST = bytes(32)         # blake2b_hashchain::absorb advances the state without reading its input (quirk F8)


def seeded(words, seed, count):
    """r1cs.seeded_elements' rule at this width: element i is SplitMix64 outputs words * i .. words * i + words - 1, the raw words"""
    out = np.zeros((count, words), dtype=np.uint64)
    for i in range(count):
        for w in range(words):
            z = (seed + (words * i + w + 1) * 0x9E3779B97F4A7C15) & MASK64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
            out[i, w] = z ^ (z >> 31)
    return out


def localization_array(loc, dim, rs_extra):
    return [1] + [loc] * ((dim - rs_extra - 1) // loc)        # fri_ldt.tcc:132-146


def prove(words, dim, rs_extra, loc, interactions, queries, seed=None, coeffs=None):
    """The serialised transcript over the binary field of `words` words.  coeffs: (count, words) uint64, at most 2^(dim - rs_extra) rows;
    default: seeded(words, seed, bound)."""
    bound = 1 << (dim - rs_extra)
    if coeffs is None:
        coeffs = seeded(words, seed, bound)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, words)
    assert coeffs.shape[0] <= bound
    chain = oracle.Hashchain()
    bitlen = oracle.pow_bitlen(dim + 3, 1)                  # default_bcs_params (common_bcs_parameters.tcc:24-25), pow.tcc:21-32
    locs = localization_array(loc, dim, rs_extra)
    nr = len(locs)
    basis, shift = oracle.standard_basis(dim, words), np.zeros(words, dtype=np.uint64)
    domains = [(basis, shift)] + [(b, s) for b, s in oracle.fri_domains_additive(basis, shift, locs)]

    roots, trees, tree_oracles = [], [], []

    def commit(oracles, cs):
        nodes = oracle.merkle_build(oracles, cs)
        trees.append(nodes); tree_oracles.append(oracles); roots.append(nodes[0].tobytes())
        chain.absorb(nodes[0].tobytes())

    # round 0: the codeword; challenges: the reducer's two coefficients, then x_0 per interaction
    f0 = oracle.additive_fft(coeffs, basis, shift)
    commit([f0], 1 << locs[0])
    chain.absorb(ZERO_DIGEST)
    ldt_coefficients = chain.squeeze(2, words)
    xs = [chain.squeeze(1, words)[0] for _ in range(interactions)]
    # coefficients_ = { one, r_0, r_1 } and the single input is of maximal degree: the combined oracle is 1 * f; the two squeezed
    # coefficients only advance the hashchain
    assert ldt_coefficients.shape == (2, words)
    cur = [f0] * interactions
    for i in range(nr):
        if i > 0:
            commit(cur, 1 << locs[i])
            chain.absorb(ZERO_DIGEST)
            xs = [chain.squeeze(1, words)[0] for _ in range(interactions)]
        b, s = domains[i]
        cur = [oracle.fri_fold_additive(cur[j], b, s, 1 << locs[i], xs[j]) for j in range(interactions)]
    final_bound = bound >> sum(locs)
    b, s = domains[nr]
    messages = [oracle.additive_ifft(cur[j], b, s)[:final_bound] for j in range(interactions)]
    chain.absorb(ZERO_DIGEST)                               # the last round: messages only, no tree
    challenge = oracle.blake2b(chain.squeeze(1, words).tobytes())      # squeeze_root_type (blake2b.tcc:105-110)
    pow_answer = oracle.pow_solve_blake2b(challenge, bitlen)[0]

    # query positions (fri_ldt.tcc:400-472, fri_aux.tcc:351-387): one random position per repetition, the whole coset of every round.  Over
    # an affine subspace a coset is contiguous (subspace.tcc:73-91) and its index is the position in the next domain.
    sizes = [1 << (dim - sum(locs[:i])) for i in range(nr)]
    qpos = [set() for _ in range(nr)]
    for _ in range(queries):
        pos = chain.squeeze_query_positions(1, sizes[0])[0]
        for r in range(nr):
            pos >>= locs[r]
            qpos[r].update((pos << locs[r]) + k for k in range(1 << locs[r]))

    out = bytearray()
    u64 = lambda v: out.extend(struct.pack("<Q", v))
    u64(len(messages))
    for m in messages:
        u64(len(m))
        out.extend(np.ascontiguousarray(m, dtype=np.uint64).tobytes())
    u64(len(roots))
    for r in roots:
        out.extend(r)
    for t in range(nr):
        positions = sorted(qpos[t])
        num_leaves = sizes[t] >> locs[t]
        leaves = sorted(set(q >> locs[t] for q in positions))
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
        for k in aux:
            out.extend(trees[t][k].tobytes())
    out.extend(pow_answer)
    return bytes(out)
