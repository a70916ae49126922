"""The Fractal preprocessing SNARK (indexer and prover, non-zk, BLAKE2b) for the additive arm in the reference's own schedule, written once over
the oracle's word-dispatching building blocks and parametrised by the word count of a binary field.

There is no oracle prover over gf128 or gf256 (oracle.fractal_prove knows gf64, gf192 and edwards Fr), so this model is what the Fractal provers
over those fields are compared with.  It is trusted because the same text, run at one and at three words, reproduces oracle.fractal_prove and
oracle.fractal_prove_csr byte for byte (index roots and transcript) and oracle.fractal_params field by field
(tests/test_gfx_fractal_wide_emu.py checks that first); at two and four words every field operation below is an oracle call that dispatches on
the word count.  Nothing in this file calls libiop_amd or the emulation library.

Steps (every virtual oracle over the WHOLE codeword domain: the only schedule of a subspace-only field).  K is the index domain, H the matrix
domain (constraints = variables + 1 = |H|), L the shifted codeword domain, all spanned by prefixes of the standard basis:
  fractal_snark_parameters, fractal_iop_parameters (fractal_snark.tcc:63-96, fractal_hiop.tcc:5-150)          params()
  matrix_indexer: row, col, val, row * col per matrix over K, extended to L, one tree (fractal_indexer.tcc:29-156,
  bcs_indexer.tcc:17-77)                                                                                         index()
  f_w, f_Az, f_Bz, f_Cz (r1cs_rs_iop.tcc:481-615)                                                                round 1, one tree
  holographic multi-lincheck: t = p_alpha M per repetition (holographic_lincheck.tcc:381-417, common.tcc:5-38)   round 2, one tree
  single-matrix denominators (holographic_lincheck_aux.tcc:97-169), the rational linear combination
  (rational_linear_combination.tcc:4-212), the rational sumcheck over K with its re-extension, its constraint
  oracle and the boundary constraint on t (rational_sumcheck.tcc:9-274, boundary_constraint.tcc), the batch
  sumcheck over H (sumcheck.tcc:58-119, 343-388), the row check (rowcheck.tcc:16-88)                              round 3, one tree
  LDT instance reducer over the six oracles of every repetition, f_w, f_Az, f_Bz, f_Cz and the row check
  (ldt_reducer_aux.tcc), FRI (fri_ldt.tcc:474-548), proof of work, queries, serialize() without the index's root
  (bcs_prover.tcc:119-134)

Oracle calls: gf_mul, gf_inv, all_subset_sums, additive_fft / additive_ifft, ldt_combine_additive, fri_fold_additive, fri_domains_additive,
merkle_build, Hashchain, pow_bitlen / pow_solve_blake2b, blake2b, membership_proof_indices.  Every virtual oracle is restated here over gf_mul,
gf_inv and XOR.  With check_degrees the model interpolates every oracle it hands to the LDT reducer over L and asserts its claimed degree bound
(DegreeCheckFailed; check_degrees="report" lists the failing oracles in stats["degree_failures"] instead and proves on): over a field without a
verifier that is what tells a satisfied assignment from an unsatisfied one."""
import math
import struct

import numpy as np

import oracle
from gf128_fri_snark_model import ZERO_DIGEST, localization_array
from gfx_aurora_model import _mul1, _rows_of, _xor_into, div_vanishing, elem, example, scaled, subspace_poly  # noqa: F401  (example: re-exported)

PARAM_NAMES = ("codeword_domain_dim", "pow_bits", "query_soundness_error_bits", "interactive_soundness_error_bits", "max_LDT_tested_degree_bound",
               "max_constraint_degree_bound", "absolute_proximity_parameter", "holographic_lincheck_repetitions", "num_output_LDT_instances",
               "fri_interactive_repetitions", "fri_query_repetitions", "index_domain_dim", "matrix_domain_dim")


class DegreeCheckFailed(AssertionError):
    pass


def mul(a, b):
    return oracle.gf_mul(np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64))


def _ceil_log2(n):
    return max(n - 1, 0).bit_length()


def _repetitions(bits, per):
    return max(1, math.ceil(-bits / per))


def _matrices(system):
    return [(np.asarray(rp, dtype=np.int64), np.asarray(col, dtype=np.int64), np.ascontiguousarray(co, dtype=np.uint64)) for rp, col, co in system["matrices"]]


# ---- parameters (fractal_snark.tcc:63-96, fractal_hiop.tcc:5-150; non-zk, heuristic FRI and optimistic-heuristic LDT-reducer soundness) ----
def params(words, cs_shape, security=128, rs_extra=3, loc=2):
    """cs_shape = (constraints, variables, the largest number of non-zero entries of a matrix)"""
    n, nv, max_nonzero = cs_shape
    assert n & (n - 1) == 0, "Fractal requires the number of constraints to be a power of two"
    assert n == nv + 1, "Fractal requires the matrices to be square"
    fbits = 64 * words                                            # libff::soundness_log_of_field_size_helper: the extension degree
    kdim, hdim = _ceil_log2(max_nonzero), _ceil_log2(n)           # fractal_hiop.tcc:28-35
    dim = _ceil_log2(4 << kdim) + rs_extra                        # :38-39
    pow_bits = hdim + 3                                           # fractal_snark.tcc:90-95
    query_bits, interactive_bits = security + 1 - pow_bits, security + 3      # fractal_hiop.tcc:77-78
    locs = localization_array(loc, dim, rs_extra)
    H = 1 << hdim
    max_tested, max_constraint = max(3 * H, H - 1), max(4 * H, 2 * H - 1)     # r1cs_rs_iop.tcc:56-97, holographic, query bound 0
    step = 1 << sum(locs)                                         # next_testable_degree_bound (fri_ldt.tcc:148-163)
    max_ldt = max_tested if max_tested % step == 0 else max_tested - max_tested % step + step
    size = 1 << dim
    assert max_ldt < size and max_constraint < size, "degree bounds exceed the codeword domain"
    proximity = min(size - max_constraint, size - max_ldt) - 1
    return {"codeword_domain_dim": dim, "pow_bits": pow_bits, "query_soundness_error_bits": query_bits, "interactive_soundness_error_bits": interactive_bits,
            "max_LDT_tested_degree_bound": max_ldt, "max_constraint_degree_bound": max_constraint, "absolute_proximity_parameter": proximity,
            "holographic_lincheck_repetitions": _repetitions(interactive_bits, 1 + hdim - fbits),             # holographic_lincheck.tcc:16-36
            "num_output_LDT_instances": _repetitions(interactive_bits, dim - fbits),
            "fri_interactive_repetitions": _repetitions(interactive_bits, math.log2((1 << locs[0]) - 1) - fbits),
            "fri_query_repetitions": _repetitions(query_bits, math.log2(1 - proximity / size)),
            "index_domain_dim": kdim, "matrix_domain_dim": hdim, "localization_parameters": locs, "max_tested_degree_bound": max_tested}


def cs_shape(system):
    return (len(system["matrices"][0][0]) - 1, system["num_variables"], max(int(np.asarray(rp)[-1]) for rp, _, _ in system["matrices"]))


# ---- domains: spans of prefixes of the standard basis; L is shifted by element_outside_of_subset (subspace.tcc:219-227) ----
class _Domains:
    def __init__(self, W, P):
        self.W, self.P = W, P
        self.kdim, self.hdim, self.dim = P["index_domain_dim"], P["matrix_domain_dim"], P["codeword_domain_dim"]
        self.zero = np.zeros(W, dtype=np.uint64)
        self.basis = oracle.standard_basis(self.dim, W)
        self.Lshift = elem(W, 1 << self.dim)
        self.bK, self.bH = self.basis[:self.kdim], self.basis[:self.hdim]
        self.nK, self.nH, self.nL = 1 << self.kdim, 1 << self.hdim, 1 << self.dim
        self.ZH, self.evH = subspace_poly(self.bH)                # Z_H(X) = sum_i ZH[i] X^(2^i): linear, so Z_H over a domain is a subset sum
        self.ZK, self.evK = subspace_poly(self.bK)
        self._xs = None

    def fft_L(self, coeffs):
        return oracle.additive_fft(coeffs, self.basis, self.Lshift)

    def xs(self):
        if self._xs is None:
            self._xs = oracle.all_subset_sums(self.basis, self.Lshift)
        return self._xs

    def over_L(self, Z, ev):
        """a linearised polynomial over the codeword domain: the subset sums of its values on the basis and the shift"""
        return oracle.all_subset_sums(np.stack([ev(Z, b) for b in self.basis]), ev(Z, self.Lshift))

    def reextend(self, evals, basis_prefix):
        return self.fft_L(oracle.additive_ifft(evals, basis_prefix, self.zero))


# ---- matrix_indexer::compute_oracles_over_K (fractal_indexer.tcc:47-121): (row, col, val, row * col) of M' = M^T scaled by 1 / u_H(col, col) ----
def index_over_K(D, matrix):
    row_ptr, col, coeff = matrix
    W = D.W
    nnz = int(row_ptr[-1])
    assert nnz <= D.nK, "index domain smaller than the number of non-zero entries"
    H = oracle.all_subset_sums(D.bH, D.zero)
    rows, cols = H[_rows_of(row_ptr)], H[col]                     # reindex_by_subset is the identity over a subspace (field_subset.tcc:130-142)
    rc = mul(rows, cols) if nnz else np.zeros((0, W), dtype=np.uint64)
    # u_H(c, c) = (DZ_H)(c), the formal derivative of a linearised polynomial: its coefficient of X (vanishing_polynomial.tcc:55-74)
    vals = scaled(coeff.reshape(-1, W), oracle.gf_inv(D.ZH[0].reshape(1, W))[0]) if nnz else rc
    pad = D.nK - nnz
    k0 = oracle.all_subset_sums(D.bK, D.zero)[0]
    fill = lambda v, e: np.ascontiguousarray(np.concatenate([v, np.broadcast_to(e, (pad, W))]))      # noqa: E731
    rows, cols, vals, rc = fill(rows, H[0]), fill(cols, H[0]), fill(vals, D.zero), fill(rc, _mul1(k0, k0))   # :99-119
    return [cols, rows, vals, rc]                                 # "We are dealing with the transpose": row and col change places


def index(words, system, security=128, rs_extra=3, loc=2):
    """(index_state, roots): the twelve index oracles over K and over the codeword domain with their tree, and the tree's root"""
    P = params(words, cs_shape(system), security, rs_extra, loc)
    D = _Domains(words, P)
    over_K = [index_over_K(D, m) for m in _matrices(system)]
    codewords = [D.reextend(v, D.bK) for four in over_K for v in four]        # fractal_indexer.tcc:123-156
    nodes = oracle.merkle_build(codewords, 1 << P["localization_parameters"][0])
    state = {"parameters": P, "over_K": over_K, "codewords": codewords, "nodes": nodes, "setup": (security, rs_extra, loc)}
    return state, [nodes[0].tobytes()]


# ---- the prover ----
def prove(words, index_state, system, assignment=None, check_degrees=False, stats=None):
    """The serialised transcript (without the index's root) over the binary field of `words` words for system = {"matrices", "num_variables",
    "num_inputs"(, "z")} and the assignment z = primary || auxiliary (default: the system's own); any assignment is proved as it stands."""
    W = words
    P = index_state["parameters"]
    D = _Domains(W, P)
    matrices = _matrices(system)
    nv, k = system["num_variables"], system["num_inputs"]
    z = np.ascontiguousarray(system["z"] if assignment is None else assignment, dtype=np.uint64).reshape(-1, W)
    assert z.shape[0] == nv
    locs, dim = P["localization_parameters"], D.dim
    nH, nK, zero, basis, Lshift, bH, bK = D.nH, D.nK, D.zero, D.basis, D.Lshift, D.bH, D.bK
    idim = _ceil_log2(k + 1)
    nI, bI = 1 << idim, basis[:idim]
    assert k + 1 == nI and nv + 1 == nH
    fft_L = D.fft_L
    one = elem(W, 1)
    chain = oracle.Hashchain()
    bitlen = oracle.pow_bitlen(P["pow_bits"], 1)
    cs0 = 1 << locs[0]

    roots, trees, tree_oracles = [], [], []

    def commit(oracles, cs, nodes=None):
        nodes = oracle.merkle_build(oracles, cs) if nodes is None else nodes
        trees.append(nodes); tree_oracles.append(oracles); roots.append(nodes[0].tobytes())
        chain.absorb(nodes[0].tobytes())
        chain.absorb(ZERO_DIGEST)                                 # the round's prover messages: hashed without being read (quirk F8)

    # ---- round 0: the index (bcs_prover.tcc:69-80 takes the trees from the index) ----
    idx_L = index_state["codewords"]
    commit(idx_L, cs0, index_state["nodes"])

    # ---- round 1: the witness oracles (r1cs_rs_iop.tcc:481-615) with constraint = variable = matrix domain ----
    zfull = np.concatenate([one.reshape(1, W), z])
    f1v = oracle.additive_ifft(zfull[:nI], bI, zero)
    fw_prime = oracle.additive_ifft(zfull ^ oracle.additive_fft(f1v, bH, zero), bH, zero)
    fw = div_vanishing(fw_prime, nH, bI, zero)
    Mz = []
    for row_ptr, col, coeff in matrices:
        v = np.zeros((nH, W), dtype=np.uint64)
        if col.shape[0]:
            _xor_into(v, _rows_of(row_ptr), mul(coeff.reshape(-1, W), zfull[col]))
        Mz.append(v)
    cw_fw = fft_L(fw)
    cw_Mz = [D.reextend(v, bH) for v in Mz]
    commit([cw_fw] + cw_Mz, cs0)
    reps = P["holographic_lincheck_repetitions"]
    alphas = [chain.squeeze(1, W)[0] for _ in range(reps)]        # holographic_lincheck.tcc:256-265
    r_Mzs = [chain.squeeze(3, W) for _ in range(reps)]

    # ---- round 2: t = p_alpha M per repetition (:381-417; compute_p_alpha_M, common.tcc:5-38) ----
    H_elems = oracle.all_subset_sums(bH, zero)
    ZH_alpha = [D.evH(D.ZH, a) for a in alphas]
    ts = []
    for rep in range(reps):
        # the unnormalised Lagrange polynomial (Z_H(alpha) - Z_H(y)) / (alpha - y) on H, where Z_H vanishes (lagrange_polynomial.tcc:38-136)
        p_alpha_H = scaled(oracle.gf_inv(H_elems ^ alphas[rep]), ZH_alpha[rep])
        over_H = np.zeros((nH, W), dtype=np.uint64)
        for q, (row_ptr, col, coeff) in enumerate(matrices):
            if col.shape[0]:
                _xor_into(over_H, col, scaled(mul(coeff.reshape(-1, W), p_alpha_H[_rows_of(row_ptr)]), r_Mzs[rep][q]))
        ts.append(D.reextend(over_H, bH))
    commit(ts, cs0)
    betas = [chain.squeeze(1, W)[0] for _ in range(reps)]         # :302-310
    sum_challenges = [chain.squeeze(1, W)[0] for _ in range(reps)]

    # ---- round 3: per repetition the claimed M(alpha, beta), the sumcheck's h over H and the rational sumcheck's re-extension over K ----
    xs = D.xs()
    xs_inv = oracle.gf_inv(xs)
    ZH_L, ZK_L = D.over_L(D.ZH, D.evH), D.over_L(D.ZK, D.evK)
    ZH_L_inv, ZK_L_inv = oracle.gf_inv(ZH_L), oracle.gf_inv(ZK_L)
    x_to_K = xs
    for _ in range(D.kdim):
        x_to_K = mul(x_to_K, x_to_K)
    x_to_K_minus_1 = mul(x_to_K, xs_inv)
    ZI, evI = subspace_poly(bI)
    fz = mul(cw_fw, D.over_L(ZI, evI)) ^ fft_L(f1v)               # fz_virtual_oracle (r1cs_rs_iop.tcc:181-222)
    eps_K_inv = oracle.gf_inv(D.ZK[0].reshape(1, W))[0]
    lincheck_degree = nH + max(nH - (k + 1) + k + 1, nH) - 1      # holographic_lincheck.tcc:146-150 with the degrees of r1cs_rs_iop.tcc:285-375
    single = nK
    numerator_degree = single + 2 * single - 2                    # holographic_lincheck.tcc:213-216, three matrices
    denominator_degree = 3 * single - 2
    constraint_degree = max(numerator_degree, denominator_degree + nK - 1) - nK       # rational_sumcheck.tcc:160-163

    def denominators(four, row_query, col_query):
        """single_matrix_denominator (holographic_lincheck_aux.tcc:117-143): (row - row_query)(col - col_query) from row, col, row * col"""
        const = np.broadcast_to(_mul1(row_query, col_query), four[0].shape)
        return scaled(four[0], col_query) ^ scaled(four[1], row_query) ^ four[3] ^ const

    def rational(Ns, Ds, coef):
        """combined_numerator / combined_denominator (rational_linear_combination.tcc:13-108), term by term"""
        numer = np.zeros_like(Ns[0])
        denom = Ds[0]
        for d in Ds[1:]:
            denom = mul(denom, d)
        for i, nmr in enumerate(Ns):
            cur = scaled(nmr, coef[i])
            for j, d in enumerate(Ds):
                if j != i:
                    cur = mul(cur, d)
            numer = numer ^ cur
        return numer, denom

    messages, hs, ps, per_rep = [], [], [], []
    for rep in range(reps):
        alpha, beta = alphas[rep], betas[rep]
        shift = _mul1(ZH_alpha[rep], D.evH(D.ZH, beta))           # :480-499
        coef = [_mul1(shift, r) for r in r_Mzs[rep]]
        # the denominators' challenge is (row_query, col_query) = (beta, alpha) (:501-513)
        N_K, D_K = rational([four[2] for four in index_state["over_K"]], [denominators(four, beta, alpha) for four in index_state["over_K"]], coef)
        assert D_K.any(axis=1).all(), "batch_inverse: zero denominator"
        coeffs = oracle.additive_ifft(mul(N_K, oracle.gf_inv(D_K)), bK, zero)
        M_value = _mul1(D.ZK[0], coeffs[nK - 1])                   # the sum over K: eps times the top coefficient (rational_sumcheck.tcc:238-244)
        p = fft_L(coeffs[:nK - 1])
        messages.append(M_value.reshape(1, W))
        # the batch sumcheck over H of p(alpha, x) sum_m r_m f_Mz(x) - f_z(x) t(x) (holographic_lincheck_aux.tcc:37-95), claimed sum 0
        p_alpha_L = mul(ZH_L ^ np.broadcast_to(ZH_alpha[rep], ZH_L.shape), oracle.gf_inv(xs ^ alpha))
        combined_Mz = scaled(cw_Mz[0], r_Mzs[rep][0]) ^ scaled(cw_Mz[1], r_Mzs[rep][1]) ^ scaled(cw_Mz[2], r_Mzs[rep][2])
        lin = mul(combined_Mz, p_alpha_L) ^ mul(fz, ts[rep])
        combined_f = scaled(lin, sum_challenges[rep])
        kd = (lincheck_degree - 1).bit_length()                   # IFFT_of_known_degree (fft.tcc:435-456): the head of the domain
        poly = oracle.additive_ifft(combined_f[:1 << kd], basis[:kd], Lshift)
        h = fft_L(div_vanishing(poly, lincheck_degree, bH, zero))
        g = combined_f ^ mul(ZH_L, h)                              # sumcheck_g_oracle with claimed sum 0 (sumcheck.tcc:73-95)
        # over the codeword domain: the boundary constraint on t, the combined rational, the rational sumcheck's constraint oracle
        t_boundary = mul(ts[rep] ^ np.broadcast_to(M_value, ts[rep].shape), oracle.gf_inv(xs ^ beta))         # boundary_constraint.tcc
        fours_L = [idx_L[4 * q:4 * q + 4] for q in range(3)]
        N_L, D_L = rational([four[2] for four in fours_L], [denominators(four, beta, alpha) for four in fours_L], coef)
        shifted_p = p ^ scaled(x_to_K_minus_1, _mul1(eps_K_inv, M_value))                                       # rational_sumcheck.tcc:58-112
        q_oracle = mul(mul(D_L, shifted_p) ^ N_L, ZK_L_inv)
        hs.append(h); ps.append(p)
        per_rep.append([ts[rep], t_boundary, h, g, p, q_oracle])
    commit([o for rep in range(reps) for o in (hs[rep], ps[rep])], cs0)      # registration order: sumcheck_H's h, then sumcheck_K's re-extension (:312-366)

    # ---- the LDT instance reducer (holographic_lincheck.tcc:550-580, r1cs_rs_iop.tcc:650-668) ----
    rowcheck = mul(mul(cw_Mz[0], cw_Mz[1]) ^ cw_Mz[2], ZH_L_inv)
    ldt_oracles, degrees = [], []
    for rep in range(reps):
        ldt_oracles += per_rep[rep]
        degrees += [nH, nH - 1, lincheck_degree - nH, nH - 1, nK - 1, constraint_degree]
    ldt_oracles += [cw_fw] + cw_Mz + [rowcheck]
    degrees += [nH - (k + 1), nH, nH, nH, nH - 1]
    assert max(degrees) <= P["max_LDT_tested_degree_bound"], "One of the oracles is registered with claimed degree greater than the max tested degree bound"
    failed = []
    if check_degrees:
        for i, (o, d) in enumerate(zip(ldt_oracles, degrees)):
            if oracle.additive_ifft(o, basis, Lshift)[d:].any():
                failed.append(i)
    if stats is not None:
        stats.update({"parameters": P, "degrees": degrees, "degree_failures": failed})
    if failed and check_degrees != "report":
        raise DegreeCheckFailed("oracles %s of the LDT reducer exceed their degree bounds %s" % (failed, [degrees[i] for i in failed]))
    num = len(ldt_oracles)
    ldt_coefficients = [chain.squeeze(2 * num, W) for _ in range(P["num_output_LDT_instances"])]
    interactions = P["fri_interactive_repetitions"]
    fri_xs = [chain.squeeze(1, W)[0] for _ in range(interactions)]
    combined = [oracle.ldt_combine_additive(ldt_oracles, degrees, c, basis, Lshift) for c in ldt_coefficients]

    # ---- FRI (fri_ldt.tcc:474-548): [interaction][ldt] ----
    nr = len(locs)
    domains = [(basis, Lshift)] + [(b, s) for b, s in oracle.fri_domains_additive(basis, Lshift, locs)]
    cur = [list(combined) for _ in range(interactions)]
    for i in range(nr):
        if i > 0:
            commit([cur[j][l] for j in range(interactions) for l in range(len(combined))], 1 << locs[i])
            fri_xs = [chain.squeeze(1, W)[0] for _ in range(interactions)]
        b, s = domains[i]
        cur = [[oracle.fri_fold_additive(cur[j][l], b, s, 1 << locs[i], fri_xs[j]) for l in range(len(combined))] for j in range(interactions)]
    final_bound = P["max_LDT_tested_degree_bound"] >> sum(locs)
    b, s = domains[nr]
    messages += [oracle.additive_ifft(cur[j][l], b, s)[:final_bound] for j in range(interactions) for l in range(len(combined))]
    chain.absorb(ZERO_DIGEST)                                     # the last round: messages only, no tree
    challenge = oracle.blake2b(chain.squeeze(1, W).tobytes())     # squeeze_root_type (blake2b.tcc:105-110)
    pow_answer = oracle.pow_solve_blake2b(challenge, bitlen)[0]

    # ---- queries (fri_ldt.tcc:400-472): round 0's positions reach the trees of the index and of rounds 1 to 3 through the virtual f_0 ----
    sizes = [1 << (dim - sum(locs[:i])) for i in range(nr)]
    qpos = [set() for _ in range(nr)]
    for _ in range(P["fri_query_repetitions"]):
        pos = chain.squeeze_query_positions(1, sizes[0])[0]
        for r in range(nr):
            pos >>= locs[r]
            qpos[r].update((pos << locs[r]) + t for t in range(1 << locs[r]))
    tree_positions = [qpos[0]] * 4 + qpos[1:]
    tree_round = [0] * 4 + list(range(1, nr))

    out = bytearray()
    u64 = lambda v: out.extend(struct.pack("<Q", v))      # noqa: E731
    u64(len(messages))
    for msg in messages:
        u64(len(msg))
        out.extend(np.ascontiguousarray(msg, dtype=np.uint64).tobytes())
    u64(len(roots) - 1)                                           # remove_index_info_from_transcript (bcs_prover.tcc:119-134): the index's root is the verifier's
    for r in roots[1:]:
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
    return bytes(out)


def index_and_prove(words, system, assignment=None, security=128, rs_extra=3, loc=2, check_degrees=False, stats=None):
    """(transcript, index roots) of a CSR system {"matrices", "num_variables", "num_inputs", "z"}"""
    state, roots = index(words, system, security, rs_extra, loc)
    return prove(words, state, system, assignment, check_degrees, stats), roots


def prove_example(words, log_n, num_inputs, seed, rs_extra=3, loc=2, check_degrees=False, stats=None):
    """(transcript, index roots, the seeded instance)"""
    inst = example(words, log_n, num_inputs, seed)
    t, roots = index_and_prove(words, inst, None, 128, rs_extra, loc, check_degrees, stats)
    return t, roots, inst
