/* libiop_amd: what the holographic (Fractal) prover needs over GF(2^64), GF(2^128) and GF(2^256) beyond Aurora's entries, included by libiop_amd.h (do not
 * include it alone).
 *
 * One parameterised text declares the five entries of a field.  For FIELD = gf64, gf128 and gf256 it declares
 *
 *   iopx_FIELD_div_dev                            d_out[j] = d_num[j] / d_den[j] (d_num NULL: 1 / d_den[j]) by batch inversion; a zero denominator yields zero.
 *                                                 The quotient buffer holds the running products on the way: it may not alias an input
 *   iopx_domain_offsets_FIELD_dev                 d_out[j] = point - x_j over span(basis[0..m)) + shift
 *   iopx_vanishing_evals_FIELD_dev                d_out[j] = constant - Z_S(x_j), S = span(vanishing_basis) + vanishing_shift
 *   iopx_rational_combine_FIELD_dev               N = sum_i c_i N_i prod_{k != i} D_k, D = prod_k D_k for 1 <= num_rationals <= 4
 *   iopx_rational_sumcheck_constraint_FIELD_dev   (D (p + eps^-1 mu x^(|K| - 1)) - N) / Z_K over the codeword domain, K = span(basis[0..summation_dim)) +
 *                                                 summation_shift, d_xinv: 1 / x over the codeword domain (with 1 / 0 = 0).  Refused: a summation domain that
 *                                                 is not spanned by a prefix of the codeword domain's basis (or m > 40), a linearly dependent prefix, a
 *                                                 codeword domain that meets K
 *
 * with the arguments, checks, return codes and messages of the gf192 entries of those names in libiop_amd.h (iopx_gf192_div_dev, iopx_domain_offsets_gf192_dev,
 * iopx_vanishing_evals_gf192_dev, iopx_rational_combine_gf192_dev, iopx_rational_sumcheck_constraint_gf192_dev), at one, two and four words per element.
 * Element arrays need only the 8-byte alignment of uint64_t: the 128-bit accesses are used when every pointer of a launch is 16-byte aligned (the profile
 * reports the other form under the kernel's name + "_w64").
 *
 * With them iopx_fractal_index, iopx_fractal_prove and iopx_aurora_instance_warm(..., protocol 1) run over IOPX_FIELD_GF64 (one GPU, BLAKE2b) when the
 * option IOPX_GFX_FRACTAL is non-zero (default 0: refused as before), and over IOPX_FIELD_GF128 and IOPX_FIELD_GF256 when the option
 * IOPX_GFX_FRACTAL_WIDE is non-zero (default 0, looked up per call: refused in the words of before, whatever IOPX_GFX_FRACTAL holds; gf64 is governed by
 * IOPX_GFX_FRACTAL alone).  A communicator, an unsupported security parameter, a codeword domain above the transforms' cap (before any device work) and a
 * proof without an index keep their refusals with either option set.  iopx_rational_combine_FIELD_dev has two forms over an element of several words,
 * one rational after the other with inlined products and a lean one through a single product site (same arguments, refusals, profile row, declared
 * bytes and output bytes); the option IOPX_GFX_RATIONAL_FORM picks one per launch (0: the field's measured choice, 1: inlined, 2: lean).  The
 * Python binding lists these names in libiop_amd.FRACTAL_SYMBOLS, beside EXPORTED_SYMBOLS, GFX_OPS_SYMBOLS, BATCH_SYMBOLS and HEAD_SYMBOLS. */
#ifndef LIBIOP_AMD_FRACTAL_H
#define LIBIOP_AMD_FRACTAL_H

#define IOPX_DECLARE_FRACTAL(FIELD)                                                                                                                            \
    int iopx_##FIELD##_div_dev(const uint64_t *d_num, const uint64_t *d_den, uint64_t *d_out, size_t count);                                                   \
    int iopx_domain_offsets_##FIELD##_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *point, uint64_t *d_out);                     \
    int iopx_vanishing_evals_##FIELD##_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *vanishing_basis, size_t vanishing_dim,     \
                                           const uint64_t *vanishing_shift, const uint64_t *constant, uint64_t *d_out);                                        \
    int iopx_rational_combine_##FIELD##_dev(const void *const *d_numerators, const void *const *d_denominators, size_t num_rationals,                         \
                                            const uint64_t *coefficients, size_t n, uint64_t *d_numerator_out, uint64_t *d_denominator_out);                   \
    int iopx_rational_sumcheck_constraint_##FIELD##_dev(const uint64_t *d_p, const uint64_t *d_N, const uint64_t *d_D, const uint64_t *d_xinv,                \
                                                        const uint64_t *basis, size_t m, const uint64_t *shift, size_t summation_dim,                         \
                                                        const uint64_t *summation_shift, const uint64_t *claimed_sum, uint64_t *d_out);

IOPX_DECLARE_FRACTAL(gf64)
IOPX_DECLARE_FRACTAL(gf128)
IOPX_DECLARE_FRACTAL(gf256)
#undef IOPX_DECLARE_FRACTAL

#endif
