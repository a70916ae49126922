/* libiop_amd: the protocol-layer steps of the encoded Aurora prover over GF(2^128) and GF(2^256), included by libiop_amd.h (do not include it alone).
 *
 * One parameterised text declares the nine entries of a field, as one kernel text implements them (libiop_amd/csrc/gfx_ops.h, instantiated in
 * gf128_ops.hip and gf256_ops.hip).  For FIELD = gf128 and gf256 it declares
 *
 *   iopx_FIELD_pow_table_dev          the powers of alpha (basic_lincheck_aux.tcc:37-45)
 *   iopx_lincomb_FIELD_dev            random_linear_combination_oracle (random_linear_combination.tcc:27-57; at most 16 oracles)
 *   iopx_lincomb_affine_FIELD_dev     its affine form (holographic_lincheck_aux.tcc:117-143)
 *   iopx_spmv_FIELD_dev               the CSR products (r1cs.tcc:236-268, basic_lincheck_aux.tcc:64-88)
 *   iopx_lincheck_FIELD_dev           multi_lincheck_virtual_oracle (basic_lincheck_aux.tcc:102-144; at most 8 matrices)
 *   iopx_rowcheck_FIELD_dev           rowcheck_ABC_virtual_oracle (rowcheck.tcc:16-88)
 *   iopx_fz_FIELD_dev                 fz_virtual_oracle (r1cs_rs_iop.tcc:181-222)
 *   iopx_sumcheck_g_FIELD_dev         sumcheck_g_oracle (sumcheck.tcc:58-119; a zero domain element inverts to zero, utils.tcc:79-97)
 *   iopx_poly_div_vanishing_FIELD_dev polynomial_over_vanishing_polynomial(...).first (vanishing_polynomial.tcc:314-371)
 *
 * with the arguments, checks and messages of the gf64 entries of those names in libiop_amd.h, at two and four words per element.  Element arrays
 * need only the 8-byte alignment of uint64_t: a launch whose device pointers are all 16-byte aligned moves an element in 128-bit accesses, any
 * other launch in 64-bit words (the profile reports the latter under the kernel's name + "_w64").  Codeword domains of dimension above 40 are
 * refused.  iopx_FIELD_add_dev, iopx_FIELD_mul_dev and iopx_FIELD_inv_dev of libiop_amd.h are the sums, products and inverses.  Aurora over these
 * fields runs through these entries from the Python prover (libiop_amd.domains.GF128AuroraOps, GF256AuroraOps) and from the native one
 * (IOPX_FIELD_GF128, IOPX_FIELD_GF256); Fractal and a distributed prover are not built (the fused re-extensions: libiop_amd_batch.h; head evaluation, behind an option: libiop_amd_head.h).
 *
 * The Python binding lists these names in libiop_amd.GFX_OPS_SYMBOLS, beside EXPORTED_SYMBOLS for the declarations of libiop_amd.h. */
#ifndef LIBIOP_AMD_GFX_H
#define LIBIOP_AMD_GFX_H

#define IOPX_DECLARE_GFX_OPS(FIELD)                                                                                                                            \
    int iopx_##FIELD##_pow_table_dev(uint64_t *d_out, size_t count, const uint64_t *base, const uint64_t *init);                                              \
    int iopx_lincomb_##FIELD##_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out);                \
    int iopx_lincomb_affine_##FIELD##_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n, \
                                          uint64_t *d_out);                                                                                                    \
    int iopx_spmv_##FIELD##_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,                 \
                                const uint64_t *scale, int accumulate, uint64_t *d_out);                                                                       \
    int iopx_lincheck_##FIELD##_dev(const uint64_t *d_fz, const void *const *d_Mz, size_t num_matrices, const uint64_t *r_Mz,                                  \
                                    const uint64_t *d_p_alpha_prime, const uint64_t *d_p_alpha_ABC, size_t n, uint64_t *d_out);                                \
    int iopx_rowcheck_##FIELD##_dev(const uint64_t *d_Az, const uint64_t *d_Bz, const uint64_t *d_Cz, const uint64_t *basis, size_t m,                         \
                                    const uint64_t *shift, size_t constraint_dim, const uint64_t *constraint_shift, uint64_t *d_out);                          \
    int iopx_fz_##FIELD##_dev(const uint64_t *d_fw, const uint64_t *d_f1v, const uint64_t *basis, size_t m, const uint64_t *shift,                             \
                              const uint64_t *input_basis, size_t input_dim, const uint64_t *input_shift, uint64_t *d_out);                                    \
    int iopx_sumcheck_g_##FIELD##_dev(const uint64_t *d_f, const uint64_t *d_h, const uint64_t *basis, size_t m, const uint64_t *shift,                        \
                                      const uint64_t *summation_basis, size_t summation_dim, const uint64_t *summation_shift,                                  \
                                      const uint64_t *claimed_sum, uint64_t *d_out);                                                                           \
    int iopx_poly_div_vanishing_##FIELD##_dev(const uint64_t *d_poly, size_t n_coeffs, const uint64_t *basis, size_t dim, const uint64_t *shift,               \
                                              uint64_t *d_quotient);

IOPX_DECLARE_GFX_OPS(gf128)
IOPX_DECLARE_GFX_OPS(gf256)
#undef IOPX_DECLARE_GFX_OPS

#endif
