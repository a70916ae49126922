/* libiop_amd: what head evaluation of the Aurora prover needs over GF(2^64), GF(2^128) and GF(2^256), included by libiop_amd.h (do not include it alone).
 *
 * One parameterised text declares the three entries of a field.  For FIELD = gf64, gf128 and gf256 it declares
 *
 *   iopx_div_by_vanishing_FIELD_dev        d_out[j] = d_in[j] / Z_S(x_j) over span(basis[0..m)) + shift, S = span(basis[0..sub_dim)) + sub_shift: Z_S is
 *                                          constant on the cosets of S, so one product per element with a per-coset inverse table (kept on the device per
 *                                          pair of domains).  d_out may be d_in.  Refused: a null argument, sub_dim > m or m > 40 ("the vanishing set must be
 *                                          spanned by a prefix of the domain's basis"), a domain on which Z_S has a zero ("the domain intersects the
 *                                          vanishing set")
 *   iopx_FIELD_vanishing_host              Z_S(x) and Z_S's linear coefficient for S = span(basis[0..dim)) + shift, host only (no device work); either
 *                                          output may be NULL
 *   iopx_add_reextend2_FIELD_batch_dev     iopx_add_reextend_FIELD_batch_dev (libiop_amd_batch.h) for two groups of vectors over cosets of the same span
 *                                          with different shifts, in one call: each group's butterflies are undone with its own eval_shift, every forward
 *                                          launch runs over all batch_a + batch_b vectors, no phase-1 launch in either direction.  d_outs: group a's
 *                                          codewords, then group b's; bit for bit the outputs of the two one-group calls
 *
 * with the arguments, checks, return codes and messages of the gf192 entries of those names in libiop_amd.h (iopx_div_by_vanishing_gf192_dev,
 * iopx_gf192_vanishing_host, iopx_add_reextend2_gf192_batch_dev), at one, two and four words per element; only the refusal of a domain that meets S is
 * worded for this entry.  Element arrays need only the 8-byte alignment of uint64_t: the 128-bit accesses are used when every pointer of a launch is
 * 16-byte aligned (the profile reports the other form under the kernel's name + "_w64").
 *
 * The native prover takes the head route over these fields when the option IOPX_GFX_HEAD_EVAL is non-zero (default 0; IOPX_HEAD_EVAL still switches it
 * off everywhere).  The Python binding lists these names in libiop_amd.HEAD_SYMBOLS, beside EXPORTED_SYMBOLS, GFX_OPS_SYMBOLS and BATCH_SYMBOLS. */
#ifndef LIBIOP_AMD_HEAD_H
#define LIBIOP_AMD_HEAD_H

#define IOPX_DECLARE_HEAD(FIELD)                                                                                                                               \
    int iopx_div_by_vanishing_##FIELD##_dev(const uint64_t *d_in, const uint64_t *basis, size_t m, const uint64_t *shift, size_t sub_dim,                     \
                                            const uint64_t *sub_shift, uint64_t *d_out);                                                                       \
    int iopx_##FIELD##_vanishing_host(const uint64_t *basis, size_t dim, const uint64_t *shift, const uint64_t *x, uint64_t *value_out,                        \
                                      uint64_t *linear_coefficient_out);                                                                                       \
    int iopx_add_reextend2_##FIELD##_batch_dev(const uint64_t *d_evals_a, size_t batch_a, const uint64_t *eval_shift_a, const uint64_t *d_evals_b,            \
                                               size_t batch_b, const uint64_t *eval_shift_b, const uint64_t *basis, size_t m, size_t d_dim,                   \
                                               const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs);

IOPX_DECLARE_HEAD(gf64)
IOPX_DECLARE_HEAD(gf128)
IOPX_DECLARE_HEAD(gf256)
#undef IOPX_DECLARE_HEAD

#endif
