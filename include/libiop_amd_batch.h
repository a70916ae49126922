/* libiop_amd: the batched transforms and the fused re-extension over GF(2^64), GF(2^128) and GF(2^256), included by libiop_amd.h (do not include it alone).
 *
 * One parameterised text declares the four entries of a field, as one kernel text implements them (libiop_amd/csrc/gfx_additive.h, instantiated in
 * gf64.hip, gf128.hip and gf256.hip).  For FIELD = gf64, gf128 and gf256 it declares
 *
 *   iopx_add_ifft_FIELD_batch_dev          `batch` inverse transforms over one domain, vectors back to back (batch * 2^m elements in and out;
 *                                          d_out may be d_evals)
 *   iopx_add_lde_FIELD_batch_dev           `batch` low-degree extensions: host arrays of device pointers, polynomial k with n_coeffs coefficients ->
 *                                          cosets [coset_begin, +coset_count) of its transform at d_outs[k] (as iopx_add_lde_FIELD_dev)
 *   iopx_add_reextend_FIELD_batch_dev      FFT_over_field_subset(IFFT_over_field_subset(evals, H), L) for `batch` vectors back to back,
 *                                          H = span(basis[0..d_dim)) + eval_shift, L = span(basis[0..m)) + shift: the butterflies of H are undone and
 *                                          those of L's cosets applied to the result; the coefficient form is never materialised (the
 *                                          shift-independent halves of the two transforms cancel exactly), the outputs are the same field elements
 *   iopx_add_reextend_lde_FIELD_batch_dev  ... and, in the same call, the codewords of n_polys polynomials of n_coeffs <= 2^d_dim coefficients each
 *                                          (d_outs: the `batch` re-extensions first, then the n_polys codewords)
 *
 * with the arguments, checks and messages of the gf192 entries of those names in libiop_amd.h, at one, two and four words per element: batch in
 * 1..65535, n_polys at most 65535, d_dim <= m <= 40, a non-empty coset range inside the 2^(m - d) cosets.  Every launch of a call covers the whole
 * batch; outputs equal those of the single-vector entries (iopx_add_ifft_FIELD_dev, iopx_add_lde_FIELD_dev) bit for bit.  Element arrays need only
 * the 8-byte alignment of uint64_t: the 128-bit accesses are used when every pointer of a launch, each element of the pointer arrays included, is
 * 16-byte aligned (the profile reports the other form under the kernel's name + "_w64").
 *
 * The Python binding lists these names in libiop_amd.BATCH_SYMBOLS, beside EXPORTED_SYMBOLS and GFX_OPS_SYMBOLS. */
#ifndef LIBIOP_AMD_BATCH_H
#define LIBIOP_AMD_BATCH_H

#define IOPX_DECLARE_ADD_BATCH(FIELD)                                                                                                                          \
    int iopx_add_ifft_##FIELD##_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, const uint64_t *shift, uint64_t *d_out);   \
    int iopx_add_lde_##FIELD##_batch_dev(const uint64_t *const *d_coeffs, size_t n_coeffs, size_t batch, const uint64_t *basis, size_t m,                     \
                                         const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs);                             \
    int iopx_add_reextend_##FIELD##_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, size_t d_dim,                           \
                                              const uint64_t *eval_shift, const uint64_t *shift, size_t coset_begin, size_t coset_count,                      \
                                              uint64_t *const *d_outs);                                                                                        \
    int iopx_add_reextend_lde_##FIELD##_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *const *d_coeffs, size_t n_coeffs, size_t n_polys,    \
                                                  const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift, const uint64_t *shift,           \
                                                  size_t coset_begin, size_t coset_count, uint64_t *const *d_outs);

IOPX_DECLARE_ADD_BATCH(gf64)
IOPX_DECLARE_ADD_BATCH(gf128)
IOPX_DECLARE_ADD_BATCH(gf256)
#undef IOPX_DECLARE_ADD_BATCH

#endif
