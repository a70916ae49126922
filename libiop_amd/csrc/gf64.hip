// GF(2^64) on gfx950: additive FFT / IFFT / low-degree extension, FRI fold and domain chain, LDT combination, vector helpers.
//
// The transforms replace additive_FFT / additive_IFFT of the reference (libiop/algebra/fft.tcc:39-124, 126-204) for FieldT = libff::gf64
// (x^64 + x^4 + x^3 + x + 1, one word).  The kernels, the host driver and the bodies of the entries are gfx_additive.h, instantiated here
// for Elem64 (gf64_elem.h): an element is one uint64_t, so these kernels have one access path (no 128-bit instantiation, no k64_*_w64 rows in
// the profile from this file).
//
// A gf64 product is ~0.13k VALU ops (three word products) and an element is 8 bytes: unlike the gf192 transform this one is bound by its
// HBM passes, so the tile is chosen for few of them — 4096 elements (32 KiB of LDS) carry 8 butterfly levels per upper pass and
// 8 + the bit reversal in the last one.  The vector add is gfx_ops.h's (gf64_ops.hip), as for the wider fields.
#include <hip/hip_runtime.h>
#include "gf64_elem.h"
#include "runtime.h"

#include "gfx_additive.h"

namespace iopx {
void clear_gf64_plans() { clear_plans_x<Elem64>(); }
} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_add_lde_gf64_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                          const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *d_out)
{
    return x_add_lde_dev<Elem64>(d_coeffs, n_coeffs, basis, m, shift, coset_begin, coset_count, d_out);
}

int iopx_add_fft_gf64_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                          const uint64_t *shift, uint64_t *d_out)
{
    return x_add_fft_dev<Elem64>(d_coeffs, n_coeffs, basis, m, shift, d_out);
}

int iopx_add_ifft_gf64_dev(const uint64_t *d_evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                           uint64_t *d_out)
{
    return x_add_ifft_dev<Elem64>(d_evals, basis, m, shift, d_out);
}

// the batched and fused forms (include/libiop_amd_batch.h)
int iopx_add_ifft_gf64_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, const uint64_t *shift, uint64_t *d_out)
{
    return x_add_ifft_batch_dev<Elem64>(d_evals, batch, basis, m, shift, d_out);
}

int iopx_add_lde_gf64_batch_dev(const uint64_t *const *d_coeffs, size_t n_coeffs, size_t batch, const uint64_t *basis, size_t m,
                                 const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_lde_batch_dev<Elem64>(d_coeffs, n_coeffs, batch, basis, m, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_reextend_gf64_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift,
                                      const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend_batch_dev<Elem64>(d_evals, batch, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_reextend_lde_gf64_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *const *d_coeffs, size_t n_coeffs, size_t n_polys,
                                          const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift, const uint64_t *shift,
                                          size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend_lde_batch_dev<Elem64>(d_evals, batch, d_coeffs, n_coeffs, n_polys, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}

// the two-group fused re-extension (include/libiop_amd_head.h)
int iopx_add_reextend2_gf64_batch_dev(const uint64_t *d_evals_a, size_t batch_a, const uint64_t *eval_shift_a, const uint64_t *d_evals_b, size_t batch_b,
                                     const uint64_t *eval_shift_b, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *shift,
                                     size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend2_batch_dev<Elem64>(d_evals_a, batch_a, eval_shift_a, d_evals_b, batch_b, eval_shift_b, basis, m, d_dim, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_fft_gf64(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                      const uint64_t *shift, uint64_t *out)
{
    return x_add_fft_host<Elem64>(coeffs, n_coeffs, basis, m, shift, out);
}

int iopx_add_ifft_gf64(const uint64_t *evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                       uint64_t *out)
{
    return x_add_ifft_host<Elem64>(evals, basis, m, shift, out);
}

int iopx_fri_fold_add_gf64_dev(const uint64_t *d_f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                               size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    return x_fri_fold_add_dev<Elem64>(d_f_i, basis, m, shift, coset_size, x_i, d_next);
}

int iopx_fri_fold_add_gf64(const uint64_t *f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                           size_t coset_size, const uint64_t *x_i, uint64_t *next)
{
    return x_fri_fold_add_host<Elem64>(f_i, basis, m, shift, coset_size, x_i, next);
}

int iopx_fri_domains_gf64(const uint64_t *basis, size_t m, const uint64_t *shift, const size_t *localization, size_t num_reductions,
                          uint64_t *out_bases, uint64_t *out_shifts)
{
    return x_fri_domains<Elem64>(basis, m, shift, localization, num_reductions, out_bases, out_shifts);
}

int iopx_ldt_combine_gf64_dev(const void *const *d_oracles, size_t num_oracles, const size_t *degrees,
                              const uint64_t *random_coefficients, const uint64_t *basis, size_t m, const uint64_t *shift,
                              uint64_t *d_out)
{
    return x_ldt_combine_dev<Elem64>(d_oracles, num_oracles, degrees, random_coefficients, basis, m, shift, d_out);
}

int iopx_gf64_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return x_mul_dev<Elem64>(d_a, d_b, d_out, count); }
int iopx_gf64_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count) { return x_inv_dev<Elem64>(d_a, d_out, count); }
int iopx_gf64_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { return x_host_mul<Elem64>(a, b, out); }
int iopx_gf64_inverse_host(const uint64_t *x, uint64_t *out) { return x_inverse_host<Elem64>(x, out); }

} // extern "C"
