// GF(2^128) on gfx950: additive FFT / IFFT / low-degree extension, FRI fold and domain chain, LDT combination, vector helpers.
//
// The transforms replace additive_FFT / additive_IFFT of the reference (libiop/algebra/fft.tcc:39-124, 126-204) for FieldT = libff::gf128
// (x^128 + x^7 + x^2 + x + 1, two words).  The kernels, the host driver and the bodies of the entries are gfx_additive.h, instantiated here
// for Elem128: an element travels as F::mem, a 16-byte block (one 128-bit access when every pointer of the launch is 16-byte aligned,
// two 64-bit words otherwise: the profile reports the latter as k128_*_w64).
#include <hip/hip_runtime.h>
#include "gf128_elem.h"
#include "runtime.h"

#include "gfx_additive.h"

namespace iopx {
void clear_gf128_plans() { clear_plans_x<Elem128>(); }
} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_add_lde_gf128_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                           const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *d_out)
{
    return x_add_lde_dev<Elem128>(d_coeffs, n_coeffs, basis, m, shift, coset_begin, coset_count, d_out);
}

int iopx_add_fft_gf128_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                           const uint64_t *shift, uint64_t *d_out)
{
    return x_add_fft_dev<Elem128>(d_coeffs, n_coeffs, basis, m, shift, d_out);
}

int iopx_add_ifft_gf128_dev(const uint64_t *d_evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                            uint64_t *d_out)
{
    return x_add_ifft_dev<Elem128>(d_evals, basis, m, shift, d_out);
}

// the batched and fused forms (include/libiop_amd_batch.h)
int iopx_add_ifft_gf128_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, const uint64_t *shift, uint64_t *d_out)
{
    return x_add_ifft_batch_dev<Elem128>(d_evals, batch, basis, m, shift, d_out);
}

int iopx_add_lde_gf128_batch_dev(const uint64_t *const *d_coeffs, size_t n_coeffs, size_t batch, const uint64_t *basis, size_t m,
                                 const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_lde_batch_dev<Elem128>(d_coeffs, n_coeffs, batch, basis, m, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_reextend_gf128_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift,
                                      const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend_batch_dev<Elem128>(d_evals, batch, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_reextend_lde_gf128_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *const *d_coeffs, size_t n_coeffs, size_t n_polys,
                                          const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift, const uint64_t *shift,
                                          size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend_lde_batch_dev<Elem128>(d_evals, batch, d_coeffs, n_coeffs, n_polys, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}

// the two-group fused re-extension (include/libiop_amd_head.h)
int iopx_add_reextend2_gf128_batch_dev(const uint64_t *d_evals_a, size_t batch_a, const uint64_t *eval_shift_a, const uint64_t *d_evals_b, size_t batch_b,
                                     const uint64_t *eval_shift_b, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *shift,
                                     size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend2_batch_dev<Elem128>(d_evals_a, batch_a, eval_shift_a, d_evals_b, batch_b, eval_shift_b, basis, m, d_dim, shift, coset_begin, coset_count, d_outs);
}

int iopx_add_fft_gf128(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                       const uint64_t *shift, uint64_t *out)
{
    return x_add_fft_host<Elem128>(coeffs, n_coeffs, basis, m, shift, out);
}

int iopx_add_ifft_gf128(const uint64_t *evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                        uint64_t *out)
{
    return x_add_ifft_host<Elem128>(evals, basis, m, shift, out);
}

int iopx_fri_fold_add_gf128_dev(const uint64_t *d_f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                                size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    return x_fri_fold_add_dev<Elem128>(d_f_i, basis, m, shift, coset_size, x_i, d_next);
}

int iopx_fri_fold_add_gf128(const uint64_t *f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                            size_t coset_size, const uint64_t *x_i, uint64_t *next)
{
    return x_fri_fold_add_host<Elem128>(f_i, basis, m, shift, coset_size, x_i, next);
}

int iopx_fri_domains_gf128(const uint64_t *basis, size_t m, const uint64_t *shift, const size_t *localization, size_t num_reductions,
                           uint64_t *out_bases, uint64_t *out_shifts)
{
    return x_fri_domains<Elem128>(basis, m, shift, localization, num_reductions, out_bases, out_shifts);
}

int iopx_ldt_combine_gf128_dev(const void *const *d_oracles, size_t num_oracles, const size_t *degrees,
                               const uint64_t *random_coefficients, const uint64_t *basis, size_t m, const uint64_t *shift,
                               uint64_t *d_out)
{
    return x_ldt_combine_dev<Elem128>(d_oracles, num_oracles, degrees, random_coefficients, basis, m, shift, d_out);
}

int iopx_gf128_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return x_mul_dev<Elem128>(d_a, d_b, d_out, count); }
int iopx_gf128_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count) { return x_inv_dev<Elem128>(d_a, d_out, count); }
int iopx_gf128_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { return x_host_mul<Elem128>(a, b, out); }
int iopx_gf128_inverse_host(const uint64_t *x, uint64_t *out) { return x_inverse_host<Elem128>(x, out); }

} // extern "C"
