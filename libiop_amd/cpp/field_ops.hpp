// Field dispatch for the C++ layer: the ONE place in libiop_amd/cpp/ that names a per-field C entry of include/libiop_amd.h (the Poseidon entries
// belong to the hash policy of iop.hpp, the distributed and the purely additive ones have no twin to choose from).  Tables of plain function pointers,
// one instance per field; a slot a field does not have is null, and entry() refuses it instead of reaching another field's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/libiop_amd.h"

namespace libiop_amd {
namespace ops {

// the entries with one signature in every field
struct vector_ops {
    const char *name;
    std::size_t soundness_bits;                  // libff::soundness_log_of_field_size_helper: the extension degree / floor(log2 p)
    bool distributed;                            // vectors over the field's domains may be split over ranks (dist.hpp)
    decltype(&iopx_fp3_host_mul) host_mul; decltype(&iopx_fp3_host_inverse) host_inverse;
    decltype(&iopx_fp3_sub_dev) sub;             // gf192: its addition
    decltype(&iopx_fp3_mul_dev) mul; decltype(&iopx_fp3_inv_dev) inv; decltype(&iopx_fp3_div_dev) div; decltype(&iopx_fp3_pow_table_dev) pow_table;
    decltype(&iopx_lincomb_fp3_dev) lincomb; decltype(&iopx_lincomb_affine_fp3_dev) lincomb_affine; decltype(&iopx_lincheck_fp3_dev) lincheck;
    decltype(&iopx_spmv_fp3_dev) spmv; decltype(&iopx_rational_combine_fp3_dev) rational_combine;
};
// ... and those the two prime fields share: host scalars, coset transforms on host buffers and on the device, the coset-shaped operators
struct prime_field_ops : vector_ops {
    decltype(&iopx_fp3_from_uint) from_uint; decltype(&iopx_fp3_host_add) host_add; decltype(&iopx_fp3_host_sub) host_sub; decltype(&iopx_fp3_host_pow) host_pow;
    decltype(&iopx_fp3_modulus) modulus; decltype(&iopx_fp3_subgroup_generator) subgroup_generator; decltype(&iopx_fp3_multiplicative_generator) multiplicative_generator;
    decltype(&iopx_mul_fft_fp3) mul_fft_host; decltype(&iopx_mul_ifft_fp3) mul_ifft_host; decltype(&iopx_fri_fold_mul_fp3) fri_fold_mul_host;
    decltype(&iopx_mul_fft_fp3_dev) mul_fft; decltype(&iopx_mul_fft_fp3_windows_dev) mul_fft_windows; decltype(&iopx_mul_ifft_fp3_dev) mul_ifft;
    decltype(&iopx_mul_ifft_known_degree_fp3_dev) mul_ifft_known_degree; decltype(&iopx_fri_fold_mul_fp3_dev) fri_fold_mul;
    decltype(&iopx_ldt_combine_fp3_dev) ldt_combine; decltype(&iopx_rowcheck_fp3_dev) rowcheck; decltype(&iopx_fz_fp3_dev) fz; decltype(&iopx_sumcheck_g_fp3_dev) sumcheck_g;
    decltype(&iopx_poly_div_vanishing_fp3_dev) poly_div_vanishing; decltype(&iopx_domain_offsets_fp3_dev) domain_offsets; decltype(&iopx_vanishing_evals_fp3_dev) vanishing_evals;
    decltype(&iopx_rational_sumcheck_constraint_fp3_dev) rational_sumcheck_constraint;
};

// ... and those a binary field has over its affine subspaces: the transforms, the FRI fold and domain chain, the subspace-shaped operators
struct subspace_ops {
    decltype(&iopx_add_fft_gf192_dev) add_fft; decltype(&iopx_add_lde_gf192_dev) add_lde; decltype(&iopx_add_ifft_gf192_dev) add_ifft;
    decltype(&iopx_fri_fold_add_gf192_dev) fri_fold_add; decltype(&iopx_fri_domains_gf192) fri_domains; decltype(&iopx_ldt_combine_gf192_dev) ldt_combine;
    decltype(&iopx_rowcheck_gf192_dev) rowcheck; decltype(&iopx_fz_gf192_dev) fz; decltype(&iopx_sumcheck_g_gf192_dev) sumcheck_g;
    decltype(&iopx_poly_div_vanishing_gf192_dev) poly_div_vanishing; decltype(&iopx_domain_offsets_gf192_dev) domain_offsets;
    decltype(&iopx_vanishing_evals_gf192_dev) vanishing_evals; decltype(&iopx_rational_sumcheck_constraint_gf192_dev) rational_sumcheck_constraint;
    // several vectors over one domain in every launch, and the fused re-extension (IFFT over H, FFT over L, no coefficient form in between)
    decltype(&iopx_add_ifft_gf192_batch_dev) add_ifft_batch; decltype(&iopx_add_lde_gf192_batch_dev) add_lde_batch;
    decltype(&iopx_add_reextend_gf192_batch_dev) add_reextend_batch; decltype(&iopx_add_reextend_lde_gf192_batch_dev) add_reextend_lde_batch;
    // what head evaluation needs: the pointwise division by Z_S, the two-group fused re-extension, Z_S(x) on the host
    decltype(&iopx_div_by_vanishing_gf192_dev) div_by_vanishing; decltype(&iopx_add_reextend2_gf192_batch_dev) add_reextend2_batch;
    decltype(&iopx_gf192_vanishing_host) vanishing_host;
};

// the slots in the order of the declarations above, line for line
inline constexpr vector_ops gf192 = {
    "gf192", 192, true,
    iopx_gf192_host_mul, iopx_gf192_inverse_host,
    iopx_gf192_add_dev, iopx_gf192_mul_dev, iopx_gf192_inv_dev, iopx_gf192_div_dev, iopx_gf192_pow_table_dev,
    iopx_lincomb_gf192_dev, iopx_lincomb_affine_gf192_dev, iopx_lincheck_gf192_dev, iopx_spmv_gf192_dev, iopx_rational_combine_gf192_dev,
};
// libff::gf64: the Aurora and Fractal provers' entries (csrc/gfx_ops.h through gf64_ops.hip; the batch division and the rational combination: include/libiop_amd_fractal.h)
inline constexpr vector_ops gf64 = {
    "gf64", 64, false,
    iopx_gf64_host_mul, iopx_gf64_inverse_host,
    iopx_gf64_add_dev, iopx_gf64_mul_dev, iopx_gf64_inv_dev, iopx_gf64_div_dev, iopx_gf64_pow_table_dev,
    iopx_lincomb_gf64_dev, iopx_lincomb_affine_gf64_dev, iopx_lincheck_gf64_dev, iopx_spmv_gf64_dev, iopx_rational_combine_gf64_dev,
};
// libff::gf128: the vector helpers of csrc/gf128.hip and the Aurora prover's entries (csrc/gf128_ops.hip), as gf64
inline constexpr vector_ops gf128 = {
    "gf128", 128, false,
    iopx_gf128_host_mul, iopx_gf128_inverse_host,
    iopx_gf128_add_dev, iopx_gf128_mul_dev, iopx_gf128_inv_dev, iopx_gf128_div_dev, iopx_gf128_pow_table_dev,
    iopx_lincomb_gf128_dev, iopx_lincomb_affine_gf128_dev, iopx_lincheck_gf128_dev, iopx_spmv_gf128_dev, iopx_rational_combine_gf128_dev,
};
// libff::gf256: the vector helpers of csrc/gf256.hip and the Aurora prover's entries (csrc/gf256_ops.hip); as gf128
inline constexpr vector_ops gf256 = {
    "gf256", 256, false,
    iopx_gf256_host_mul, iopx_gf256_inverse_host,
    iopx_gf256_add_dev, iopx_gf256_mul_dev, iopx_gf256_inv_dev, iopx_gf256_div_dev, iopx_gf256_pow_table_dev,
    iopx_lincomb_gf256_dev, iopx_lincomb_affine_gf256_dev, iopx_lincheck_gf256_dev, iopx_spmv_gf256_dev, iopx_rational_combine_gf256_dev,
};
inline constexpr subspace_ops gf192_subspace = {
    iopx_add_fft_gf192_dev, iopx_add_lde_gf192_dev, iopx_add_ifft_gf192_dev,
    iopx_fri_fold_add_gf192_dev, iopx_fri_domains_gf192, iopx_ldt_combine_gf192_dev,
    iopx_rowcheck_gf192_dev, iopx_fz_gf192_dev, iopx_sumcheck_g_gf192_dev,
    iopx_poly_div_vanishing_gf192_dev, iopx_domain_offsets_gf192_dev,
    iopx_vanishing_evals_gf192_dev, iopx_rational_sumcheck_constraint_gf192_dev,
    iopx_add_ifft_gf192_batch_dev, iopx_add_lde_gf192_batch_dev,
    iopx_add_reextend_gf192_batch_dev, iopx_add_reextend_lde_gf192_batch_dev,
    iopx_div_by_vanishing_gf192_dev, iopx_add_reextend2_gf192_batch_dev,
    iopx_gf192_vanishing_host,
};
inline constexpr subspace_ops gf64_subspace = {
    iopx_add_fft_gf64_dev, iopx_add_lde_gf64_dev, iopx_add_ifft_gf64_dev,
    iopx_fri_fold_add_gf64_dev, iopx_fri_domains_gf64, iopx_ldt_combine_gf64_dev,
    iopx_rowcheck_gf64_dev, iopx_fz_gf64_dev, iopx_sumcheck_g_gf64_dev,
    iopx_poly_div_vanishing_gf64_dev, iopx_domain_offsets_gf64_dev,
    iopx_vanishing_evals_gf64_dev, iopx_rational_sumcheck_constraint_gf64_dev,
    iopx_add_ifft_gf64_batch_dev, iopx_add_lde_gf64_batch_dev,
    iopx_add_reextend_gf64_batch_dev, iopx_add_reextend_lde_gf64_batch_dev,
    iopx_div_by_vanishing_gf64_dev, iopx_add_reextend2_gf64_batch_dev,
    iopx_gf64_vanishing_host,
};
inline constexpr subspace_ops gf128_subspace = {
    iopx_add_fft_gf128_dev, iopx_add_lde_gf128_dev, iopx_add_ifft_gf128_dev,
    iopx_fri_fold_add_gf128_dev, iopx_fri_domains_gf128, iopx_ldt_combine_gf128_dev,
    iopx_rowcheck_gf128_dev, iopx_fz_gf128_dev, iopx_sumcheck_g_gf128_dev,
    iopx_poly_div_vanishing_gf128_dev, iopx_domain_offsets_gf128_dev,
    iopx_vanishing_evals_gf128_dev, iopx_rational_sumcheck_constraint_gf128_dev,
    iopx_add_ifft_gf128_batch_dev, iopx_add_lde_gf128_batch_dev,
    iopx_add_reextend_gf128_batch_dev, iopx_add_reextend_lde_gf128_batch_dev,
    iopx_div_by_vanishing_gf128_dev, iopx_add_reextend2_gf128_batch_dev,
    iopx_gf128_vanishing_host,
};
inline constexpr subspace_ops gf256_subspace = {
    iopx_add_fft_gf256_dev, iopx_add_lde_gf256_dev, iopx_add_ifft_gf256_dev,
    iopx_fri_fold_add_gf256_dev, iopx_fri_domains_gf256, iopx_ldt_combine_gf256_dev,
    iopx_rowcheck_gf256_dev, iopx_fz_gf256_dev, iopx_sumcheck_g_gf256_dev,
    iopx_poly_div_vanishing_gf256_dev, iopx_domain_offsets_gf256_dev,
    iopx_vanishing_evals_gf256_dev, iopx_rational_sumcheck_constraint_gf256_dev,
    iopx_add_ifft_gf256_batch_dev, iopx_add_lde_gf256_batch_dev,
    iopx_add_reextend_gf256_batch_dev, iopx_add_reextend_lde_gf256_batch_dev,
    iopx_div_by_vanishing_gf256_dev, iopx_add_reextend2_gf256_batch_dev,
    iopx_gf256_vanishing_host,
};
inline constexpr prime_field_ops edwards_Fr = {
    { "edwards Fr", 180, true,
      iopx_fp3_host_mul, iopx_fp3_host_inverse,
      iopx_fp3_sub_dev, iopx_fp3_mul_dev, iopx_fp3_inv_dev, iopx_fp3_div_dev, iopx_fp3_pow_table_dev,
      iopx_lincomb_fp3_dev, iopx_lincomb_affine_fp3_dev, iopx_lincheck_fp3_dev, iopx_spmv_fp3_dev, iopx_rational_combine_fp3_dev },
    iopx_fp3_from_uint, iopx_fp3_host_add, iopx_fp3_host_sub, iopx_fp3_host_pow,
    iopx_fp3_modulus, iopx_fp3_subgroup_generator, iopx_fp3_multiplicative_generator,
    iopx_mul_fft_fp3, iopx_mul_ifft_fp3, iopx_fri_fold_mul_fp3,
    iopx_mul_fft_fp3_dev, iopx_mul_fft_fp3_windows_dev, iopx_mul_ifft_fp3_dev,
    iopx_mul_ifft_known_degree_fp3_dev, iopx_fri_fold_mul_fp3_dev,
    iopx_ldt_combine_fp3_dev, iopx_rowcheck_fp3_dev, iopx_fz_fp3_dev, iopx_sumcheck_g_fp3_dev,
    iopx_poly_div_vanishing_fp3_dev, iopx_domain_offsets_fp3_dev, iopx_vanishing_evals_fp3_dev,
    iopx_rational_sumcheck_constraint_fp3_dev,
};
inline constexpr prime_field_ops alt_bn128_Fr = {
    { "alt_bn128 Fr", 253, false,
      iopx_bn128_host_mul, iopx_bn128_host_inverse,
      iopx_bn128_sub_dev, iopx_bn128_mul_dev, iopx_bn128_inv_dev, iopx_bn128_div_dev, iopx_bn128_pow_table_dev,
      iopx_lincomb_bn128_dev, iopx_lincomb_affine_bn128_dev, iopx_lincheck_bn128_dev, iopx_spmv_bn128_dev, iopx_rational_combine_bn128_dev },
    iopx_bn128_from_uint, iopx_bn128_host_add, iopx_bn128_host_sub, iopx_bn128_host_pow,
    iopx_bn128_modulus, iopx_bn128_subgroup_generator, iopx_bn128_multiplicative_generator,
    iopx_mul_fft_bn128, iopx_mul_ifft_bn128, iopx_fri_fold_mul_bn128,
    iopx_mul_fft_bn128_dev, iopx_mul_fft_bn128_windows_dev, iopx_mul_ifft_bn128_dev,
    iopx_mul_ifft_known_degree_bn128_dev, iopx_fri_fold_mul_bn128_dev,
    iopx_ldt_combine_bn128_dev, iopx_rowcheck_bn128_dev, iopx_fz_bn128_dev, iopx_sumcheck_g_bn128_dev,
    iopx_poly_div_vanishing_bn128_dev, iopx_domain_offsets_bn128_dev, iopx_vanishing_evals_bn128_dev,
    iopx_rational_sumcheck_constraint_bn128_dev,
};

// ---- selection ---------------------------------------------------------------------------------------------------------------------
template<std::size_t Bytes, bool Additive> struct field;                   // by field_kind<FieldT> and sizeof(FieldT)
template<const vector_ops *Vec, const subspace_ops *Sub> struct binary_field {
    static constexpr const vector_ops *vec = Vec; static constexpr const subspace_ops *sub = Sub; static constexpr const prime_field_ops *prime = nullptr; static constexpr bool additive = true;
};
template<> struct field<24, true> : binary_field<&gf192, &gf192_subspace> {};
template<> struct field<8, true> : binary_field<&gf64, &gf64_subspace> {};
template<> struct field<16, true> : binary_field<&gf128, &gf128_subspace> {};
template<> struct field<32, true> : binary_field<&gf256, &gf256_subspace> {};
template<> struct field<24, false> { static constexpr const prime_field_ops *vec = &edwards_Fr, *prime = &edwards_Fr; static constexpr const subspace_ops *sub = nullptr; static constexpr bool additive = false; };
template<> struct field<32, false> { static constexpr const prime_field_ops *vec = &alt_bn128_Fr, *prime = &alt_bn128_Fr; static constexpr const subspace_ops *sub = nullptr; static constexpr bool additive = false; };
// by size alone, for reference_binding.hpp (it does not see field_kind): the prime field of that size; the domain's kind tells gf192 from edwards Fr
template<std::size_t Bytes> struct layout;
template<> struct layout<24> : field<24, false> { static constexpr const subspace_ops *sub = &gf192_subspace; static constexpr bool additive = true; };
template<> struct layout<32> : field<32, false> {};

[[noreturn]] inline void missing(const std::string &op, const char *field) { throw std::invalid_argument(op + ": " + field + " has no such entry"); }

// The C entry of one table slot for the selected field F.  A slot the field does not have throws: nothing falls through to another field's entry.
template<class F, typename Fn> inline Fn entry(Fn vector_ops::*slot, const char *op)
{
    if (!(F::vec->*slot)) missing(op, F::vec->name);
    return F::vec->*slot;
}
template<class F, typename Fn> inline Fn entry(Fn prime_field_ops::*slot, const char *op)
{
    const prime_field_ops *P = F::prime;
    if (!P || !(P->*slot)) missing(std::string(op) + " (multiplicative coset)", F::vec->name);
    return P->*slot;
}
template<class F, typename Fn> inline Fn entry(Fn subspace_ops::*slot, const char *op)
{
    const subspace_ops *S = F::sub;
    if (!S) missing(std::string(op) + " (affine subspace)", F::vec->name);
    if (!(S->*slot)) missing(op, F::vec->name);
    return S->*slot;
}

// ---- domain-shaped operations --------------------------------------------------------------------------------------------------------
// A domain as the C entries take it, all host pointers: basis[dim] + shift for a subspace (gen unused), shift * <gen> of order 2^dim for a coset (basis unused)
struct domain { bool additive; const uint64_t *basis, *gen, *shift; std::size_t dim; };

template<class F> inline bool subspace(const domain &D, const char *op)
{
    if (D.additive && !F::additive) missing(std::string(op) + " (affine subspace)", F::vec->name);
    return D.additive;
}

// the transforms over affine subspaces, the FRI fold and the FRI domain chain (the arguments of the C entries)
template<class F> inline int add_fft(const uint64_t *d_coeffs, std::size_t n_coeffs, const uint64_t *basis, std::size_t m, const uint64_t *shift, uint64_t *d_out)
{
    return entry<F>(&subspace_ops::add_fft, "add_fft")(d_coeffs, n_coeffs, basis, m, shift, d_out);
}
template<class F> inline int add_lde(const uint64_t *d_coeffs, std::size_t n_coeffs, const uint64_t *basis, std::size_t m, const uint64_t *shift, std::size_t coset_begin,
                                     std::size_t coset_count, uint64_t *d_out)
{
    return entry<F>(&subspace_ops::add_lde, "add_lde")(d_coeffs, n_coeffs, basis, m, shift, coset_begin, coset_count, d_out);
}
template<class F> inline int add_ifft(const uint64_t *d_evals, const uint64_t *basis, std::size_t m, const uint64_t *shift, uint64_t *d_out)
{
    return entry<F>(&subspace_ops::add_ifft, "add_ifft")(d_evals, basis, m, shift, d_out);
}
template<class F> inline int add_ifft_batch(const uint64_t *d_evals, std::size_t batch, const uint64_t *basis, std::size_t m, const uint64_t *shift, uint64_t *d_out)
{
    return entry<F>(&subspace_ops::add_ifft_batch, "add_ifft_batch")(d_evals, batch, basis, m, shift, d_out);
}
template<class F> inline int add_lde_batch(const uint64_t *const *d_coeffs, std::size_t n_coeffs, std::size_t batch, const uint64_t *basis, std::size_t m, const uint64_t *shift,
                                           std::size_t coset_begin, std::size_t coset_count, uint64_t *const *d_outs)
{
    return entry<F>(&subspace_ops::add_lde_batch, "add_lde_batch")(d_coeffs, n_coeffs, batch, basis, m, shift, coset_begin, coset_count, d_outs);
}
template<class F> inline int add_reextend_batch(const uint64_t *d_evals, std::size_t batch, const uint64_t *basis, std::size_t m, std::size_t d_dim, const uint64_t *eval_shift,
                                                const uint64_t *shift, std::size_t coset_begin, std::size_t coset_count, uint64_t *const *d_outs)
{
    return entry<F>(&subspace_ops::add_reextend_batch, "add_reextend_batch")(d_evals, batch, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}
template<class F> inline int add_reextend_lde_batch(const uint64_t *d_evals, std::size_t batch, const uint64_t *const *d_coeffs, std::size_t n_coeffs, std::size_t n_polys,
                                                    const uint64_t *basis, std::size_t m, std::size_t d_dim, const uint64_t *eval_shift, const uint64_t *shift,
                                                    std::size_t coset_begin, std::size_t coset_count, uint64_t *const *d_outs)
{
    return entry<F>(&subspace_ops::add_reextend_lde_batch, "add_reextend_lde_batch")(d_evals, batch, d_coeffs, n_coeffs, n_polys, basis, m, d_dim, eval_shift, shift, coset_begin,
                                                                                     coset_count, d_outs);
}
template<class F> inline int add_reextend2_batch(const uint64_t *d_evals_a, std::size_t batch_a, const uint64_t *eval_shift_a, const uint64_t *d_evals_b, std::size_t batch_b,
                                                 const uint64_t *eval_shift_b, const uint64_t *basis, std::size_t m, std::size_t d_dim, const uint64_t *shift,
                                                 std::size_t coset_begin, std::size_t coset_count, uint64_t *const *d_outs)
{
    return entry<F>(&subspace_ops::add_reextend2_batch, "add_reextend2_batch")(d_evals_a, batch_a, eval_shift_a, d_evals_b, batch_b, eval_shift_b, basis, m, d_dim, shift,
                                                                               coset_begin, coset_count, d_outs);
}
// d_out[j] = d_in[j] / Z_S(x_j) over D, S = span(D.basis[0..sub_dim)) + sub_shift
template<class F> inline int div_by_vanishing(const domain &D, const uint64_t *d_in, std::size_t sub_dim, const uint64_t *sub_shift, uint64_t *d_out)
{
    if (!subspace<F>(D, "div_by_vanishing")) missing("div_by_vanishing (multiplicative coset)", F::vec->name);
    return entry<F>(&subspace_ops::div_by_vanishing, "div_by_vanishing")(d_in, D.basis, D.dim, D.shift, sub_dim, sub_shift, d_out);
}
// Z_S(x) and Z_S's linear coefficient on the host (either output may be null)
template<class F> inline int vanishing_host(const domain &S, const uint64_t *x, uint64_t *value_out, uint64_t *linear_coefficient_out)
{
    if (!subspace<F>(S, "vanishing_host")) missing("vanishing_host (multiplicative coset)", F::vec->name);
    return entry<F>(&subspace_ops::vanishing_host, "vanishing_host")(S.basis, S.dim, S.shift, x, value_out, linear_coefficient_out);
}
template<class F> inline int fri_fold_add(const uint64_t *d_f, const uint64_t *basis, std::size_t m, const uint64_t *shift, std::size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    return entry<F>(&subspace_ops::fri_fold_add, "fri_fold_add")(d_f, basis, m, shift, coset_size, x_i, d_next);
}
template<class F> inline int fri_domains(const uint64_t *basis, std::size_t m, const uint64_t *shift, const std::size_t *localization, std::size_t num_reductions, uint64_t *out_bases,
                                         uint64_t *out_shifts)
{
    return entry<F>(&subspace_ops::fri_domains, "fri_domains")(basis, m, shift, localization, num_reductions, out_bases, out_shifts);
}

template<class F> inline int ldt_combine(const domain &L, const void *const *d_oracles, std::size_t num_oracles, const std::size_t *degrees, const uint64_t *coefficients, uint64_t *d_out)
{
    if (subspace<F>(L, "ldt_combine")) return entry<F>(&subspace_ops::ldt_combine, "ldt_combine")(d_oracles, num_oracles, degrees, coefficients, L.basis, L.dim, L.shift, d_out);
    return entry<F>(&prime_field_ops::ldt_combine, "ldt_combine")(d_oracles, num_oracles, degrees, coefficients, L.dim, L.gen, L.shift, d_out);
}
template<class F> inline int rowcheck(const domain &L, const uint64_t *d_Az, const uint64_t *d_Bz, const uint64_t *d_Cz, std::size_t h_dim, const uint64_t *h_shift, uint64_t *d_out)
{
    if (subspace<F>(L, "rowcheck")) return entry<F>(&subspace_ops::rowcheck, "rowcheck")(d_Az, d_Bz, d_Cz, L.basis, L.dim, L.shift, h_dim, h_shift, d_out);
    return entry<F>(&prime_field_ops::rowcheck, "rowcheck")(d_Az, d_Bz, d_Cz, L.dim, L.gen, L.shift, h_dim, h_shift, d_out);
}
template<class F> inline int fz(const domain &L, const domain &I, const uint64_t *d_fw, const uint64_t *d_f1v, uint64_t *d_out)
{
    if (subspace<F>(L, "fz")) return entry<F>(&subspace_ops::fz, "fz")(d_fw, d_f1v, L.basis, L.dim, L.shift, I.basis, I.dim, I.shift, d_out);
    return entry<F>(&prime_field_ops::fz, "fz")(d_fw, d_f1v, L.dim, L.gen, L.shift, I.dim, I.shift, d_out);
}
template<class F> inline int sumcheck_g(const domain &L, const domain &H, const uint64_t *d_f, const uint64_t *d_h, const uint64_t *claimed_sum, uint64_t *d_out)
{
    if (subspace<F>(L, "sumcheck_g")) return entry<F>(&subspace_ops::sumcheck_g, "sumcheck_g")(d_f, d_h, L.basis, L.dim, L.shift, H.basis, H.dim, H.shift, claimed_sum, d_out);
    return entry<F>(&prime_field_ops::sumcheck_g, "sumcheck_g")(d_f, d_h, L.dim, L.gen, L.shift, H.dim, H.shift, claimed_sum, d_out);
}
template<class F> inline int poly_div_vanishing(const domain &D, const uint64_t *d_poly, std::size_t n_coeffs, uint64_t *d_quotient)
{
    if (subspace<F>(D, "poly_div_vanishing")) return entry<F>(&subspace_ops::poly_div_vanishing, "poly_div_vanishing")(d_poly, n_coeffs, D.basis, D.dim, D.shift, d_quotient);
    return entry<F>(&prime_field_ops::poly_div_vanishing, "poly_div_vanishing")(d_poly, n_coeffs, D.dim, D.shift, d_quotient);
}
template<class F> inline int domain_offsets(const domain &D, const uint64_t *point, uint64_t *d_out)
{
    if (subspace<F>(D, "domain_offsets")) return entry<F>(&subspace_ops::domain_offsets, "domain_offsets")(D.basis, D.dim, D.shift, point, d_out);
    return entry<F>(&prime_field_ops::domain_offsets, "domain_offsets")(D.dim, D.gen, D.shift, point, d_out);
}
template<class F> inline int vanishing_evals(const domain &D, const domain &S, const uint64_t *constant, uint64_t *d_out)
{
    if (subspace<F>(D, "vanishing_evals")) return entry<F>(&subspace_ops::vanishing_evals, "vanishing_evals")(D.basis, D.dim, D.shift, S.basis, S.dim, S.shift, constant, d_out);
    return entry<F>(&prime_field_ops::vanishing_evals, "vanishing_evals")(D.dim, D.gen, D.shift, S.dim, S.shift, constant, d_out);
}
// d_xinv: 1 / x over L, read by the subspace arm only
template<class F> inline int rational_sumcheck_constraint(const domain &L, const uint64_t *d_p, const uint64_t *d_N, const uint64_t *d_D, const uint64_t *d_xinv, std::size_t k_dim,
                                                          const uint64_t *k_shift, const uint64_t *claimed_sum, uint64_t *d_out)
{
    if (subspace<F>(L, "rational_sumcheck_constraint"))
        return entry<F>(&subspace_ops::rational_sumcheck_constraint, "rational_sumcheck_constraint")(d_p, d_N, d_D, d_xinv, L.basis, L.dim, L.shift, k_dim, k_shift, claimed_sum, d_out);
    return entry<F>(&prime_field_ops::rational_sumcheck_constraint, "rational_sumcheck_constraint")(d_p, d_N, d_D, L.dim, L.gen, L.shift, k_dim, k_shift, claimed_sum, d_out);
}

} // namespace ops
} // namespace libiop_amd
