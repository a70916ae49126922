// GF(2^256) on gfx950: additive FFT / IFFT / low-degree extension, FRI fold and domain chain, LDT combination, vector helpers.
//
// The transforms replace additive_FFT / additive_IFFT of the reference (libiop/algebra/fft.tcc:39-124, 126-204) for FieldT = libff::gf256
// (x^256 + x^10 + x^5 + x^2 + 1, four words).  The kernels, the host driver and the bodies of the entries are gfx_additive.h, instantiated
// here for Elem256: an element travels as F::mem, a 32-byte block (two 128-bit accesses when every pointer of the
// launch is 16-byte aligned, four 64-bit words otherwise: the profile reports the latter as k256_*_w64).  The LDS tile is an array of
// 32-byte elements.
#include <hip/hip_runtime.h>
#include "gf256_dev.h"
#include "gf256_host.h"
#include "runtime.h"

namespace iopx {

// ---------------------------------------------------------------------------------------------
// the element trait
// ---------------------------------------------------------------------------------------------
struct Elem256 {
    static constexpr int W = 4;                     // uint64 words per element
    struct alignas(16) mem { uint64_t w[4]; };      // the form in HBM and LDS
    typedef gf256 reg;

    template<bool A16>
    static __device__ __forceinline__ mem load(const uint64_t *p, size_t idx)
    {
        if (A16) return *reinterpret_cast<const mem *>(p + 4 * idx);
        mem r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r.w[i] = p[4 * idx + i];
        return r;
    }
    template<bool A16>
    static __device__ __forceinline__ void store(uint64_t *p, size_t idx, const mem &v)
    {
        if (A16) { *reinterpret_cast<mem *>(p + 4 * idx) = v; return; }
#pragma unroll
        for (int i = 0; i < 4; ++i) p[4 * idx + i] = v.w[i];
    }
    static __device__ __forceinline__ mem zero() { mem r; r.w[0] = 0; r.w[1] = 0; r.w[2] = 0; r.w[3] = 0; return r; }
    static __device__ __forceinline__ mem one() { mem r; r.w[0] = 1; r.w[1] = 0; r.w[2] = 0; r.w[3] = 0; return r; }
    static __device__ __forceinline__ mem add(const mem &a, const mem &b)
    {
        mem r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r.w[i] = a.w[i] ^ b.w[i];
        return r;
    }
    static __device__ __forceinline__ reg unpack(const mem &a) { return g256_from(a.w[0], a.w[1], a.w[2], a.w[3]); }
    static __device__ __forceinline__ mem pack(const reg &a)
    {
        mem r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r.w[i] = g256_word(a, i);
        return r;
    }
    static __device__ __forceinline__ reg rmul(const reg &a, const reg &b) { return g256_mul(a, b); }
    static __device__ __forceinline__ mem mul(const mem &a, const mem &b) { return pack(g256_mul(unpack(a), unpack(b))); }
    static __device__ __forceinline__ mem inv(const mem &a) { return pack(g256_inv(unpack(a))); }

    // the host side
    typedef hgf256 host;
    static const char *stem() { return "k256_"; }
    static const char *option(int i)
    {
        static const char *const names[4] = { "IOPX_GF256_TILE_BITS", "IOPX_GF256_P1_COLS", "IOPX_GF256_P2_COLS", "IOPX_GF256_P2_TOP" };
        return names[i];
    }
    static constexpr int TILE_DEFAULT = 10, TILE_MAX = 11;      // 2^10 elements = 32 KiB of LDS; 2^11 = 64 KiB, the cap
    static constexpr int P1_COLS_DEFAULT = 2, P2_TOP_DEFAULT = 2;       // 4 x 32 B = one line
    static constexpr int P2_COLS_DEFAULT = 3;                   // the upper passes gain from runs of two lines
    static constexpr int UPPER_WAVES = 6;                       // kx_bfly_upper: 74 registers, gf128's bound holds
    static constexpr int STAGE_BITS = 24;                       // 512 MiB of staging
    static constexpr bool SPLIT_ACCESS = true;                  // 128-bit accesses where the pointers allow them
    static const char *cold_plan() { return "gf256_plan"; }
    static const char *cold_pow() { return "gf256_pow_tables"; }
    static constexpr uint64_t LDT_TAG = 0x6c6474323536;         // "ldt256"
    static constexpr size_t CACHE_BYTES = (size_t)6 << 30;      // the same dimensions as gf128's 3 GiB at twice the element
};

} // namespace iopx

#include "gfx_additive.h"

namespace iopx {
void clear_gf256_plans() { clear_plans_x<Elem256>(); }
} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_add_lde_gf256_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                           const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *d_out)
{
    return x_add_lde_dev<Elem256>(d_coeffs, n_coeffs, basis, m, shift, coset_begin, coset_count, d_out);
}

int iopx_add_fft_gf256_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                           const uint64_t *shift, uint64_t *d_out)
{
    return x_add_fft_dev<Elem256>(d_coeffs, n_coeffs, basis, m, shift, d_out);
}

int iopx_add_ifft_gf256_dev(const uint64_t *d_evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                            uint64_t *d_out)
{
    return x_add_ifft_dev<Elem256>(d_evals, basis, m, shift, d_out);
}

int iopx_add_fft_gf256(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                       const uint64_t *shift, uint64_t *out)
{
    return x_add_fft_host<Elem256>(coeffs, n_coeffs, basis, m, shift, out);
}

int iopx_add_ifft_gf256(const uint64_t *evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                        uint64_t *out)
{
    return x_add_ifft_host<Elem256>(evals, basis, m, shift, out);
}

int iopx_fri_fold_add_gf256_dev(const uint64_t *d_f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                                size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    return x_fri_fold_add_dev<Elem256>(d_f_i, basis, m, shift, coset_size, x_i, d_next);
}

int iopx_fri_fold_add_gf256(const uint64_t *f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                            size_t coset_size, const uint64_t *x_i, uint64_t *next)
{
    return x_fri_fold_add_host<Elem256>(f_i, basis, m, shift, coset_size, x_i, next);
}

int iopx_fri_domains_gf256(const uint64_t *basis, size_t m, const uint64_t *shift, const size_t *localization, size_t num_reductions,
                           uint64_t *out_bases, uint64_t *out_shifts)
{
    return x_fri_domains<Elem256>(basis, m, shift, localization, num_reductions, out_bases, out_shifts);
}

int iopx_ldt_combine_gf256_dev(const void *const *d_oracles, size_t num_oracles, const size_t *degrees,
                               const uint64_t *random_coefficients, const uint64_t *basis, size_t m, const uint64_t *shift,
                               uint64_t *d_out)
{
    return x_ldt_combine_dev<Elem256>(d_oracles, num_oracles, degrees, random_coefficients, basis, m, shift, d_out);
}

int iopx_gf256_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return x_mul_dev<Elem256>(d_a, d_b, d_out, count); }
int iopx_gf256_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count) { return x_inv_dev<Elem256>(d_a, d_out, count); }
int iopx_gf256_add_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return x_add_dev<Elem256>(d_a, d_b, d_out, count); }
int iopx_gf256_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { return x_host_mul<Elem256>(a, b, out); }
int iopx_gf256_inverse_host(const uint64_t *x, uint64_t *out) { return x_inverse_host<Elem256>(x, out); }

} // extern "C"
