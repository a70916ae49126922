// GF(2^256): the element trait that gfx_additive.h (gf256.hip) and gfx_ops.h (gf256_ops.hip) are instantiated for.
#pragma once
#include <hip/hip_runtime.h>
#include "gf256_dev.h"
#include "gf256_host.h"

namespace iopx {

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

    static constexpr uint64_t MODULUS_LOW = 0x425;               // x^256 + x^10 + x^5 + x^2 + 1 without its leading term
    static constexpr bool DIV_EUCLID = true;                    // kx_div inverts a workgroup's root by the binary Euclid: measured faster
    static constexpr bool RATIONAL_LEAN = true;                 // kx_rational_combine_lean is the rational combination's form: measured faster

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
    static constexpr uint64_t OPS_TAG = 0x6f7073323536;         // "ops256": the domain tables of gfx_ops.h
    static constexpr size_t CACHE_BYTES = (size_t)6 << 30;      // the same dimensions as gf128's 3 GiB at twice the element
};

} // namespace iopx
