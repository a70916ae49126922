// GF(2^128): the element trait that gfx_additive.h (gf128.hip) and gfx_ops.h (gf128_ops.hip) are instantiated for.
#pragma once
#include <hip/hip_runtime.h>
#include "gf128_dev.h"
#include "gf128_host.h"

namespace iopx {

struct Elem128 {
    static constexpr int W = 2;                     // uint64 words per element
    struct alignas(16) mem { uint64_t w[2]; };      // the form in HBM and LDS
    typedef gf128 reg;

    template<bool A16>
    static __device__ __forceinline__ mem load(const uint64_t *p, size_t idx)
    {
        if (A16) return *reinterpret_cast<const mem *>(p + 2 * idx);
        mem r;
        r.w[0] = p[2 * idx]; r.w[1] = p[2 * idx + 1];
        return r;
    }
    template<bool A16>
    static __device__ __forceinline__ void store(uint64_t *p, size_t idx, const mem &v)
    {
        if (A16) { *reinterpret_cast<mem *>(p + 2 * idx) = v; return; }
        p[2 * idx] = v.w[0]; p[2 * idx + 1] = v.w[1];
    }
    static __device__ __forceinline__ mem zero() { mem r; r.w[0] = 0; r.w[1] = 0; return r; }
    static __device__ __forceinline__ mem one() { mem r; r.w[0] = 1; r.w[1] = 0; return r; }
    static __device__ __forceinline__ mem add(const mem &a, const mem &b) { mem r; r.w[0] = a.w[0] ^ b.w[0]; r.w[1] = a.w[1] ^ b.w[1]; return r; }
    static __device__ __forceinline__ reg unpack(const mem &a) { return g128_from(a.w[0], a.w[1]); }
    static __device__ __forceinline__ mem pack(const reg &a) { mem r; r.w[0] = g128_lo(a); r.w[1] = g128_hi(a); return r; }
    static __device__ __forceinline__ reg rmul(const reg &a, const reg &b) { return g128_mul(a, b); }
    static __device__ __forceinline__ mem mul(const mem &a, const mem &b) { return pack(g128_mul(unpack(a), unpack(b))); }
    static __device__ __forceinline__ mem inv(const mem &a) { return pack(g128_inv(unpack(a))); }

    static constexpr uint64_t MODULUS_LOW = 0x87;               // x^128 + x^7 + x^2 + x + 1 without its leading term
    static constexpr bool DIV_EUCLID = true;                    // kx_div inverts a workgroup's root by the binary Euclid: measured faster
    static constexpr bool RATIONAL_LEAN = false;                // kx_rational_combine keeps its inlined products: the lean form measured slower

    // the host side
    typedef hgf128 host;
    static const char *stem() { return "k128_"; }
    static const char *option(int i)
    {
        static const char *const names[4] = { "IOPX_GF128_TILE_BITS", "IOPX_GF128_P1_COLS", "IOPX_GF128_P2_COLS", "IOPX_GF128_P2_TOP" };
        return names[i];
    }
    static constexpr int TILE_DEFAULT = 11, TILE_MAX = 11;      // 2^11 elements = 32 KiB of LDS
    static constexpr int P1_COLS_DEFAULT = 3, P2_COLS_DEFAULT = 3, P2_TOP_DEFAULT = 3;      // 8 x 16 B = one line
    static constexpr int UPPER_WAVES = 6;                       // kx_bfly_upper: 80 registers
    static constexpr int STAGE_BITS = 24;                       // 256 MiB of staging
    static constexpr bool SPLIT_ACCESS = true;                  // 128-bit accesses where the pointers allow them
    static const char *cold_plan() { return "gf128_plan"; }
    static const char *cold_pow() { return "gf128_pow_tables"; }
    static constexpr uint64_t LDT_TAG = 0x6c6474313238;         // "ldt128"
    static constexpr uint64_t OPS_TAG = 0x6f7073313238;         // "ops128": the domain tables of gfx_ops.h
    static constexpr size_t CACHE_BYTES = (size_t)3 << 30;
};

} // namespace iopx
