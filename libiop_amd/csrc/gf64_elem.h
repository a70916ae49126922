// GF(2^64): the element trait that gfx_additive.h (gf64.hip) and gfx_ops.h (gf64_ops.hip) are instantiated for.
#pragma once
#include <hip/hip_runtime.h>
#include "gf64_dev.h"
#include "gf64_host.h"

namespace iopx {

struct Elem64 {
    static constexpr int W = 1;                     // uint64 words per element
    typedef uint64_t mem;                           // the form in HBM and LDS
    typedef gf64 reg;

    template<bool A16> static __device__ __forceinline__ mem load(const uint64_t *p, size_t idx) { return p[idx]; }
    template<bool A16> static __device__ __forceinline__ void store(uint64_t *p, size_t idx, mem v) { p[idx] = v; }
    static __device__ __forceinline__ mem zero() { return 0; }
    static __device__ __forceinline__ mem one() { return 1; }
    static __device__ __forceinline__ mem add(mem a, mem b) { return a ^ b; }
    static __device__ __forceinline__ reg unpack(mem a) { return g64_from(a); }
    static __device__ __forceinline__ mem pack(const reg &a) { return g64_word(a); }
    static __device__ __forceinline__ reg rmul(const reg &a, const reg &b) { return g64_mul(a, b); }
    static __device__ __forceinline__ mem mul(mem a, mem b) { return g64_word(g64_mul(g64_from(a), g64_from(b))); }
    static __device__ __forceinline__ mem inv(mem a) { return g64_word(g64_inv(g64_from(a))); }

    static constexpr uint64_t MODULUS_LOW = 0x1B;               // x^64 + x^4 + x^3 + x + 1 without its leading term
    static constexpr bool DIV_EUCLID = true;                    // kx_div inverts a workgroup's root by the binary Euclid: measured faster
    static constexpr bool RATIONAL_LEAN = false;                // kx_rational_combine keeps its inlined products: one form over a one-word element

    // the host side
    typedef hgf64 host;
    static const char *stem() { return "k64_"; }
    static const char *option(int i)
    {
        static const char *const names[4] = { "IOPX_GF64_TILE_BITS", "IOPX_GF64_P1_COLS", "IOPX_GF64_P2_COLS", "IOPX_GF64_P2_TOP" };
        return names[i];
    }
    static constexpr int TILE_DEFAULT = 12, TILE_MAX = 12;      // 2^12 elements = 32 KiB of LDS
    static constexpr int P1_COLS_DEFAULT = 4, P2_COLS_DEFAULT = 4, P2_TOP_DEFAULT = 4;      // 16 x 8 B = one line
    static constexpr int UPPER_WAVES = 1;                       // kx_bfly_upper: 66 registers, no occupancy to bound them to
    static constexpr int STAGE_BITS = 25;                       // 256 MiB of staging
    static constexpr bool SPLIT_ACCESS = false;                 // an element is one 64-bit word
    static const char *cold_plan() { return "gf64_plan"; }
    static const char *cold_pow() { return "gf64_pow_tables"; }
    static constexpr uint64_t LDT_TAG = 0x6c64743634;           // "ldt64"
    static constexpr uint64_t OPS_TAG = 0x6f70733634;           // "ops64": the domain tables of gfx_ops.h
    static constexpr size_t CACHE_BYTES = (size_t)3 << 30;
};

} // namespace iopx
