// GF(2^64) = GF(2)[x]/(x^64 + x^4 + x^3 + x + 1) on gfx950 (CDNA4).
//
// Element layout in HBM is libff gf64's in-memory layout: one little-endian uint64 word, polynomial basis.  gfx950 has no carry-less
// multiply: the 64x64 product is Karatsuba over the two 32-bit halves on the 32x32 product "with holes" of gf192_dev.h (three word
// products, 48 integer multiplies), then a two-step fold of the 127-bit result.  About 0.13k VALU ops against ~1.0k for a gf192 product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gf192_dev.h"

struct gf64 {
    uint32_t w[2];
};

__device__ __forceinline__ gf64 g64_from(uint64_t v)
{
    gf64 r;
    r.w[0] = (uint32_t)v; r.w[1] = (uint32_t)(v >> 32);
    return r;
}

__device__ __forceinline__ uint64_t g64_word(const gf64 &v)
{
    return (uint64_t)v.w[0] | ((uint64_t)v.w[1] << 32);
}

__device__ __forceinline__ gf64 g64_add(const gf64 &a, const gf64 &b)
{
    gf64 r;
    r.w[0] = a.w[0] ^ b.w[0]; r.w[1] = a.w[1] ^ b.w[1];
    return r;
}

// Fold a 4-word (127-bit) carry-less product modulo x^64 + x^4 + x^3 + x + 1: with H = c[2..3] the result is L + H (1 + x + x^3 + x^4)
// and a second fold of the at most 4 bits (64..67) that the first one pushes past bit 63.  Word j of H << s is one v_alignbit.
__device__ __forceinline__ gf64 g64_reduce(const uint32_t (&c)[4])
{
    gf64 r;
    uint32_t prev = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t h = c[2 + j];
        const uint32_t s1 = gf_funnel(h, prev, 1), s3 = gf_funnel(h, prev, 3), s4 = gf_funnel(h, prev, 4);
        r.w[j] = xor3(xor3(c[j], h, s1), s3, s4);
        prev = h;
    }
    const uint32_t t = (prev >> 31) ^ (prev >> 29) ^ (prev >> 28);      // bits 64..67 of H (1 + x + x^3 + x^4)
    r.w[0] ^= t ^ (t << 1) ^ (t << 3) ^ (t << 4);
    return r;
}

__device__ __forceinline__ gf64 g64_mul(const gf64 &a, const gf64 &b)
{
    const holes4 a0 = holes_split(a.w[0]), a1 = holes_split(a.w[1]), b0 = holes_split(b.w[0]), b1 = holes_split(b.w[1]);
    uint32_t d0l, d0h, d1l, d1h, ml, mh;
    clmul32_holes(a0, b0, d0l, d0h);
    clmul32_holes(a1, b1, d1l, d1h);
    clmul32_holes(holes_add(a0, a1), holes_add(b0, b1), ml, mh);
    // (a0 + a1 X)(b0 + b1 X) = d0 + X (m + d0 + d1) + X^2 d1,  X = x^32
    uint32_t c[4];
    c[0] = d0l;
    c[1] = d0h ^ xor3(ml, d0l, d1l);
    c[2] = d1l ^ xor3(mh, d0h, d1h);
    c[3] = d1h;
    return g64_reduce(c);
}

// squaring is GF(2)-linear: bit i moves to bit 2i, then the reduction
__device__ __forceinline__ gf64 g64_sqr(const gf64 &a)
{
    uint32_t c[4];
    c[0] = gf_spread16(a.w[0] & 0xFFFFu); c[1] = gf_spread16(a.w[0] >> 16);
    c[2] = gf_spread16(a.w[1] & 0xFFFFu); c[3] = gf_spread16(a.w[1] >> 16);
    return g64_reduce(c);
}

// a^(2^64 - 2) = (a^(2^63 - 1))^2 by the Itoh-Tsujii chain on 63 = 0b111111: 63 squarings + 10 products; zero maps to zero
__device__ inline gf64 g64_inv(const gf64 &a)
{
    gf64 beta = a;                          // beta_k = a^(2^k - 1)
    int k = 1;
    for (int bit = 4; bit >= 0; --bit) {
        gf64 t = beta;
        for (int i = 0; i < k; ++i) t = g64_sqr(t);
        beta = g64_mul(t, beta);            // beta_2k
        k *= 2;
        if ((63 >> bit) & 1) { beta = g64_mul(g64_sqr(beta), a); k += 1; }
    }
    return g64_sqr(beta);
}
