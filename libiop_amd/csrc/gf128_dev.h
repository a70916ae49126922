// GF(2^128) = GF(2)[x]/(x^128 + x^7 + x^2 + x + 1) on gfx950 (CDNA4).
//
// Element layout in HBM is libff gf128's in-memory layout: two little-endian uint64 words, polynomial basis.  The 128x128 product is
// Karatsuba over the two 64-bit halves, each 64x64 product Karatsuba over its 32-bit halves as in g64_mul: nine word products on the
// 32x32 product "with holes" of gf192_dev.h (144 integer multiplies), then the two-step fold of the 255-bit result.  About 0.47k VALU ops
// against ~0.13k for a gf64 product and ~1.0k for a gf192 one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gf192_dev.h"

struct gf128 {
    uint32_t w[4];
};

__device__ __forceinline__ gf128 g128_from(uint64_t lo, uint64_t hi)
{
    gf128 r;
    r.w[0] = (uint32_t)lo; r.w[1] = (uint32_t)(lo >> 32); r.w[2] = (uint32_t)hi; r.w[3] = (uint32_t)(hi >> 32);
    return r;
}

__device__ __forceinline__ uint64_t g128_lo(const gf128 &v) { return (uint64_t)v.w[0] | ((uint64_t)v.w[1] << 32); }
__device__ __forceinline__ uint64_t g128_hi(const gf128 &v) { return (uint64_t)v.w[2] | ((uint64_t)v.w[3] << 32); }

__device__ __forceinline__ gf128 g128_add(const gf128 &a, const gf128 &b)
{
    gf128 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = a.w[i] ^ b.w[i];
    return r;
}

// Fold an 8-word (255-bit) carry-less product modulo x^128 + x^7 + x^2 + x + 1: with H = c[4..7] the result is L + H (1 + x + x^2 + x^7)
// and a second fold of the at most 7 bits (128..134) that the first one pushes past bit 127.  Word j of H << s is one v_alignbit.
__device__ __forceinline__ gf128 g128_reduce(const uint32_t (&c)[8])
{
    gf128 r;
    uint32_t prev = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t h = c[4 + j];
        const uint32_t s1 = gf_funnel(h, prev, 1), s2 = gf_funnel(h, prev, 2), s7 = gf_funnel(h, prev, 7);
        r.w[j] = xor3(xor3(c[j], h, s1), s2, s7);
        prev = h;
    }
    const uint32_t t = (prev >> 31) ^ (prev >> 30) ^ (prev >> 25);      // bits 128..134 of H (1 + x + x^2 + x^7)
    r.w[0] ^= t ^ (t << 1) ^ (t << 2) ^ (t << 7);
    return r;
}

// 2 x 2 words -> 4 words: the Karatsuba step of g64_mul.  The sums are formed on the WORDS and every word product splits its own two
// operands into the hole form (clmul32_words, as gf_mul_lean does): splitting all eight input words up front costs 64 VGPRs before the
// first multiply and put the butterfly kernels at 157 registers; this form keeps them under 80.
__device__ __forceinline__ void clmul64_words(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t (&c)[4])
{
    uint32_t d0l, d0h, d1l, d1h, ml, mh;
    clmul32_words(a0, b0, d0l, d0h);
    clmul32_words(a1, b1, d1l, d1h);
    clmul32_words(a0 ^ a1, b0 ^ b1, ml, mh);
    // (a0 + a1 X)(b0 + b1 X) = d0 + X (m + d0 + d1) + X^2 d1,  X = x^32
    c[0] = d0l;
    c[1] = d0h ^ xor3(ml, d0l, d1l);
    c[2] = d1l ^ xor3(mh, d0h, d1h);
    c[3] = d1h;
}

__device__ __forceinline__ gf128 g128_mul(const gf128 &a, const gf128 &b)
{
    uint32_t p0[4], p1[4], p2[4];
    clmul64_words(a.w[0], a.w[1], b.w[0], b.w[1], p0);
    clmul64_words(a.w[2], a.w[3], b.w[2], b.w[3], p2);
    clmul64_words(a.w[0] ^ a.w[2], a.w[1] ^ a.w[3], b.w[0] ^ b.w[2], b.w[1] ^ b.w[3], p1);
    // (A0 + A1 Y)(B0 + B1 Y) = P0 + Y (P1 + P0 + P2) + Y^2 P2,  Y = x^64
    uint32_t c[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = p0[i]; c[4 + i] = p2[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) c[2 + i] ^= xor3(p1[i], p0[i], p2[i]);
    return g128_reduce(c);
}

// squaring is GF(2)-linear: bit i moves to bit 2i, then the reduction
__device__ __forceinline__ gf128 g128_sqr(const gf128 &a)
{
    uint32_t c[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[2 * i] = gf_spread16(a.w[i] & 0xFFFFu); c[2 * i + 1] = gf_spread16(a.w[i] >> 16); }
    return g128_reduce(c);
}

// a^(2^128 - 2) = (a^(2^127 - 1))^2 by the Itoh-Tsujii chain on 127 = 0b1111111: 127 squarings + 12 products; zero maps to zero
__device__ inline gf128 g128_inv(const gf128 &a)
{
    gf128 beta = a;                         // beta_k = a^(2^k - 1)
    int k = 1;
    for (int bit = 5; bit >= 0; --bit) {
        gf128 t = beta;
        for (int i = 0; i < k; ++i) t = g128_sqr(t);
        beta = g128_mul(t, beta);           // beta_2k
        k *= 2;
        if ((127 >> bit) & 1) { beta = g128_mul(g128_sqr(beta), a); k += 1; }
    }
    return g128_sqr(beta);
}
