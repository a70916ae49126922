// GF(2^256) = GF(2)[x]/(x^256 + x^10 + x^5 + x^2 + 1) on gfx950 (CDNA4).
//
// Element layout in HBM is libff gf256's in-memory layout: four little-endian uint64 words, polynomial basis.  The 256x256 product is
// Karatsuba over the two 128-bit halves, each 128x128 product the Karatsuba step of g128_mul over its 64-bit words: nine 64x64 products,
// each of them clmul64_words (three 32x32 products "with holes"), 27 word products in all against 9 for gf128 and 18 for gf192.  The
// 511-bit result folds in two steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gf128_dev.h"

struct gf256 {
    uint32_t w[8];
};

__device__ __forceinline__ gf256 g256_from(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3)
{
    gf256 r;
    r.w[0] = (uint32_t)w0; r.w[1] = (uint32_t)(w0 >> 32); r.w[2] = (uint32_t)w1; r.w[3] = (uint32_t)(w1 >> 32);
    r.w[4] = (uint32_t)w2; r.w[5] = (uint32_t)(w2 >> 32); r.w[6] = (uint32_t)w3; r.w[7] = (uint32_t)(w3 >> 32);
    return r;
}

__device__ __forceinline__ uint64_t g256_word(const gf256 &v, int i) { return (uint64_t)v.w[2 * i] | ((uint64_t)v.w[2 * i + 1] << 32); }

__device__ __forceinline__ gf256 g256_add(const gf256 &a, const gf256 &b)
{
    gf256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = a.w[i] ^ b.w[i];
    return r;
}

// Fold a 16-word (511-bit) carry-less product modulo x^256 + x^10 + x^5 + x^2 + 1: with H = c[8..15] the result is
// L + H (1 + x^2 + x^5 + x^10) and a second fold of the at most 10 bits (256..265) that the first one pushes past bit 255.
// Word j of H << s is one v_alignbit.
__device__ __forceinline__ gf256 g256_reduce(const uint32_t (&c)[16])
{
    gf256 r;
    uint32_t prev = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t h = c[8 + j];
        const uint32_t s2 = gf_funnel(h, prev, 2), s5 = gf_funnel(h, prev, 5), s10 = gf_funnel(h, prev, 10);
        r.w[j] = xor3(xor3(c[j], h, s2), s5, s10);
        prev = h;
    }
    const uint32_t t = (prev >> 30) ^ (prev >> 27) ^ (prev >> 22);      // bits 256..265 of H (1 + x^2 + x^5 + x^10)
    r.w[0] ^= t ^ (t << 2) ^ (t << 5) ^ (t << 10);
    return r;
}

// 4 x 4 words -> 8 words: the Karatsuba step of g128_mul without its reduction.  As there, the sums are formed on the words and every
// word product splits its own operands.
__device__ __forceinline__ void clmul128_words(const uint32_t (&a)[4], const uint32_t (&b)[4], uint32_t (&c)[8])
{
    uint32_t p0[4], p1[4], p2[4];
    clmul64_words(a[0], a[1], b[0], b[1], p0);
    clmul64_words(a[2], a[3], b[2], b[3], p2);
    clmul64_words(a[0] ^ a[2], a[1] ^ a[3], b[0] ^ b[2], b[1] ^ b[3], p1);
    // (A0 + A1 Y)(B0 + B1 Y) = P0 + Y (P1 + P0 + P2) + Y^2 P2,  Y = x^64
#pragma unroll
    for (int i = 0; i < 4; ++i) { c[i] = p0[i]; c[4 + i] = p2[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) c[2 + i] ^= xor3(p1[i], p0[i], p2[i]);
}

__device__ __forceinline__ gf256 g256_mul(const gf256 &a, const gf256 &b)
{
    uint32_t c[16], mid[8];
    {
        const uint32_t al[4] = { a.w[0], a.w[1], a.w[2], a.w[3] }, bl[4] = { b.w[0], b.w[1], b.w[2], b.w[3] };
        uint32_t q[8];
        clmul128_words(al, bl, q);
#pragma unroll
        for (int i = 0; i < 8; ++i) { c[i] = q[i]; mid[i] = q[i]; }
    }
    {
        const uint32_t ah[4] = { a.w[4], a.w[5], a.w[6], a.w[7] }, bh[4] = { b.w[4], b.w[5], b.w[6], b.w[7] };
        uint32_t q[8];
        clmul128_words(ah, bh, q);
#pragma unroll
        for (int i = 0; i < 8; ++i) { c[8 + i] = q[i]; mid[i] ^= q[i]; }
    }
    {
        const uint32_t am[4] = { a.w[0] ^ a.w[4], a.w[1] ^ a.w[5], a.w[2] ^ a.w[6], a.w[3] ^ a.w[7] };
        const uint32_t bm[4] = { b.w[0] ^ b.w[4], b.w[1] ^ b.w[5], b.w[2] ^ b.w[6], b.w[3] ^ b.w[7] };
        uint32_t q[8];
        clmul128_words(am, bm, q);
        // (A0 + A1 Z)(B0 + B1 Z) = Q0 + Z (Q1 + Q0 + Q2) + Z^2 Q2,  Z = x^128
#pragma unroll
        for (int i = 0; i < 8; ++i) c[4 + i] ^= mid[i] ^ q[i];
    }
    return g256_reduce(c);
}

// squaring is GF(2)-linear: bit i moves to bit 2i, then the reduction
__device__ __forceinline__ gf256 g256_sqr(const gf256 &a)
{
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { c[2 * i] = gf_spread16(a.w[i] & 0xFFFFu); c[2 * i + 1] = gf_spread16(a.w[i] >> 16); }
    return g256_reduce(c);
}

// a^(2^256 - 2) = (a^(2^255 - 1))^2 by the Itoh-Tsujii chain on 255 = 0b11111111: 255 squarings + 14 products; zero maps to zero.
// The chain is one rolled loop of fourteen steps with a single product in its body — an even step doubles (beta_2k = beta_k^(2^k) beta_k),
// an odd one adds one (beta_(k+1) = beta_k^2 a): with two inlined products per iteration (g128_inv's form) the scheduler takes every
// register and spills.
__device__ inline gf256 g256_inv(const gf256 &a)
{
    gf256 beta = a;                         // beta_k = a^(2^k - 1)
    int k = 1;
#pragma unroll 1
    for (int step = 0; step < 14; ++step) {
        const bool plus_one = step & 1;
        const int n = plus_one ? 1 : k;
        gf256 t = beta, o;
#pragma unroll 1
        for (int i = 0; i < n; ++i) t = g256_sqr(t);
#pragma unroll
        for (int i = 0; i < 8; ++i) o.w[i] = plus_one ? a.w[i] : beta.w[i];
        beta = g256_mul(t, o);
        k = plus_one ? k + 1 : 2 * k;
    }
    return g256_sqr(beta);
}
