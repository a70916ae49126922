// Host-side arithmetic in alt_bn128 Fr (libff Fp_model<4> Montgomery words, R = 2^256) for the O(log n) per-call
// constants of the multiplicative-domain kernels over that field (generators, inverse shift, n^-1, fold and LDT
// constants).  Never touches codeword-sized data.
#pragma once
#include <cstdint>
#include <cstring>

namespace iopx {

struct hbn {
    uint64_t w[4];
    typedef unsigned __int128 u128;
    static constexpr uint64_t P[4] = { 0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull };
    static constexpr uint64_t INV = 0xc2e1f593efffffffull;     // -p^-1 mod 2^64

    hbn() { w[0] = w[1] = w[2] = w[3] = 0; }
    static hbn from_words(const uint64_t *p) { hbn r; memcpy(r.w, p, 32); return r; }
    bool operator==(const hbn &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    bool is_zero() const { return (w[0] | w[1] | w[2] | w[3]) == 0; }

    static bool geq_p(const uint64_t *a)
    {
        for (int i = 3; i >= 0; --i) if (a[i] != P[i]) return a[i] > P[i];
        return true;
    }
    static void sub_p(uint64_t *a)
    {
        u128 borrow = 0;
        for (int i = 0; i < 4; ++i) { const u128 d = (u128)a[i] - P[i] - borrow; a[i] = (uint64_t)d; borrow = (d >> 64) & 1; }
    }
    hbn operator*(const hbn &b) const
    {
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) {
            u128 carry = 0;
            for (int j = 0; j < 4; ++j) { const u128 cur = (u128)w[j] * b.w[i] + t[j] + carry; t[j] = (uint64_t)cur; carry = cur >> 64; }
            u128 cur = (u128)t[4] + carry;
            t[4] = (uint64_t)cur; t[5] = (uint64_t)(cur >> 64);
            const uint64_t m = t[0] * INV;
            cur = (u128)m * P[0] + t[0];
            carry = cur >> 64;
            for (int j = 1; j < 4; ++j) { cur = (u128)m * P[j] + t[j] + carry; t[j - 1] = (uint64_t)cur; carry = cur >> 64; }
            cur = (u128)t[4] + carry;
            t[3] = (uint64_t)cur;
            t[4] = t[5] + (uint64_t)(cur >> 64);
        }
        hbn r; r.w[0] = t[0]; r.w[1] = t[1]; r.w[2] = t[2]; r.w[3] = t[3];
        if (t[4] || geq_p(r.w)) sub_p(r.w);
        return r;
    }
    hbn operator+(const hbn &b) const
    {
        hbn r;
        u128 carry = 0;
        for (int i = 0; i < 4; ++i) { const u128 s = (u128)w[i] + b.w[i] + carry; r.w[i] = (uint64_t)s; carry = s >> 64; }
        if (carry || geq_p(r.w)) sub_p(r.w);
        return r;
    }
    hbn operator-(const hbn &b) const
    {
        hbn r;
        u128 borrow = 0;
        for (int i = 0; i < 4; ++i) { const u128 d = (u128)w[i] - b.w[i] - borrow; r.w[i] = (uint64_t)d; borrow = (d >> 64) & 1; }
        if (borrow) { u128 carry = 0; for (int i = 0; i < 4; ++i) { const u128 t = (u128)r.w[i] + P[i] + carry; r.w[i] = (uint64_t)t; carry = t >> 64; } }
        return r;
    }
    hbn squared() const { return *this * *this; }
    // 2^k mod p as a plain integer, by doubling
    static hbn pow2_mod_p(int k)
    {
        hbn r; r.w[0] = 1;
        for (int i = 0; i < k; ++i) {
            uint64_t carry = 0;
            for (int j = 0; j < 4; ++j) { const uint64_t nc = r.w[j] >> 63; r.w[j] = (r.w[j] << 1) | carry; carry = nc; }
            if (carry || geq_p(r.w)) sub_p(r.w);
        }
        return r;
    }
    static hbn one() { return pow2_mod_p(256); }              // R mod p
    hbn pow_limbs(const uint64_t *e, int n) const
    {
        hbn r = one();
        for (int i = 64 * n - 1; i >= 0; --i) { r = r.squared(); if ((e[i / 64] >> (i % 64)) & 1) r = r * *this; }
        return r;
    }
    hbn pow(uint64_t e) const { return pow_limbs(&e, 1); }
    hbn inverse() const { uint64_t e[4] = { P[0] - 2, P[1], P[2], P[3] }; return pow_limbs(e, 4); }
    static hbn from_uint(uint64_t v)        // v * R mod p = v (raw) * R^2 * R^-1
    {
        hbn raw; raw.w[0] = v;
        return raw * pow2_mod_p(512);
    }
    // The device multiplies in Montgomery radix 2^261 (bn254_dev.h): a multiplier t is uploaded as t * 2^261 mod p, i.e. the
    // stored words of t * 2^5, so that a product with data held as x * 2^256 is again x t * 2^256.
    hbn table_form() const { return *this * from_uint(32); }
};

} // namespace iopx
