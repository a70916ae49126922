// Host-side GF(2^128) arithmetic (x^128 + x^7 + x^2 + x + 1) used only to prepare the per-domain constants (recursed bases, shifts,
// fold multipliers, subspace polynomials: O(m^2) field operations per plan).  Portable C++: the hot path runs on the GPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace iopx {

struct hgf128 {
    uint64_t lo, hi;

    hgf128() : lo(0), hi(0) {}
    hgf128(uint64_t l, uint64_t h) : lo(l), hi(h) {}
    explicit hgf128(const uint64_t *w) : lo(w[0]), hi(w[1]) {}
    static hgf128 zero() { return hgf128(); }
    static hgf128 one() { return hgf128(1, 0); }

    void store(uint64_t *w) const { w[0] = lo; w[1] = hi; }
    bool is_zero() const { return (lo | hi) == 0; }
    bool operator==(const hgf128 &o) const { return lo == o.lo && hi == o.hi; }
    bool operator!=(const hgf128 &o) const { return !(*this == o); }

    hgf128 operator+(const hgf128 &o) const { return hgf128(lo ^ o.lo, hi ^ o.hi); }
    hgf128 &operator+=(const hgf128 &o) { lo ^= o.lo; hi ^= o.hi; return *this; }

    // 256 -> 128 bits: H (1 + x + x^2 + x^7), then the at most 7 bits that pushes past bit 127
    static hgf128 reduce(const uint64_t (&c)[4])
    {
        const uint64_t h0 = c[2], h1 = c[3];
        uint64_t l0 = c[0] ^ h0 ^ (h0 << 1) ^ (h0 << 2) ^ (h0 << 7);
        const uint64_t l1 = c[1] ^ h1 ^ ((h1 << 1) | (h0 >> 63)) ^ ((h1 << 2) | (h0 >> 62)) ^ ((h1 << 7) | (h0 >> 57));
        const uint64_t t = (h1 >> 63) ^ (h1 >> 62) ^ (h1 >> 57);
        l0 ^= t ^ (t << 1) ^ (t << 2) ^ (t << 7);
        return hgf128(l0, l1);
    }

    hgf128 operator*(const hgf128 &o) const
    {
        uint64_t c[4] = { 0, 0, 0, 0 };
        const uint64_t a[2] = { lo, hi }, b[2] = { o.lo, o.hi };
        for (int w = 0; w < 2; ++w) {
            for (int i = 0; i < 64; ++i) {
                if (!((b[w] >> i) & 1)) continue;
                for (int k = 0; k < 2; ++k) {
                    c[w + k] ^= a[k] << i;
                    if (i) c[w + k + 1] ^= a[k] >> (64 - i);
                }
            }
        }
        return reduce(c);
    }
    hgf128 &operator*=(const hgf128 &o) { *this = *this * o; return *this; }

    hgf128 squared() const
    {
        uint64_t c[4];
        for (int i = 0; i < 4; ++i) {
            uint64_t x = ((i < 2 ? lo : hi) >> (32 * (i & 1))) & 0xffffffffull;
            x = (x | (x << 16)) & 0x0000ffff0000ffffull;
            x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
            x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
            x = (x | (x << 2)) & 0x3333333333333333ull;
            x = (x | (x << 1)) & 0x5555555555555555ull;
            c[i] = x;
        }
        return reduce(c);
    }

    // a^(2^128 - 2) = (a^(2^127 - 1))^2, Itoh–Tsujii chain on 127: beta_k = a^(2^k - 1), beta_2k = beta_k^(2^k) beta_k, beta_(k+1) = beta_k^2 a
    hgf128 inverse() const
    {
        hgf128 beta = *this;
        int k = 1;
        for (int bit = 5; bit >= 0; --bit) {        // 127 = 0b1111111
            hgf128 t = beta;
            for (int i = 0; i < k; ++i) t = t.squared();
            beta = t * beta;
            k *= 2;
            if ((127 >> bit) & 1) { beta = beta.squared() * *this; k += 1; }
        }
        return beta.squared();
    }
};

} // namespace iopx
