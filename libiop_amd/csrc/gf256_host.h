// Host-side GF(2^256) arithmetic (x^256 + x^10 + x^5 + x^2 + 1) used only to prepare the per-domain constants (recursed bases, shifts,
// fold multipliers, subspace polynomials: O(m^2) field operations per plan).  Portable C++: the hot path runs on the GPU.
#pragma once
#include <cstdint>
#include <cstring>

namespace iopx {

struct hgf256 {
    uint64_t w[4];

    hgf256() : w{ 0, 0, 0, 0 } {}
    explicit hgf256(const uint64_t *p) : w{ p[0], p[1], p[2], p[3] } {}
    static hgf256 zero() { return hgf256(); }
    static hgf256 one() { hgf256 r; r.w[0] = 1; return r; }

    void store(uint64_t *p) const { for (int i = 0; i < 4; ++i) p[i] = w[i]; }
    bool is_zero() const { return (w[0] | w[1] | w[2] | w[3]) == 0; }
    bool operator==(const hgf256 &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    bool operator!=(const hgf256 &o) const { return !(*this == o); }

    hgf256 operator+(const hgf256 &o) const { hgf256 r; for (int i = 0; i < 4; ++i) r.w[i] = w[i] ^ o.w[i]; return r; }
    hgf256 &operator+=(const hgf256 &o) { for (int i = 0; i < 4; ++i) w[i] ^= o.w[i]; return *this; }

    // 512 -> 256 bits: H (1 + x^2 + x^5 + x^10), then the at most 10 bits that pushes past bit 255
    static hgf256 reduce(const uint64_t (&c)[8])
    {
        hgf256 r;
        uint64_t prev = 0;
        for (int j = 0; j < 4; ++j) {
            const uint64_t h = c[4 + j];
            r.w[j] = c[j] ^ h ^ ((h << 2) | (prev >> 62)) ^ ((h << 5) | (prev >> 59)) ^ ((h << 10) | (prev >> 54));
            prev = h;
        }
        const uint64_t t = (prev >> 62) ^ (prev >> 59) ^ (prev >> 54);
        r.w[0] ^= t ^ (t << 2) ^ (t << 5) ^ (t << 10);
        return r;
    }

    hgf256 operator*(const hgf256 &o) const
    {
        uint64_t c[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int v = 0; v < 4; ++v) {
            for (int i = 0; i < 64; ++i) {
                if (!((o.w[v] >> i) & 1)) continue;
                for (int k = 0; k < 4; ++k) {
                    c[v + k] ^= w[k] << i;
                    if (i) c[v + k + 1] ^= w[k] >> (64 - i);
                }
            }
        }
        const uint64_t c8[8] = { c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7] };      // c[8] stays zero: the product has 511 bits
        return reduce(c8);
    }
    hgf256 &operator*=(const hgf256 &o) { *this = *this * o; return *this; }

    hgf256 squared() const
    {
        uint64_t c[8];
        for (int i = 0; i < 8; ++i) {
            uint64_t x = (w[i >> 1] >> (32 * (i & 1))) & 0xffffffffull;
            x = (x | (x << 16)) & 0x0000ffff0000ffffull;
            x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
            x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
            x = (x | (x << 2)) & 0x3333333333333333ull;
            x = (x | (x << 1)) & 0x5555555555555555ull;
            c[i] = x;
        }
        return reduce(c);
    }

    // a^(2^256 - 2) = (a^(2^255 - 1))^2, Itoh–Tsujii chain on 255: beta_k = a^(2^k - 1), beta_2k = beta_k^(2^k) beta_k, beta_(k+1) = beta_k^2 a
    hgf256 inverse() const
    {
        hgf256 beta = *this;
        int k = 1;
        for (int bit = 6; bit >= 0; --bit) {        // 255 = 0b11111111
            hgf256 t = beta;
            for (int i = 0; i < k; ++i) t = t.squared();
            beta = t * beta;
            k *= 2;
            if ((255 >> bit) & 1) { beta = beta.squared() * *this; k += 1; }
        }
        return beta.squared();
    }
};

} // namespace iopx
