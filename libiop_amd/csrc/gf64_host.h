// Host-side GF(2^64) arithmetic (x^64 + x^4 + x^3 + x + 1) used only to prepare the per-domain constants (recursed bases, shifts,
// fold multipliers, subspace polynomials: O(m^2) field operations per plan).  Portable C++: the hot path runs on the GPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "subspace_poly.h"

namespace iopx {

struct hgf64 {
    uint64_t v;

    hgf64() : v(0) {}
    explicit hgf64(uint64_t x) : v(x) {}
    explicit hgf64(const uint64_t *w) : v(w[0]) {}     // from an element's words, as the wider fields' host types
    void store(uint64_t *out) const { out[0] = v; }
    static hgf64 zero() { return hgf64(); }
    static hgf64 one() { return hgf64(1); }

    bool is_zero() const { return v == 0; }
    bool operator==(const hgf64 &o) const { return v == o.v; }
    bool operator!=(const hgf64 &o) const { return v != o.v; }

    hgf64 operator+(const hgf64 &o) const { return hgf64(v ^ o.v); }
    hgf64 &operator+=(const hgf64 &o) { v ^= o.v; return *this; }

    // 128 -> 64 bits: H (1 + x + x^3 + x^4), then the at most 4 bits that pushes past bit 63
    static uint64_t reduce(uint64_t lo, uint64_t hi)
    {
        lo ^= hi ^ (hi << 1) ^ (hi << 3) ^ (hi << 4);
        const uint64_t t = (hi >> 63) ^ (hi >> 61) ^ (hi >> 60);
        return lo ^ t ^ (t << 1) ^ (t << 3) ^ (t << 4);
    }

    hgf64 operator*(const hgf64 &o) const
    {
        uint64_t lo = 0, hi = 0;
        for (int i = 0; i < 64; ++i) {
            if ((o.v >> i) & 1) { lo ^= v << i; if (i) hi ^= v >> (64 - i); }
        }
        return hgf64(reduce(lo, hi));
    }
    hgf64 &operator*=(const hgf64 &o) { *this = *this * o; return *this; }

    hgf64 squared() const
    {
        uint64_t c[2];
        for (int i = 0; i < 2; ++i) {
            uint64_t x = (v >> (32 * i)) & 0xffffffffull;
            x = (x | (x << 16)) & 0x0000ffff0000ffffull;
            x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
            x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
            x = (x | (x << 2)) & 0x3333333333333333ull;
            x = (x | (x << 1)) & 0x5555555555555555ull;
            c[i] = x;
        }
        return hgf64(reduce(c[0], c[1]));
    }

    // a^(2^64 - 2) = (a^(2^63 - 1))^2, Itoh–Tsujii chain on 63: beta_k = a^(2^k - 1), beta_2k = beta_k^(2^k) beta_k, beta_(k+1) = beta_k^2 a
    hgf64 inverse() const
    {
        hgf64 beta = *this;
        int k = 1;
        for (int bit = 4; bit >= 0; --bit) {        // 63 = 0b111111
            hgf64 t = beta;
            for (int i = 0; i < k; ++i) t = t.squared();
            beta = t * beta;
            k *= 2;
            if ((63 >> bit) & 1) { beta = beta.squared() * *this; k += 1; }
        }
        return beta.squared();
    }
};

typedef SubspacePolyX<hgf64> SubspacePoly64;

} // namespace iopx
